/* srt_host_c.h -- plain-C handles over srt_host.h (libsrt_host.so) so that Python (ctypes) tests, bench.py and other FFI users can
 * drive the host-side mirror.  No compute here; exceptions never cross the boundary.
 *
 * Handles are void*: an ObjectManager (om), a FlatScene (flat), a Renderer or a MultiRenderer (r).  A function that can fail returns
 * -1 (status and counts) or NULL (handles) and leaves its message for srth_last_error(), per thread; srth_decode_image returns 1.
 * Matrices are 16 floats, column-major (glm::mat4 memory order).  simple_raytracer_amd/host.py mirrors this file (PROTOTYPES, in
 * this order), and tests/test_host_abi_mirror.py holds the two together. */
#ifndef SRT_HOST_C_H
#define SRT_HOST_C_H

#include <stdint.h>

#include "../../../include/srt.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* srth_last_error(void);

/* ---- ObjectManager ----------------------------------------------------------------------------- */
void* srth_om_new(void);
void srth_om_free(void* om);
int srth_om_load_obj(void* om, const char* name);
/* Object fed from arrays with the loader's defaults (Object.cpp:29-34, 81-84) */
int srth_om_add_object(void* om, const char* name, uint32_t n, const float* points);
/* decode an image file as the loader does; rgb == NULL: dimensions only.  Returns 0, or 1 if the file does not decode. */
int srth_decode_image(const char* path, int32_t* w, int32_t* h, uint8_t* rgb);
/* Array-fed textured object: the state loadObjFile leaves for a textured mesh (Object.cpp:98-161) */
int srth_om_add_texture(void* om, const char* texname, int32_t w, int32_t h, const uint8_t* rgb);
int srth_om_add_textured_object(void* om, const char* name, uint32_t n, const float* points, const float* texcoord, const char* texname);
/* object with several textures (house.obj): per triangle an index into the newline-separated `names`, -1 = untextured */
int srth_om_add_multi_textured_object(void* om, const char* name, uint32_t n, const float* points, const float* texcoord,
                                      const int32_t* tri_tex, const char* names);
/* objTriangles[dst] = getTriangles(src), as main() clones objects (simple_raytracer.cpp:565,597,644) */
int srth_om_clone(void* om, const char* src, const char* dst);
int srth_om_set_color(void* om, const char* name, float r, float g, float b);
int srth_om_set_props(void* om, const char* name, float ka, float ks, float sh);
int srth_om_transform(void* om, const char* name, const float* m);
void srth_set_build_tasks(int on);
int srth_sort_keys_both_ways(const float* keys, uint32_t n, uint32_t* order_parallel, uint32_t* order_std);
int srth_om_build_bvh(void* om, const char* name);
int64_t srth_om_num_tris(void* om, const char* name);
int srth_om_get_points(void* om, const char* name, float* out);
/* the hierarchy of an object as srt_scene_update_frame takes it: node count, then points (n x 12, source order, at build time), the
 * build's permutation (n), node boxes (m x 3 each, pre-order) */
int64_t srth_om_hierarchy_nodes(void* om, const char* name);
int srth_om_hierarchy(void* om, const char* name, float* points, uint32_t* order, float* node_min, float* node_max);
int srth_om_get_tri_attrs(void* om, const char* name, float* texcoord, float* color, int32_t* has_tex, float* normals);

/* ---- flattener --------------------------------------------------------------------------------- */
void* srth_flatten(void* om);
void srth_flat_free(void* flat);
void srth_flat_desc(void* flat, srt_scene_desc* out);
uint32_t srth_flat_names(void* flat, char* buf, uint32_t cap);

/* ---- drop-in entry point (GPU) + writer -------------------------------------------------------- */
/* Dense H x W x 3 float image like oracle/ref_harness.cpp's ref_render: 0 where nothing was emitted. */
int64_t srth_render(void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, int device, float* rgb);
int srth_write_bmp(const char* path, uint32_t W, uint32_t H, const uint8_t* rgb);

/* ---- Transformation.h factories + the glm ops main() applies ----------------------------------- */
float srth_radians(float d);
void srth_mat_scale(float x, float y, float z, float* m);
void srth_mat_rotx(float a, float* m);
void srth_mat_roty(float a, float* m);
void srth_mat_rotz(float a, float* m);
void srth_mat_mirror(int x, int y, int z, float* m);
void srth_mat_shear(float xy, float xz, float yx, float yz, float zx, float zy, float* m);
void srth_mat_translate(float x, float y, float z, float* m);
void srth_mat_view(const float* pos, const float* rot, float* m);
void srth_mat_inverse(const float* a, float* m);
void srth_mat_mul(const float* a, const float* b, float* m);
void srth_mat_mul_vec4(const float* a, const float* v, float* out);

/* ---- Renderer: a device scene kept across frames (srt_host.h) ---------------------------------- */
void* srth_renderer_new(int device);
void srth_renderer_free(void* r);
uint64_t srth_renderer_fast_frames(void* r);
void srth_renderer_set_fast_path(void* r, int on);
/* rgb = NULL: the frame is rendered and collected but not written out densely (timing runs) */
int64_t srth_renderer_render(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, float* rgb);
int srth_renderer_submit(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount);
int64_t srth_renderer_collect(void* r, uint32_t W, uint32_t H, float* rgb);
int64_t srth_renderer_render_from_camera(void* r, void* om, uint32_t W, uint32_t H, const float* light4_world, const float* view16,
                                         int light_amount, int scene_changed, float* rgb);
/* pose: mats = n_mats x 16 floats, column-major, one per object in the scene's object order */
int64_t srth_renderer_render_posed(void* r, void* om, uint32_t W, uint32_t H, const float* light4, const float* mats, uint32_t n_mats,
                                   int light_amount, int scene_changed, float* rgb);

/* ---- MultiRenderer: several devices, one process (the framebuffer split on the C++ host) ------- */
void* srth_multi_new(const int* devices, uint32_t n, uint32_t block_rows);
void srth_multi_free(void* r);
int64_t srth_multi_render(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, float* rgb);

#ifdef __cplusplus
}
#endif
#endif
