// srt_host_c.cpp -- the plain-C handles srt_host_c.h declares (the comment on each function is there).  No compute here.
#include "srt_host_c.h"

#include <cstring>
#include <string>

#include "srt_host.h"
#include "srt_host_internal.h"

using namespace srt_host;

static thread_local std::string g_err;

// Exceptions never cross the boundary: every function that can throw runs its body here, which records the message for
// srth_last_error and returns the failure value of the function's kind -- -1 (status, count), nullptr (handle), 1 (srth_decode_image).
// Bare, because they cannot throw: srth_last_error, the four *_free, srth_set_build_tasks, srth_flat_desc, srth_flat_names, the
// Renderer's fast-path getter and setter, srth_radians and the srth_mat_* helpers.
template <class T, class F> static T guard(T fail, F&& body) {
    try { return body(); }
    catch (const std::exception& e) { g_err = e.what(); }
    catch (...) { g_err = "unknown"; }
    return fail;
}
template <class F> static int status(F&& body) { return guard(-1, [&] { body(); return 0; }); }

static ObjectManager* OM(void* om) { return (ObjectManager*)om; }
static vec2 frame_size(uint32_t W, uint32_t H) { return vec2((float)W, (float)H); }

// what the render calls return: the count of emitted pixels, and, unless rgb is NULL, the dense H x W x 3 image
static int64_t image_to_dense(const ImageData& d, uint32_t W, uint32_t H, float* rgb) {
    if (!rgb) return (int64_t)d.imagePoints.size();
    std::memset(rgb, 0, (size_t)W * H * 3 * sizeof(float));
    for (size_t i = 0; i < d.imagePoints.size(); i++) {
        const size_t x = (size_t)d.imagePoints[i].x, y = (size_t)d.imagePoints[i].y;
        float* c = rgb + (y * W + x) * 3;
        c[0] = d.imageColors[i].x; c[1] = d.imageColors[i].y; c[2] = d.imageColors[i].z;
    }
    return (int64_t)d.imagePoints.size();
}
template <class F> static int64_t frame(uint32_t W, uint32_t H, float* rgb, F&& render) {
    return guard((int64_t)-1, [&] { return image_to_dense(render(), W, H, rgb); });
}

static void set_texcoords(Triangle& t, const float* tc) {
    t.colorOneCoordinate = vec2(tc[0], tc[1]); t.colorTwoCoordinate = vec2(tc[2], tc[3]); t.colorThreeCoordinate = vec2(tc[4], tc[5]);
}

extern "C" {

const char* srth_last_error() { return g_err.c_str(); }

// ---- ObjectManager -------------------------------------------------------------------------------
void* srth_om_new() { return guard((void*)nullptr, [&]() -> void* { return new ObjectManager(); }); }
void srth_om_free(void* om) { delete OM(om); }
int srth_om_load_obj(void* om, const char* name) { return status([&] { OM(om)->loadObjFile(name); }); }

int srth_om_add_object(void* om_, const char* name, uint32_t n, const float* points) {
    return status([&] {
        ObjectManager* om = OM(om_);
        om->objColors[name] = vec3(1.f, 0.f, 0.f);
        om->objProperties[name] = vec3(0.2f, 0.5f, 15.0f);
        std::vector<Triangle>& tris = om->objTriangles[name];      // filled in place: a 69 k-triangle object is 10 MB of Triangle
        tris.clear(); tris.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const float* p = points + (size_t)i * 12;
            tris[i].pointOne = vec4(p[0], p[1], p[2], p[3]); tris[i].pointTwo = vec4(p[4], p[5], p[6], p[7]); tris[i].pointThree = vec4(p[8], p[9], p[10], p[11]);
            tris[i].color = vec3(1.f, 1.f, 1.f);
        }
    });
}
int srth_decode_image(const char* path, int32_t* w, int32_t* h, uint8_t* rgb) {
    return guard(1, [&] {
        Texture t;
        if (!load_texture(path, t)) return 1;
        *w = t.dim.x; *h = t.dim.y;
        if (rgb) std::memcpy(rgb, t.rgb.data(), t.rgb.size());
        return 0;
    });
}
int srth_om_add_texture(void* om, const char* texname, int32_t w, int32_t h, const uint8_t* rgb) {
    return status([&] {
        Texture t; t.dim.x = w; t.dim.y = h; t.rgb.assign(rgb, rgb + (size_t)w * h * 3);
        OM(om)->textureData[texname] = std::move(t);
    });
}
int srth_om_add_textured_object(void* om, const char* name, uint32_t n, const float* points, const float* texcoord, const char* texname) {
    int rc = srth_om_add_object(om, name, n, points);
    if (rc) return rc;
    return status([&] {
        std::vector<Triangle>& tris = OM(om)->objTriangles[name];
        for (uint32_t i = 0; i < n; i++) { set_texcoords(tris[i], texcoord + (size_t)i * 6); tris[i].textureName = texname; }
    });
}
int srth_om_add_multi_textured_object(void* om, const char* name, uint32_t n, const float* points, const float* texcoord,
                                      const int32_t* tri_tex, const char* names) {
    int rc = srth_om_add_object(om, name, n, points);
    if (rc) return rc;
    return status([&] {
        std::vector<std::string> list;
        for (const char* p = names; *p;) { const char* e = std::strchr(p, '\n'); if (!e) e = p + std::strlen(p); list.emplace_back(p, e); p = *e ? e + 1 : e; }
        std::vector<Triangle>& tris = OM(om)->objTriangles[name];
        for (uint32_t i = 0; i < n; i++) {
            if (tri_tex[i] < 0) continue;
            set_texcoords(tris[i], texcoord + (size_t)i * 6);
            tris[i].textureName = list.at((size_t)tri_tex[i]);
        }
    });
}
int srth_om_clone(void* om, const char* src, const char* dst) {
    return status([&] { std::vector<Triangle> t = OM(om)->getTriangles(src); OM(om)->objTriangles[dst] = t; });
}
int srth_om_set_color(void* om, const char* name, float r, float g, float b) { return status([&] { OM(om)->setColor(name, vec3(r, g, b)); }); }
int srth_om_set_props(void* om, const char* name, float ka, float ks, float sh) { return status([&] { OM(om)->objProperties[name] = vec3(ka, ks, sh); }); }
int srth_om_transform(void* om, const char* name, const float* m) { return status([&] { OM(om)->transformTriangles(name, mat4_from_floats(m)); }); }
void srth_set_build_tasks(int on) { setHierarchyBuildTasks(on != 0); }
int srth_sort_keys_both_ways(const float* keys, uint32_t n, uint32_t* order_parallel, uint32_t* order_std) {
    return status([&] { sort_keys_both_ways(keys, n, order_parallel, order_std); });
}
int srth_om_build_bvh(void* om, const char* name) { return status([&] { OM(om)->createBoundingHierarchy(name); }); }
int64_t srth_om_num_tris(void* om, const char* name) { return guard((int64_t)-1, [&] { return (int64_t)OM(om)->getTriangles(name).size(); }); }
int srth_om_get_points(void* om, const char* name, float* out) {
    return status([&] {
        const std::vector<Triangle>& v = OM(om)->getTriangles(name);
        for (size_t i = 0; i < v.size(); i++) {
            const vec4* p[3] = { &v[i].pointOne, &v[i].pointTwo, &v[i].pointThree };
            for (int k = 0; k < 3; k++) for (int c = 0; c < 4; c++) out[(i * 3 + k) * 4 + c] = (*p[k])[c];
        }
    });
}
int64_t srth_om_hierarchy_nodes(void* om, const char* name) {
    return guard((int64_t)-1, [&] { return (int64_t)OM(om)->boundingVolumeHierarchy.at(name).nodes.size(); });
}
int srth_om_hierarchy(void* om, const char* name, float* points, uint32_t* order, float* node_min, float* node_max) {
    return status([&] {
        const ObjectManager::Hierarchy& h = OM(om)->boundingVolumeHierarchy.at(name);
        std::memcpy(points, h.points.data(), h.points.size() * sizeof(float));
        std::memcpy(order, h.order.data(), h.order.size() * sizeof(uint32_t));
        std::memcpy(node_min, h.node_min.data(), h.node_min.size() * sizeof(float));
        std::memcpy(node_max, h.node_max.data(), h.node_max.size() * sizeof(float));
    });
}
int srth_om_get_tri_attrs(void* om, const char* name, float* texcoord, float* color, int32_t* has_tex, float* normals) {
    return status([&] {
        const std::vector<Triangle>& v = OM(om)->getTriangles(name);
        for (size_t i = 0; i < v.size(); i++) {
            const vec2* tc[3] = { &v[i].colorOneCoordinate, &v[i].colorTwoCoordinate, &v[i].colorThreeCoordinate };
            for (int k = 0; k < 3; k++) { texcoord[i * 6 + k * 2] = tc[k]->x; texcoord[i * 6 + k * 2 + 1] = tc[k]->y; }
            color[i * 3] = v[i].color.x; color[i * 3 + 1] = v[i].color.y; color[i * 3 + 2] = v[i].color.z;
            has_tex[i] = v[i].textureName.empty() ? 0 : 1;
            const vec3* nn[3] = { &v[i].normalOne, &v[i].normalTwo, &v[i].normalThree };
            for (int k = 0; k < 3; k++) for (int c = 0; c < 3; c++) normals[i * 9 + k * 3 + c] = (*nn[k])[c];
        }
    });
}

// ---- flattener ---------------------------------------------------------------------------------
void* srth_flatten(void* om) { return guard((void*)nullptr, [&]() -> void* { return new FlatScene(flattenScene(OM(om))); }); }
void srth_flat_free(void* f) { delete (FlatScene*)f; }
void srth_flat_desc(void* f, srt_scene_desc* out) { *out = ((FlatScene*)f)->desc(); }
uint32_t srth_flat_names(void* f_, char* buf, uint32_t cap) {      // every name followed by '\n', cut to cap - 1 characters, NUL-terminated
    const FlatScene* f = (const FlatScene*)f_;
    uint32_t at = 0;
    auto put = [&](char c) { if (at + 1 < cap) buf[at++] = c; };
    for (const std::string& n : f->names) { for (char c : n) put(c); put('\n'); }
    if (cap) buf[at] = 0;
    return (uint32_t)f->names.size();
}

// ---- drop-in entry point (GPU) + writer -----------------------------------------------------------
int64_t srth_render(void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, int device, float* rgb) {
    return frame(W, H, rgb, [&] { return sendRaysAndIntersectPointsColors(frame_size(W, H), light_vec4(light4), OM(om), light_amount, device); });
}
int srth_write_bmp(const char* path, uint32_t W, uint32_t H, const uint8_t* rgb) { return status([&] { writeBmp(path, W, H, rgb); }); }

// ---- Transformation.h factories + the glm ops main() applies --------------------------------------
float srth_radians(float d) { return radians(d); }
void srth_mat_scale(float x, float y, float z, float* m) { mat4_to_floats(Transformation::scaleObj(x, y, z), m); }
void srth_mat_rotx(float a, float* m) { mat4_to_floats(Transformation::rotateObjX(a), m); }
void srth_mat_roty(float a, float* m) { mat4_to_floats(Transformation::rotateObjY(a), m); }
void srth_mat_rotz(float a, float* m) { mat4_to_floats(Transformation::rotateObjZ(a), m); }
void srth_mat_mirror(int x, int y, int z, float* m) { mat4_to_floats(Transformation::mirrorObj(x, y, z), m); }
void srth_mat_shear(float xy, float xz, float yx, float yz, float zx, float zy, float* m) { mat4_to_floats(Transformation::shearObj(xy, xz, yx, yz, zx, zy), m); }
void srth_mat_translate(float x, float y, float z, float* m) { mat4_to_floats(Transformation::changeObjPosition(vec3(x, y, z)), m); }
void srth_mat_view(const float* pos, const float* rot, float* m) { mat4_to_floats(Transformation::createViewMatrix(vec3(pos[0], pos[1], pos[2]), vec3(rot[0], rot[1], rot[2])), m); }
void srth_mat_inverse(const float* a, float* m) { mat4_to_floats(inverse(mat4_from_floats(a)), m); }
void srth_mat_mul(const float* a, const float* b, float* m) { mat4_to_floats(mat4_from_floats(a) * mat4_from_floats(b), m); }
void srth_mat_mul_vec4(const float* a, const float* v, float* out) { vec4 r = mat4_from_floats(a) * light_vec4(v); std::memcpy(out, &r.x, 16); }

// ---- Renderer: a device scene kept across frames (srt_host.h) ------------------------------------------------------------
void* srth_renderer_new(int device) { return guard((void*)nullptr, [&]() -> void* { return new Renderer(device); }); }
void srth_renderer_free(void* r) { delete (Renderer*)r; }
uint64_t srth_renderer_fast_frames(void* r) { return ((Renderer*)r)->fastFrames(); }
void srth_renderer_set_fast_path(void* r, int on) { ((Renderer*)r)->setFastPath(on != 0); }
int64_t srth_renderer_render(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, float* rgb) {
    return frame(W, H, rgb, [&] { return ((Renderer*)r)->render(frame_size(W, H), light_vec4(light4), OM(om), light_amount); });
}
int srth_renderer_submit(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount) {
    return status([&] { ((Renderer*)r)->submit(frame_size(W, H), light_vec4(light4), OM(om), light_amount); });
}
int64_t srth_renderer_collect(void* r, uint32_t W, uint32_t H, float* rgb) {
    return frame(W, H, rgb, [&] { return ((Renderer*)r)->collect(); });
}
int64_t srth_renderer_render_from_camera(void* r, void* om, uint32_t W, uint32_t H, const float* light4_world, const float* view16,
                                         int light_amount, int scene_changed, float* rgb) {
    return frame(W, H, rgb, [&] {
        return ((Renderer*)r)->renderFromCamera(frame_size(W, H), light_vec4(light4_world), mat4_from_floats(view16), OM(om), light_amount, scene_changed != 0);
    });
}
int64_t srth_renderer_render_posed(void* r, void* om, uint32_t W, uint32_t H, const float* light4, const float* mats, uint32_t n_mats,
                                   int light_amount, int scene_changed, float* rgb) {
    return frame(W, H, rgb, [&] {
        std::vector<mat4> ms(n_mats);
        for (uint32_t k = 0; k < n_mats; k++) ms[k] = mat4_from_floats(mats + 16 * (size_t)k);
        return ((Renderer*)r)->renderPosed(frame_size(W, H), light_vec4(light4), ms, OM(om), light_amount, scene_changed != 0);
    });
}

// ---- MultiRenderer: several devices, one process (the framebuffer split on the C++ host) -------------------------------------
void* srth_multi_new(const int* devices, uint32_t n, uint32_t block_rows) {
    return guard((void*)nullptr, [&]() -> void* { return new MultiRenderer(std::vector<int>(devices, devices + n), block_rows); });
}
void srth_multi_free(void* r) { delete (MultiRenderer*)r; }
int64_t srth_multi_render(void* r, void* om, uint32_t W, uint32_t H, const float* light4, int light_amount, float* rgb) {
    return frame(W, H, rgb, [&] { return ((MultiRenderer*)r)->render(frame_size(W, H), light_vec4(light4), OM(om), light_amount); });
}

} // extern "C"
