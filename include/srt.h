/* include/srt.h -- C ABI of the MI355X-native ray-trace core for simple_raytracer scenes.
 *
 * This is the drop-in boundary for ONE path of leonlang/simple_raytracer: the per-pixel loop
 *
 *     ImageData sendRaysAndIntersectPointsColors(const glm::vec2& imageSize,
 *                                                const glm::vec4& lightPos,
 *                                                ObjectManager* objManager);   // simple_raytracer.cpp:505
 *
 * called once per frame from main() (simple_raytracer.cpp:784) and consumed by drawImage (:793).
 * The reference has no FFI of its own; the seam is that one call.  Everything here is plain C:
 * PODs, caller-owned buffers, int return codes, no exceptions, no glm / STL / torch types.
 * All compute behind these entry points is hand-written HIP for gfx950; there is NO CPU fallback
 * (the CPU restatement used to check results lives in oracle/ and is test infrastructure only).
 *
 * Thread-safety: one host thread per srt_scene handle.  One handle lives on one HIP device.
 */
#ifndef SRT_H
#define SRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_ABI_VERSION 3

/* ---- error codes (the reference signals nothing: it prints, throws or crashes) -- */
enum {
    SRT_OK              = 0,
    SRT_ERR_ARG         = 1,   /* null pointer / zero size / inconsistent counts                    */
    SRT_ERR_LAYOUT      = 2,   /* scene arrays violate the layout contract below                    */
    SRT_ERR_DEVICE      = 3,   /* HIP runtime error (srt_last_hip_error() has the hipError_t)       */
    SRT_ERR_NO_GPU      = 4,   /* no HIP device visible: the product path never falls back to CPU   */
    SRT_ERR_TEXTURE     = 5,   /* triangle references a texture id >= n_textures                    */
    SRT_ERR_LIMIT       = 6,   /* size exceeds an implementation limit (n_tris < 2^26, n_nodes < 2^26) */
    SRT_ERR_OOM         = 7    /* host allocation failed (std::bad_alloc caught at the boundary)    */
};
/* No entry point lets a C++ exception escape: bad_alloc -> SRT_ERR_OOM, anything else -> SRT_ERR_DEVICE. */

/* ---- flat scene: what the host hands over once per frame ---------------------------------------
 * It is the reference's ObjectManager state (Object.h:59-89) with the string-keyed maps and Node*
 * trees written out as arrays:
 *   objects    in objTriangles iteration order (the order rayIntersection:409 visits them),
 *   nodes      each object's Node tree (Object.h:46-57) in any order, children by global index,
 *   triangles  in VISIT order: object order -> DFS left-first leaf order (boundingBoxIntersection
 *              :296-317) -> in-leaf order.  The index in this order is the canonical triangle id
 *              reported in hit_id, and ties in t resolve to the lowest id exactly as the reference's
 *              strict '<' (:429) does.
 * Layout contract (checked, SRT_ERR_LAYOUT): every node is reachable from exactly one root; a leaf
 * has left == right == -1 and owns triangles [first, first+count), 0 <= count; walking all objects'
 * trees DFS left-first meets the leaves' ranges contiguously in increasing order, covering
 * [0, n_tris) exactly once; tri_obj[i] equals the object whose tree owns triangle i.
 */
typedef struct srt_scene_desc {
    uint32_t n_objects, n_nodes, n_tris, n_textures;
    /* nodes: Node::minBox / maxBox (Object.h:47-48), left / right (:50-51) */
    const float*    node_min;      /* n_nodes x 3                                                   */
    const float*    node_max;      /* n_nodes x 3                                                   */
    const int32_t*  node_left;     /* n_nodes, global child index or -1                             */
    const int32_t*  node_right;    /* n_nodes                                                       */
    const int32_t*  node_first;    /* n_nodes, first triangle of a leaf (ignored for inner nodes)   */
    const int32_t*  node_count;    /* n_nodes, triangle count of a leaf (ignored for inner nodes)   */
    const uint32_t* obj_root;      /* n_objects, root node of each object's tree                    */
    /* triangles: Triangle::pointOne/Two/Three (Object.h:17-19) as raw homogeneous xyzw             */
    const float*    tri_points;    /* n_tris x 3 x 4                                                */
    const int32_t*  tri_obj;       /* n_tris, owning object                                         */
    const int32_t*  tri_tex;       /* n_tris, texture id or -1 (Triangle::textureName empty)        */
    const float*    tri_texcoord;  /* n_tris x 6, colorOne/Two/ThreeCoordinate (Object.h:23-25):    */
                                   /* integer texel coords stored as floats; may be NULL if no tex  */
    const float*    tri_normals;   /* n_tris x 9 vertex normals (Object.h:20-22) or NULL; only read */
                                   /* with SRT_FLAG_SMOOTH_NORMALS                                   */
    /* objects: objColors / objProperties (Object.h:64,68) */
    const float*    obj_color;     /* n_objects x 3                                                 */
    const float*    obj_material;  /* n_objects x 3: ambient, specularStrength, shininess           */
    /* textures: textureData / textureDimensions (Object.h:70-71), 8-bit RGB rows top-down          */
    const uint8_t*  tex_rgb;       /* concatenated                                                  */
    const uint64_t* tex_off;       /* n_textures byte offsets into tex_rgb                          */
    const uint32_t* tex_w;         /* n_textures                                                    */
    const uint32_t* tex_h;         /* n_textures                                                    */
} srt_scene_desc;

/* ---- render parameters: every compile-time literal of the reference path, as data -------------- */
enum {
    SRT_FLAG_NONE           = 0,
    SRT_FLAG_SMOOTH_NORMALS = 1u << 0,  /* interpolateNormal (simple_raytracer.cpp:132-140) instead of the flat face
                                         * normal: the line the reference keeps commented out at :162; needs
                                         * srt_scene_desc.tri_normals.  The function is pinned by a reference KAT,
                                         * the images only by the oracle (the reference cannot render this mode) */
    SRT_FLAG_COUNT_WORK     = 1u << 1,  /* run the counting build: fills node/tri test counters      */
    SRT_FLAG_NO_TIMING      = 1u << 2,  /* record no HIP events: for launches captured into a hipGraph (an even number
                                         * of renders per graph keeps the two alternating counter sets in step)     */
    SRT_FLAG_FRAMES_IN_FLIGHT = 1u << 3 /* a HINT, results do not depend on it: this frame is one of several the caller keeps in
                                         * flight on the device (other streams, other handles).  Launches of a fixed number of
                                         * waves that pull work (the shadow rays of 16+ light samples) then keep only as many waves
                                         * as the frame's work can feed and leave the rest of the machine to the other frames; a
                                         * frame that has the device to itself wants every wave (1080p, 16 samples: 12-16 % faster
                                         * with the hint on four streams, 11-23 % slower with it on one).  With 1..7 light
                                         * samples the fused trace launch then runs two waves of 8x4 pixels per 8x8 tile instead
                                         * of four of 4x4 -- waves that live longer and leave the launch a longer tail, which the
                                         * next frame fills (1080p, 1 sample: 18 % faster with the hint on four streams, 24 %
                                         * slower if a single stream were given that form)                                 */
};

typedef struct srt_params {
    uint32_t width, height;        /* imageSize (simple_raytracer.cpp:773)                          */
    /* scanline blocks rendered by THIS call: blocks of block_rows rows; this call owns blocks
     * block_first, block_first+block_stride, ...  Output row r_local = k*block_rows + (y % block_rows)
     * for the k-th owned block.  Whole frame on one device: block_rows = height, first 0, stride 1. */
    uint32_t block_rows, block_first, block_stride;
    /* block_cols = 0: full-width scanline blocks, as above.  block_cols = C > 0 (C and block_rows multiples of 8): the frame is cut
     * into tiles of block_rows x C pixels and tile (bx, by) belongs to the call with (bx + by) % block_stride == block_first -- a
     * diagonal deal, so that every call owns tiles in every block row and every block column (expensive pixels cluster: tree crowns,
     * a bunny; whole-width rows spread them over 8 devices only coarsely).  Output: `height` rows x srt_cols_owned(p) columns; local
     * column xl of image row y is image column ((xl / C) * block_stride + (block_first + block_stride - (y / block_rows) %
     * block_stride) % block_stride) * C + xl % C, and local columns whose image column is >= width are padding (not written). */
    uint32_t block_cols;
    float    focal;                /* 400 (:506)                                                    */
    uint32_t n_lights;             /* lightAmount (:348,445)                                        */
    const float* light_pos;        /* n_lights x 3, host-accumulated staircase (:372-382)           */
    /* NULL = the reference's frame: the scene has been transformed into camera space (main() applies inverse(viewMatrix) to every
     * triangle each frame, simple_raytracer.cpp:558 etc.) and rays leave the origin.  Non-NULL = CAMERA MODE, an opt-in EXTENSION
     * (SURVEY.md s8 f1): the scene and the light stay where they are, the hierarchy is built once, and the camera moves instead --
     * 16 floats, column-major like glm::mat4, the matrix M that takes a camera-space ray into the scene's space (for the
     * reference's scenes: M = the viewMatrix whose inverse main() applies to the triangles).  Ray origin = M[3].xyz, direction =
     * (M[0] * dx + M[1] * dy) + M[2] * dz with (dx, dy, dz) the reference's (i, j, focal).  Same geometry, different rounding:
     * results are pinned by the oracle run in the same mode, not by the reference. */
    const float* ray_matrix;
    float    shadow_div;           /* 5   (:369)                                                    */
    float    reinhard;             /* 0.5 (:391)                                                    */
    float    gamma;                /* 1.1 (:396)                                                    */
    uint8_t  background[4];        /* 173,216,230 (:476); [3] unused                                */
    uint32_t spp;                  /* 1 = reference.  n*n > 1 = EXTENSION (the reference has no supersampling):
                                    * regular n x n sub-pixel grid, offsets (k+0.5)/n - 0.5 added to dir.xy, the
                                    * sub-frames' pre-tone-map sums added in order, divided by spp, tone-mapped
                                    * once; hit_id / t report sub-sample 0                            */
    uint32_t flags;                /* SRT_FLAG_* in bits 0..7; bits 8..15: kernel-variant selector for A/B measurements and
                                    * the parity tests (0 = the shipped pipeline; the others compute the same results with
                                    * older or differently configured kernels; `enum Variant` in
                                    * simple_raytracer_amd/csrc/srt_hip.hip is the list of the numbers)                  */
} srt_params;
/* TILE SPANS.  A whole frame in the reference's ray form with 1..7 light samples (the fused pipeline, variant 0) starts trace
 * workgroups only for the 8x8 tiles that the projection of the objects' root boxes can reach -- per tile row one span of tiles,
 * computed on the host from the boxes of the last srt_scene_create / srt_scene_update / srt_scene_update_frame -- and the shading
 * launch writes the background into the others: the same outputs, bit for bit.  It does not apply (every tile gets its workgroup, as
 * before) in camera mode, to shares of a split (block_stride != 1 or block_cols != 0), with spp > 1, under SRT_FLAG_COUNT_WORK, to the
 * frames of srt_render_device_batch, to scenes whose records take the XCD-row or packet pipelines, to a frame of more than 4096 rows, to a scene of more than 4096 objects,
 * to a scene with a non-finite, inverted or huge (beyond 2^100) root box -- and after srt_scene_pose or srt_scene_refit_device, which
 * change the boxes on the device only, until the next of the three uploads above.  Variant 64 is variant 0 with the spans off.
 * Under SRT_FLAG_FRAMES_IN_FLIGHT with 1..4 light samples the trace workgroups over the spans are single waves, half a tile each
 * (k_trace_nq_wave8_spans): the same outputs, bit for bit.  Variant 67 is variant 0 with the two-wave workgroups kept, 31 takes the
 * one-wave workgroups without the flag and at every sample count, 32 is 31 with a tile's halves next to each other in dispatch order.
 * A render CAPTURED into a hipGraph holds the table of the boxes it was captured with.  It therefore launches the whole grid, and its
 * kernels skip the tiles outside the spans only while a word of the records -- rewritten in stream order by srt_scene_update,
 * srt_scene_update_frame, srt_scene_pose and srt_scene_refit_device -- still holds the number the table was made at: a replay after any
 * of those calls renders the new scene, without culling, until the render is captured again.  And once one of those four calls has
 * ITSELF been captured into a graph -- its replays change the boxes with no host code running, so the host's copy of them can be stale
 * at any time -- the scene's records (every handle that shares them) get no tile spans any more. */
/* CAPTURED LAUNCHES AND MATERIALS.  Every shading kernel has two builds: a general one, and one for scenes in which every object's
 * shininess is an integer in [1, 64], whose per-sample pow is a short square-and-multiply.  The host chooses at each call from the
 * materials last handed in (srt_scene_create, srt_scene_update, srt_scene_update_frame, srt_scene_pose), so an eager render, shaded
 * query or path call right after a material change shades the new materials whatever they are.  A render, srt_shade_rays*,
 * srt_shade_paths* or srt_render_paths* call CAPTURED into a hipGraph keeps the build it was captured with.  A graph captured while some
 * shininess was outside the integers 1..64 holds the general builds: its replays follow every later material change.  A graph captured
 * while every shininess was such an integer holds the specialised builds: its replays follow a change of colours, ka, ks and of
 * shininess WITHIN the integers 1..64, but after a change that leaves them (7.5, 65, 0) they would raise to the shininess truncated to an
 * integer, and nothing reports it -- capture the calls again after such a change.  (The specialised builds do not test the exponent per
 * sample: the test and the out-of-line general pow cost k_shade_tile_spans<1> 16 bytes of scratch and five path kernels an occupancy
 * class) */

typedef struct srt_stats {
    uint64_t primary_rays;         /* width x owned rows x spp (of the last render)                 */
    uint64_t hit_rays;             /* primary rays that hit                                         */
    uint64_t shadow_rays;          /* hit_rays x n_lights (algorithmic count)         */
    /* work of the kernels' own traversal; SRT_FLAG_COUNT_WORK only, else 0 */
    uint64_t node_tests_primary;   /* slab tests in the closest-hit kernel                          */
    uint64_t tri_tests_primary;    /* Moller-Trumbore tests in the closest-hit kernel               */
    uint64_t node_tests_shadow;    /* slab tests in the shadow/shade kernel                         */
    uint64_t tri_tests_shadow;     /* Moller-Trumbore tests in the shadow/shade kernel              */
    /* HIP-event times on the launch stream, AVERAGED over the `launches` renders since the previous
     * srt_sync (at most 64 are kept; older ones are dropped from the average) */
    float    ms_primary;           /* closest-hit kernel                                            */
    float    ms_shadow;            /* shadow-ray kernel                                             */
    float    ms_shade;             /* shading kernel                                                */
    float    ms_total;             /* first launch -> last kernel done                              */
    uint32_t launches;
    uint32_t rows;                 /* rows written by the last render                               */
} srt_stats;

typedef struct srt_scene srt_scene;     /* opaque: device-resident flat scene + workspace           */

/* Fill p with the reference's literals for a WxH frame and one light at (lx,ly,lz) rendered
 * whole on one device.  light_pos is left NULL: point it at a table (srt_light_staircase). */
void srt_params_default(srt_params* p, uint32_t width, uint32_t height);

/* The soft-shadow light table of softShadow (simple_raytracer.cpp:363-383): sample 0 = base, then
 * x, y, z, x, ... += 3.0f accumulated in f32 exactly as the reference does.  out = n x 3. */
void srt_light_staircase(const float base[3], uint32_t n, float* out);

/* Number of rows a call with these params writes (<= height) and the width of those rows (width unless block_cols > 0). */
uint32_t srt_rows_owned(const srt_params* p);
uint32_t srt_cols_owned(const srt_params* p);

/* Validate + upload a flat scene to HIP device `device`.  The descriptor's arrays are only read
 * during the call. */
int srt_scene_create(int device, const srt_scene_desc* desc, srt_scene** out);
int srt_scene_destroy(srt_scene* s);

/* Another handle on the SAME device records (no copy of the geometry; they are freed with the last handle): its own workspace,
 * counters, statistics and stream, so that several frames of one static scene -- other lights, another camera (ray_matrix),
 * another share of the frame -- can be in flight at once (streams, srt_render_device_batch) while the records stay hot in L2 /
 * Infinity Cache once.  srt_scene_update through any of the handles rewrites the records all of them read; it is ordered on THAT
 * call's stream only, so the other handles must not have renders in flight and must not render before it has completed (e.g. a
 * render enqueued behind it on the same stream has been waited for). */
int srt_scene_share(srt_scene* src, srt_scene** out);

/* The next frame's geometry into the SAME device allocations (the reference re-transforms and rebuilds everything per frame,
 * simple_raytracer.cpp:534-618): `desc` must have the counts of the scene's current contents (n_objects, n_nodes, n_tris,
 * n_textures, the same triangles textured / with normals) and the texture table of the uploaded scene (tex_off, tex_w, tex_h), else
 * SRT_ERR_LAYOUT -- create a new scene then.  Texture images are uploaded again only when their bytes differ from what the device
 * holds (a 64-bit content hash is compared; they rarely change between frames); tri_tex / tri_texcoord always are.  Asynchronous on `stream`: the copies are
 * ordered behind the renders already enqueued there (NULL = the scene's own stream, the one srt_render / srt_render_async use);
 * the descriptor's arrays are only read during the call. */
int srt_scene_update(srt_scene* s, const srt_scene_desc* desc, void* stream);

/* ---- f1, the device half of the per-frame rebuild (Object.cpp:183-190 transform, :205-221 boxes, :225-284 build) ----
 * The reference re-transforms every triangle and rebuilds every hierarchy per frame.  What the HOST must keep doing for an exact
 * result is the build's std::sort (its order of equal keys is libstdc++'s; tests/test_host_mirror.py) and, on the way, the node boxes
 * that choose each split axis.  Everything else of a frame's scene is derived ON THE DEVICE from what that build leaves behind:
 *   the transformed points in SOURCE order (as the host holds them: object by object, inside an object in load order),
 *   the permutation the build leaves (visit order -> source index inside the object), and the node boxes in DFS pre-order.
 * The device gathers the triangles into visit order, derives the ray-independent triangle records (P1 = p1 / w, e1, e2, the face
 * normal, tvec and qvec of rays from the origin -- the same IEEE operations srt_scene_create runs on the host, bit for bit), permutes
 * the per-triangle attributes, and writes the boxes into the node records.  Per frame the host sends 52 bytes a triangle and 24 a node
 * instead of flattening, deriving and copying ~130 bytes a triangle.
 * Contract: the scene was created (srt_scene_create) from hierarchies of the same SHAPE -- same objects in the same order, same
 * triangle count per object (the reference's builder halves while a node holds more than 8 triangles, so the shape depends on the
 * count alone) -- and only positions, order and boxes change.  Counts are checked (SRT_ERR_LAYOUT), the shape cannot be.          */
typedef struct srt_frame_geometry {
    uint32_t n_objects;
    const uint32_t*        obj_n_tris;     /* n_objects: triangles per object (checked against the scene)                      */
    const uint32_t*        obj_n_nodes;    /* n_objects: nodes per object (checked against the scene)                          */
    const float* const*    obj_points;     /* per object: n_tris x 3 x 4 transformed points (Triangle::pointOne/Two/Three), SOURCE order */
    const uint32_t* const* obj_order;      /* per object: n_tris; visit-order triangle i of the object is its source triangle obj_order[k][i] */
    const float* const*    obj_node_min;   /* per object: n_nodes x 3, the object's nodes in DFS pre-order (root first, left subtree, right subtree) */
    const float* const*    obj_node_max;
    const float*           obj_color;      /* n_objects x 3 or NULL (unchanged)                                                */
    const float*           obj_material;   /* n_objects x 3 or NULL (unchanged)                                                */
} srt_frame_geometry;

/* Per-triangle attributes in SOURCE order (objects concatenated in the scene's order), set once: srt_scene_update_frame permutes
 * them into each frame's visit order.  tri_texcoord: n_tris x 6 (needed if the scene has textured triangles), tri_normals: n_tris x 9
 * or NULL (needed if the scene was created with normals), tri_tex: n_tris texture ids or NULL (= none textured).  A later
 * srt_scene_update (a whole new flat scene) discards them: set them again before the next srt_scene_update_frame.                 */
int srt_scene_set_source(srt_scene* s, const float* tri_texcoord, const float* tri_normals, const int32_t* tri_tex);

/* The next frame's geometry, derived on the device (see above).  Asynchronous on `stream` (NULL = the scene's own stream), ordered
 * behind the renders already enqueued there; the arrays are only read during the call. */
int srt_scene_update_frame(srt_scene* s, const srt_frame_geometry* g, void* stream);

/* ---- POSE, an opt-in EXTENSION (like camera mode and spp): move objects by matrix, the hierarchy REFITTED on the device -------------
 * What a frame costs the host on the exact path above is the reference's rebuild (sort, boxes) plus 52 bytes a triangle over PCIe.  When
 * the objects only MOVE -- rigidly or by any 4x4 matrix -- the tree can keep its shape and the triangles their order: the points are
 * transformed, the triangle records derived and every node box recomputed on the device, from one matrix per object (64 bytes an object
 * per frame, no host work proportional to triangles or nodes).  Unlike camera mode it moves objects against each other and against the
 * light, stays in the reference's frame (rays from the origin: every shipped pipeline applies), and needs no rebuild on the host.
 * PARITY: the tree is the one built at the pose the scene was created (or last updated) from, not the one the reference would build at
 * the new pose.  Triangle ids keep the numbering of that scene, and equal-t ties and grazing box culls may resolve differently from the
 * reference's frame at that pose.  What is pinned, bit for bit, is: the oracle rendering the SAME flat scene -- same order, same tree
 * shape, moved points, refitted boxes -- gives the same hit ids, t bits and colours.  The arithmetic (all without contraction):
 *   point    per component i, glm's mat4 * vec4: (m[0][i]*x + m[1][i]*y) + (m[2][i]*z + m[3][i]*w), all four components;
 *   records  as srt_scene_create derives them, from the moved points;
 *   box      per component from (+FLT_MAX, -FLT_MAX), over the node's triangles in visit order, points one, two, three, raw xyz:
 *            if (v < mn) mn = v; if (mx < v) mx = v;  (a leaf without triangles keeps the start values; a NaN never enters a box);
 *   the union of the root boxes as srt_scene_create computes it.
 * Matrices and points are not validated.  A matrix with inf or NaN entries, one that overflows the points or makes them subnormal, the
 * zero matrix, a projective last row (w' of any value, 0 included), a mirror: the moved point is what IEEE arithmetic gives (inf - inf
 * and 0 * inf are NaN), and boxes and records treat it as stated under REFIT below -- a NaN coordinate enters no box, +inf only a
 * maximum and -inf only a minimum, subnormals compare as the numbers they are, of equal values (+0 and -0) the first in visit order
 * stays, the box ignores w' and the records divide by it.
 * Pipeline choice: srt_scene_overlap_estimate and the packet / node-queue decision keep the value last computed on the host (create,
 * update, update_frame); results never depend on that choice.
 *
 * srt_scene_set_pose_source: the points the poses are applied to, n_tris x 3 x 4 floats in the scene's CURRENT visit order (the layout
 * of srt_scene_desc.tri_points).  Copied to the device once (48 B a triangle); waits for the device.  They belong to the device records,
 * so every handle of srt_scene_share sees them.  A later srt_scene_update or srt_scene_update_frame changes the visit order and discards
 * them: set them again before the next srt_scene_pose.  NULL handle or points: SRT_ERR_ARG.  A tree of height above 255 (a root
 * that is a leaf has height 0): SRT_ERR_LIMIT, before anything is touched -- the scene keeps rendering, and has no pose source. */
int srt_scene_set_pose_source(srt_scene* s, const float* tri_points);

/* The next frame from one matrix per object: obj_matrix = n_objects x 16 floats, column-major like glm::mat4; every point of object k
 * becomes obj_matrix[k] * (its pose-source point) -- poses do not accumulate.  obj_color / obj_material: n_objects x 3 or NULL
 * (unchanged), as in srt_frame_geometry.  Asynchronous on `stream` (NULL = the scene's own stream), ordered behind the renders already
 * enqueued there; the arrays are only read during the call.  Through a shared handle it rewrites the records all handles read, under
 * the ordering rule of srt_scene_update (see srt_scene_share).  Errors, all before anything is touched: NULL handle or obj_matrix, or no
 * valid pose source: SRT_ERR_ARG; n_objects other than the scene's: SRT_ERR_LAYOUT. */
int srt_scene_pose(srt_scene* s, uint32_t n_objects, const float* obj_matrix,
                   const float* obj_color, const float* obj_material, void* stream);

/* ---- REFIT from device points, an opt-in EXTENSION like pose: the caller's vertex buffer in DEVICE memory, the hierarchy refitted ----
 * Pose covers rigid motion; a mesh that DEFORMS -- skinning, cloth, morph targets, a simulation step, an optimiser moving vertices --
 * lives in a device buffer of the caller's.  srt_scene_refit_device takes the points from there: the tree keeps the shape and the
 * triangles the order of the scene as created or last updated (PARITY as for pose: ids keep that scene's numbering), both triangle
 * records are derived and every node box recomputed on the device.  No arithmetic is applied to a point or a normal: they are copied,
 * then the records are derived.
 * What is pinned, bit for bit: the device records after a refit are byte for byte what srt_scene_create derives from the flat scene with
 *   points   those points, a stride of 3 meaning w = 1.0f exactly;
 *   box      pose's fold: per component from (+FLT_MAX, -FLT_MAX), over the node's triangles in visit order, points one, two, three,
 *            raw xyz: if (v < mn) mn = v; if (mx < v) mx = v;  -- the left operand is kept on ties, a NaN never enters a box, a leaf
 *            without triangles keeps the start values;
 *   the union of the root boxes as srt_scene_create computes it;
 *   normals  d_normals given: tri_normals becomes exactly those floats -- direct form row i, indexed form the three gathered rows in
 *            point order one, two, three; NULL: unchanged.  Texel coordinates and texture ids stay.
 * Every render and query afterwards equals the oracle on that same flat scene.  Point values are not validated: non-finite points are
 * memory-safe and give what the arithmetic gives.  In full:
 *   NaN        a NaN coordinate (quiet or signalling, either sign) enters no box; the other coordinates of the point still do.  A leaf
 *              or an object whose points are all NaN keeps (+FLT_MAX, -FLT_MAX), as a leaf without triangles.
 *   +-inf      +inf becomes a maximum and never a minimum (inf < FLT_MAX is false: the start value stays), -inf the reverse.
 *   +-FLT_MAX  ties with the start value; the box holds the same bits either way.
 *   zeros      of equal values the first in visit order stays, and an inner node keeps its left child's: a box holds -0 or +0
 *              according to which came first (no compare of a walk tells them apart).
 *   subnormal  coordinates compare as the numbers they are; nothing is flushed to zero, in a box or in a record.
 *   w          the box reads raw xyz and ignores w; the records divide by it: w = +-0 gives +-inf or NaN points, w = NaN NaN points, a
 *              huge or tiny w what the divide gives.  Rays meet such records as the oracle does on the same flat scene.
 * Pipeline choice: srt_scene_overlap_estimate and the packet / node-queue decision keep the host's last value, as for pose.  A pose source stays valid across refits: poses apply to their source and do not accumulate.
 *
 * srt_scene_refit_prepare, a set-up call, once per tree: derives the refit's static schedule from the tree's shape (the one pose uses)
 * and, for the indexed form, takes the index buffer: tri_vertex = n_tris x 3 entries in HOST memory, in the scene's current visit order;
 * point j of triangle i is vertex tri_vertex[3 i + j] of a buffer of n_verts vertices.  Every entry is validated: one >= n_verts is
 * SRT_ERR_LAYOUT, before anything is touched.  The indices are copied to the device once (12 B a triangle) and belong to the device
 * records, so every handle of srt_scene_share sees the preparation.  tri_vertex == NULL prepares the direct form only (and drops earlier
 * indices); n_verts is then ignored.  Waits for the device.  A later srt_scene_update or srt_scene_update_frame discards the preparation,
 * as it discards the pose source.  NULL handle: SRT_ERR_ARG.  A tree of height above 255: SRT_ERR_LIMIT, before anything is touched --
 * the scene keeps rendering, and is not prepared. */
int srt_scene_refit_prepare(srt_scene* s, uint32_t n_verts, const uint32_t* tri_vertex);

typedef struct srt_refit_desc {
    uint32_t     n_verts;    /* 0: DIRECT form, d_points = n_tris x 3 points in the scene's current visit order (the layout of
                                srt_scene_desc.tri_points); > 0: INDEXED form, d_points = n_verts points, point j of triangle i is
                                d_points[tri_vertex[3 i + j]]; must equal the prepared n_verts                                       */
    uint32_t     stride;     /* floats per point: 4 = raw homogeneous xyzw; 3 = xyz, w taken as 1.0f                                 */
    const float* d_points;   /* DEVICE                                                                                               */
    const float* d_normals;  /* DEVICE or NULL (= unchanged).  direct: n_tris x 9; indexed: n_verts x 3                              */
} srt_refit_desc;

/* The next frame from the caller's device buffers.  Asynchronous on `stream` (NULL = the scene's own stream), ordered behind the updates,
 * poses, renders and queries already enqueued there.  The call allocates nothing, copies nothing and stages nothing; it looks at no
 * triangle or node on the host and does not wait.  It is a fixed sequence of kernel launches and may be captured into a hipGraph; the
 * caller's buffers are read when the kernels run, not during the call.  Any float-aligned pointer is legal: points of stride 4 in a
 * 16-byte aligned buffer are read with 16-byte loads, everything else with 4-byte loads -- a point of stride 3 is read as exactly
 * 12 bytes, nothing past the last point of a buffer.  Through a handle of srt_scene_share it rewrites the records all handles read,
 * under the ordering rule of srt_scene_update.  Errors, all before anything is touched: NULL handle, g or d_points, a stride other
 * than 3 or 4, a scene that is not prepared, the indexed form without prepared indices, d_normals on a scene created without
 * normals: SRT_ERR_ARG; n_verts other than the prepared one: SRT_ERR_LAYOUT. */
int srt_scene_refit_device(srt_scene* s, const srt_refit_desc* g, void* stream);

/* Render into DEVICE buffers (rows = srt_rows_owned(p)); any output pointer may be NULL.
 *   d_hit_id     rows x W   int32   canonical triangle id, -1 = miss
 *   d_t          rows x W   f32     closest-hit distance (+inf on miss)
 *   d_rgb_linear rows x W x 3 f32   pre-tone-map light-sample sum (softShadow:362-383); 0 on miss
 *   d_rgb8       rows x W x 3 u8    tone-mapped, quantised (:391-398,447-449), black -> background
 *                                   (:518, drawImage:476-487)
 * Asynchronous on `stream` (a hipStream_t, NULL = default stream); stats->ms_* are valid after
 * srt_sync().  */
int srt_render_device(srt_scene* s, const srt_params* p, void* stream,
                      int32_t* d_hit_id, float* d_t, float* d_rgb_linear, uint8_t* d_rgb8);

/* The frames of a step (the reference's main() renders a 36-frame orbit, simple_raytracer.cpp:534) in ONE set of launches:
 * frame i = srt_render_device(scenes[i], &params[i], stream, d_hit_id[i], ...), with bitwise the same outputs.  The handles must
 * be n DISTINCT handles on one device (a handle's workspace serves one frame at a time; srt_scene_share gives n handles on one
 * copy of a scene); each output table may be NULL, and so may its entries.  Frames of two classes are held back and share launches,
 * which fills the chip where one frame, or the eighth of it one of eight GPUs owns, does not (a silhouette tile occupies its
 * workgroup for the better part of such a launch).  Both classes: variant 0, one common size, spp 1, no SRT_FLAG_COUNT_WORK, no camera
 * matrix, a scene without the packet preference (srt_scene_overlap_estimate <= 150).  Class one, a pair of launches: 1..7 light
 * samples, records of at most 32 MiB.  Class two, three launches: the frames whose shadow rays take the packet kernel -- 16 and more
 * samples, or 8..15 on a scene whose estimate is 14 or more.  Any other frame is launched on its own as srt_render_device would:
 * among them 8..15 samples on a scene of few nodes (estimate < 14), which take the chunked node-queue shadow launch.  srt_scene_pipeline
 * says "(batched)" for a held frame.  The frames' arguments travel
 * by value with the launches (up to 36 frames a launch, more frames = more launches): nothing is allocated or copied, and the call
 * may be captured into a hipGraph like any other (ABI version 3; earlier versions kept argument tables in device memory and could not
 * make one while capturing).  Frames of class two: the shadow-ray launch of a call remembers which 4x4-pixel
 * quadrants had long walks and the next call on the same handles deals those early -- order only, results do not depend on it
 * (SRT_HEAVY_STEPS=0 in the environment turns it off; single frames without SRT_FLAG_FRAMES_IN_FLIGHT do the same).  No per-frame times: srt_sync()'s ms_* keep the values of the last timed
 * render of each handle. */
int srt_render_device_batch(uint32_t n, srt_scene* const* scenes, const srt_params* params, void* stream,
                            int32_t* const* d_hit_id, float* const* d_t, float* const* d_rgb_linear, uint8_t* const* d_rgb8);

/* Same, into HOST buffers: allocates nothing per call beyond the scene's workspace, copies back,
 * synchronises.  stats may be NULL. */
int srt_render(srt_scene* s, const srt_params* p,
               int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8, srt_stats* stats);

/* srt_render without the wait: the kernels and the copies into the host buffers are enqueued on the scene's own stream and the
 * call returns; srt_sync() waits.  With buffers from srt_host_alloc (pinned memory) the copies are asynchronous and run at full
 * PCIe rate; with ordinary memory they still work.  srt_scene_update(scene, desc, NULL) is ordered on the same stream, so
 * "update, render_async, (build the next frame on the CPU), sync" keeps the GPU work off the host's critical path. */
int srt_render_async(srt_scene* s, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8);
void* srt_host_alloc(size_t bytes);        /* pinned host memory, NULL on failure */
void  srt_host_free(void* p);

/* Wait for the last srt_render_device / srt_render_async on this scene and collect its stats. */
int srt_sync(srt_scene* s, srt_stats* stats);

/* ---- RAY QUERIES, an opt-in EXTENSION (the reference traces only the pixels of its own camera) -------------------------------------
 * What does THIS ray hit, and is the way from here towards there blocked -- for rays the caller supplies (picking, placing an object on
 * the ground, a probe or range sensor, visibility between arbitrary points), against the records a scene keeps on the device.
 * rays = n x 6 floats: origin xyz, direction xyz, in the space of the scene's records.
 * Directions are NOT normalised; t is in units of the direction, as everywhere in the reference.
 * PARITY: the reference cannot take a ray from a caller, so what is pinned, bit for bit, is the oracle on the same flat scene.  A ray
 * (o, d) is the one pixel of a 1 x 1 camera-mode frame with focal 1 and ray_matrix columns (0, 0, d, o); a W x H camera-mode frame is
 * W * H rays with directions (M[0] * dx + M[1] * dy) + M[2] * dz.  The query's hit id and t bits are those frames' -- the literal slab
 * test with the ray's origin, the general Moller-Trumbore test on the triangle's points, no t pruning, strict '<' (lowest id among equal
 * t) -- and the occlusion bit is shadowIntersection:321-342 on that scene.  Results never depend on the order of the rays in a call.
 * Non-finite rays are memory-safe and give whatever the walk gives.  n == 0: SRT_OK, nothing happens.
 * Errors, all before anything is touched: NULL handle, NULL rays with n > 0, flags other than 0 or SRT_FLAG_COUNT_WORK: SRT_ERR_ARG.
 *
 * Closest hit.  Any output pointer may be NULL.
 *   hit_id  n       int32  canonical triangle id, -1 = miss
 *   t       n       f32    distance in units of the direction, +inf on a miss
 *   bary    n x 3   f32    calculateBarycentricCoords (:79-117) (u, v, w) at origin + direction * t, the operations the textured shading
 *                          path runs; (0, 0, 0) on a miss
 * Occlusion.  occluded[i] = 1 if any object's tree but skip_obj[i]'s yields a candidate triangle whose Moller-Trumbore result is not
 * -inf (NaN included, as the reference), else 0; t is unbounded, as in the reference (srt_occluded_range bounds it).  skip_obj: the object whose own tree is left out
 * (the hit object's, for a shadow ray), n entries or NULL; an entry of -1 -- or any entry outside [0, n_objects), which is not
 * validated on the host -- leaves nothing out.
 * A NULL occluded / d_occluded leaves the call nothing to report: it returns SRT_OK and launches nothing.
 *
 * The _device entry points take device pointers (rays that are 8-byte aligned are read with wide loads), are asynchronous on `stream`
 * (NULL = the scene's own stream), ordered behind the updates, poses and renders already enqueued there, allocate nothing and copy
 * nothing; without SRT_FLAG_COUNT_WORK they may be captured into a hipGraph.  They leave alone what srt_sync and srt_scene_pipeline
 * report and the alternating counter sets of the renders; through a handle of srt_scene_share they read the one copy of the records.
 * The host entry points take host pointers, stage through the handle's pinned staging block, wait, and fill *stats (may be NULL):
 * primary_rays = n, hit_rays, and under SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary, from a counter set private to
 * queries; every other field is 0.  That set belongs to the handle, and only the host entry points report it (they zero it, count
 * into it and read it back within the call).  A _device call with SRT_FLAG_COUNT_WORK runs the counting build and zeroes and fills
 * the same set, which no call hands to a device caller: it is there to measure the counting build, and it must not be in flight
 * while another query runs on the same handle.  Queries on several streams at once: without the flag, or one handle of
 * srt_scene_share each. */
int srt_trace_rays_device(srt_scene* s, uint32_t n, const float* d_rays, uint32_t flags, void* stream,
                          int32_t* d_hit_id, float* d_t, float* d_bary /* n x 3 (u,v,w) or NULL */);
int srt_trace_rays(srt_scene* s, uint32_t n, const float* rays, uint32_t flags,
                   int32_t* hit_id, float* t, float* bary, srt_stats* stats);
int srt_occluded_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_skip_obj /* n or NULL */,
                        void* stream, uint8_t* d_occluded);
int srt_occluded(srt_scene* s, uint32_t n, const float* rays, const int32_t* skip_obj, uint8_t* occluded);

/* A t interval per ray.  The _range forms take t_range = n x 2 floats, (t_min, t_max) per ray, and answer for the part of each ray inside
 * its interval: visibility between two points as a segment (d = B - A, range (0, 1)), a sensor with a reach, a ray that starts ON a
 * surface (t_min a little above 0, the origin not moved), the second hit along a ray (t_min = the next float after the first hit's t;
 * srt_trace_rays_multi below gives the K nearest hits in one walk, ties included).
 * Unless said here everything is as for the forms above: the layout of rays and of every output, the flags, the ordering on `stream`,
 * what the host forms stage (t_range travels through the same pinned block as the rays), wait for and report in *stats, the private
 * counter set, hipGraph capture of the _device forms without SRT_FLAG_COUNT_WORK, the rules of srt_scene_share, the errors, n == 0, a NULL
 * occluded.  t_range is read like rays: host memory in the host forms; in the _device forms a device pointer, one 8-byte load per ray where
 * it is 8-byte aligned and two 4-byte loads where it is only float-aligned.
 * DEFINITION.  The candidate set of a ray is unchanged -- the reference's: every leaf whose ancestors all pass the literal slab test, no
 * pruning by t -- and a candidate's t is the same Moller-Trumbore result on the same operands.  A candidate is IN RANGE iff
 * !(t < t_min) && !(t > t_max): the interval is closed, a NaN bound bounds nothing, a NaN t is in range.
 *   Closest hit: among the candidates with t != -inf && t < +inf that are in range, the minimum t; equal t goes to the lowest id, and +0
 *                and -0 tie as they do without an interval.  The reported t is the winner's own bits, bary is taken at
 *                origin + direction * t.  No such candidate: -1, +inf, (0, 0, 0).
 *   Occlusion:   1 iff a candidate outside skip_obj[i]'s tree has t != -inf (NaN included) and is in range.
 *   Identities:  a NULL t_range, or a ray whose interval is (0, +inf), (-inf, +inf) or (NaN, NaN), gives bit for bit what the unbounded
 *                call gives for that ray, NaN candidates included.  t_min > t_max: a miss / not occluded.
 * Boxes are NOT rejected by t_max: the walk visits exactly the nodes the unbounded call visits, so under SRT_FLAG_COUNT_WORK the
 * closest-hit form reports the node_tests_primary and tri_tests_primary of the unbounded call on the same rays; the interval costs
 * 8 bytes per ray and two comparisons per tested triangle, and saves no work.
 * The shaded query takes an interval too: srt_shade_rays_range, declared after srt_shade_rays below. */
int srt_trace_rays_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2: t_min, t_max; or NULL */,
                                uint32_t flags, void* stream, int32_t* d_hit_id, float* d_t, float* d_bary);
int srt_trace_rays_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags,
                         int32_t* hit_id, float* t, float* bary, srt_stats* stats);
int srt_occluded_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range,
                              const int32_t* d_skip_obj, void* stream, uint8_t* d_occluded);
int srt_occluded_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const int32_t* skip_obj, uint8_t* occluded);

/* The K nearest hits of a ray in one walk: what lies BEHIND the first hit -- the exit point of a solid, the thickness a ray passes
 * through, how many surfaces it crosses, the first hit a later filter accepts.  (The chain of srt_trace_rays_range calls with t_min = the
 * next float after the last t steps over every other candidate with the same t -- coplanar duplicates, the +0 / -0 pair -- and costs one
 * full walk and one round trip per hit.)  k = the hits wanted per ray, 1 .. SRT_MULTI_HIT_MAX.
 * Unless said here everything is as for srt_trace_rays_range: the layout of rays and t_range with wide loads where they are 8-byte
 * aligned, a NULL t_range, the flags, the ordering on `stream`, the private counter set, the rules of srt_scene_share, n == 0, the errors.
 * DEFINITION.  The candidate set of a ray and each candidate's t are exactly those of srt_trace_rays_range: every leaf whose ancestors all
 * pass the literal slab test, no pruning by t -- not by the interval, and not by the k-th hit found so far.  The QUALIFYING set Q of a ray
 * holds its candidates with t != -inf && t < +inf that are in range, !(t < t_min) && !(t > t_max); a NULL t_range bounds nothing.
 *   n_hits  n           u32    |Q|, the full count: it may exceed k.  Each triangle id counts once (a leaf the walk takes in slices adds
 *                              nothing twice).
 *   hit_id  n x k       int32  row i: the min(|Q|, k) first elements of Q in ascending order of (t with -0 keyed as +0, id) -- equal t
 *   t       n x k       f32    goes to the lowest id first, the two zeros tie -- each t with that candidate's own bits, the sign of a zero
 *   bary    n x k x 3   f32    included, each bary calculateBarycentricCoords at origin + direction * t of THAT hit.  The remaining slots
 *                              of a row are -1, +inf, (0, 0, 0).
 * Any output pointer may be NULL; the _device form with all four NULL returns SRT_OK and launches nothing.
 *   Identities:  column 0 of every row is bit for bit what srt_trace_rays_range gives for that ray, for any k and any interval (the four
 *                identity intervals included); n_hits[i] > 0 iff that call hits; results never depend on the order of the rays; the row
 *                of a ray at a smaller k is a prefix of its row at a larger k.
 * The _device form allocates and copies nothing; without SRT_FLAG_COUNT_WORK it is one launch and may be captured into a hipGraph.  The
 * host form stages through the handle's pinned block, waits, and fills *stats: primary_rays = n, hit_rays = the rays with n_hits > 0, and
 * under SRT_FLAG_COUNT_WORK the node_tests_primary / tri_tests_primary of the unbounded srt_trace_rays on the same rays -- the walk visits
 * the same nodes and tests the same triangles.
 * Errors beyond those of srt_trace_rays_range, before anything is touched: k == 0: SRT_ERR_ARG; k > SRT_MULTI_HIT_MAX: SRT_ERR_LIMIT. */
#define SRT_MULTI_HIT_MAX 16
int srt_trace_rays_multi_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                uint32_t k, uint32_t flags, void* stream,
                                uint32_t* d_n_hits /* n */, int32_t* d_hit_id /* n x k */, float* d_t /* n x k */,
                                float* d_bary /* n x k x 3 */);
int srt_trace_rays_multi(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t k, uint32_t flags,
                         uint32_t* n_hits, int32_t* hit_id, float* t, float* bary, srt_stats* stats);

/* Shaded colour: what comes back along each ray -- everything the library does after the closest hit for the pixels of its own camera
 * (texture lookup, the soft-shadow light samples, Phong, smooth normals, tone map, quantiser, background rule), for rays the caller
 * supplies: a mirror, a second view, a probe that sees light, a picking preview.  rays as above.  srt_params is reused, so that
 * srt_params_default still supplies the reference's literals.  Fields READ: n_lights and light_pos (host pointer, n_lights x 3),
 * shadow_div, reinhard, gamma, background, flags.  Fields IGNORED: width, height, block_rows, block_first, block_stride, block_cols,
 * focal, ray_matrix, spp.
 * PARITY: per ray the one pixel of the oracle's 1 x 1 camera-mode frame for that ray (see above) with those lights, literals and flags:
 *   hit_id      n       int32  exactly what srt_trace_rays gives; -1 on a miss
 *   t           n       f32    exactly what srt_trace_rays gives; +inf on a miss
 *   rgb_linear  n x 3   f32    the pre-tone-map sum over the light samples (softShadow:362-383), in light order l = 0 .. n_lights - 1, one
 *                              f32 add per sample; a sample whose shadow ray (shadowIntersection:321-342 from so = o + d * t towards
 *                              sd = L - so, the hit object's tree left out, t unbounded, NaN counts) is blocked is divided by shadow_div
 *                              per component.  Colour = the object's, or the texel found through calculateBarycentricCoords at o + d * t
 *                              (index clamped into the image, as in a render); normal = the record's face normal, or
 *                              interpolateNormal under SRT_FLAG_SMOOTH_NORMALS; Phong with the ray's own origin and direction.
 *                              (0, 0, 0) on a miss
 *   rgb8        n x 3   u8     tone-mapped, quantised (:391-398,447-449); all-black -- a miss, or a hit that sums to black -- becomes
 *                              `background` (:518, drawImage:476-487)
 * n_lights == 0 is allowed: a hit then has rgb_linear 0 and rgb8 = background.  Any output pointer may be NULL, and so may all of them.
 * Flags: 0, SRT_FLAG_COUNT_WORK, SRT_FLAG_SMOOTH_NORMALS or both; SRT_FLAG_SMOOTH_NORMALS on a scene without normals fails as
 * srt_render_device does (SRT_ERR_ARG); any other bit, the variant bits 8..15 included: SRT_ERR_ARG.
 * Errors, all before anything is touched: NULL handle, NULL p, NULL rays with n > 0, n_lights > 0 with NULL light_pos: SRT_ERR_ARG;
 * n * max(n_lights, 1) >= 2^32: SRT_ERR_LIMIT.  n == 0 (with valid arguments): SRT_OK, nothing happens.
 * The _device form: device pointers, one launch, asynchronous on `stream` (NULL = the scene's own stream), ordered behind the updates,
 * poses and renders already enqueued there; it allocates nothing proportional to n and leaves alone what srt_sync and srt_scene_pipeline
 * report and the renders' alternating counter sets.  The light table goes to the device as a render's does -- through a pinned copy, and
 * again only when its bytes differ from the last query's -- into a buffer PRIVATE TO QUERIES (a render's table may be in use on another
 * stream).  Like the query counter set it belongs to the handle: ONE light table per handle at a time -- a call with another table must
 * not be enqueued while a query with the previous one is in flight on a different stream; for concurrent calls with different tables take
 * one handle of srt_scene_share each.  Without SRT_FLAG_COUNT_WORK, and with the table already on the device -- an earlier call
 * with the same table on the same stream, or on any stream once its upload has completed (a wait on that stream, or any host-form call) --
 * the call is a single kernel launch and may be captured into a hipGraph; while an upload made on ANOTHER stream is still pending, the
 * call first makes its stream wait for it.  SRT_FLAG_COUNT_WORK: as for srt_trace_rays_device.
 * The host form stages the rays through the handle's pinned block, waits, copies out and fills *stats (may be NULL): primary_rays = n,
 * hit_rays, shadow_rays = hit_rays x n_lights, and under SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary / node_tests_shadow /
 * tri_tests_shadow -- the oracle's algorithmic counts: every shadow ray walked on its own, objects in order, the hit object's tree left
 * out, left at the first hit; every other field is 0. */
int srt_shade_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const srt_params* p, void* stream,
                          int32_t* d_hit_id, float* d_t, float* d_rgb_linear /* n x 3 */, uint8_t* d_rgb8 /* n x 3 */);
int srt_shade_rays(srt_scene* s, uint32_t n, const float* rays, const srt_params* p,
                   int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8, srt_stats* stats);

/* Shaded colour inside a t interval per ray: the colour of the closest hit IN RANGE -- a reflected ray that starts ON a surface (t_min a
 * little above 0, the origin not moved, so that the shadow origin and Phong's view vector keep their bits), the colour seen through a first
 * surface, the colour at the exit point of a solid.
 * Unless said here everything is as for srt_shade_rays: the params fields read and ignored, the flags, the errors (checked before anything
 * is touched), n == 0, NULL outputs, the one-light-table-per-handle rule, hipGraph capture of the _device form, srt_scene_share.  t_range is
 * read exactly as srt_trace_rays_range reads it: n x 2 floats (t_min, t_max), one 8-byte load per ray where the pointer is 8-byte aligned,
 * two 4-byte loads where it is only float-aligned; the host form stages it through the same pinned block as the rays.
 * DEFINITION.
 *   hit_id, t         bit for bit what srt_trace_rays_range gives for that ray and interval: the candidate set is unchanged, a candidate is
 *                     in range iff !(t < t_min) && !(t > t_max), equal t goes to the lowest id, +0 ties with -0, and the reported t has the
 *                     winner's own bits.
 *   rgb_linear, rgb8  everything srt_shade_rays computes after the closest hit, applied to THAT hit: the surface lookup at o + d * t, the
 *                     shadow rays from so = o + d * t towards L - so, Phong with the ray's own o and d, the sum in light order, the tone
 *                     map, the quantiser and the background rule.  The origin is never moved.  The shadow rays stay unbounded, with the hit
 *                     object's tree left out, as in the reference: the interval bounds the primary ray only.
 *   No in-range candidate: -1, +inf, (0, 0, 0) and the background.
 *   Identities:  a NULL t_range gives srt_shade_rays' bits in every output for every ray (and launches its kernels); so does a ray whose
 *                interval is (0, +inf), (-inf, +inf) or (NaN, NaN).  t_min > t_max: a miss.
 * *stats: primary_rays = n, hit_rays = the rays with an in-range hit, shadow_rays = hit_rays x n_lights.  Under SRT_FLAG_COUNT_WORK
 * node_tests_primary and tri_tests_primary are those of the unbounded srt_trace_rays on the same rays (the walk is the same: boxes are not
 * rejected by t_max), node_tests_shadow and tri_tests_shadow the oracle's algorithmic counts for the shadow rays of the hits reported. */
int srt_shade_rays_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                const srt_params* p, void* stream,
                                int32_t* d_hit_id, float* d_t, float* d_rgb_linear, uint8_t* d_rgb8);
int srt_shade_rays_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                         int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8, srt_stats* stats);

/* The surface at a hit, and the reflected ray: WHAT is there -- the normal, the owning object, the colour and the material shading would
 * use -- and the mirrored ray, ready to go back into any _range query: a multi-bounce mirror, a deferred shader, a normal or albedo probe
 * on device arrays, with no copy of the geometry on the caller's side.  srt_surface_rays finds the hit itself; srt_surface_hits takes hits
 * the caller already holds (a render's hit_id / t with the frame's rays, any column of srt_trace_rays_multi) and walks nothing.
 * Unless said here everything is as for srt_trace_rays_range: the layout of rays and t_range with wide loads where they are 8-byte aligned,
 * a NULL t_range, the ordering on `stream`, the rules of srt_scene_share, n == 0, the private counter set, what the host form stages (through
 * the handle's pinned block), waits for and reports in *stats -- primary_rays = n, hit_rays, and under SRT_FLAG_COUNT_WORK the
 * node_tests_primary / tri_tests_primary of the unbounded srt_trace_rays on the same rays --, hipGraph capture of the _device form without
 * SRT_FLAG_COUNT_WORK, as one launch.
 * DEFINITION (srt_surface_rays).
 *   hit_id, t   bit for bit what srt_trace_rays_range gives for that ray and interval (the candidate set, the range rule, the ties, the
 *               winner's own t bits, the four identity intervals); a NULL t_range gives srt_trace_rays' bits.
 *   the fields of srt_surface_out, any of which may be NULL: exactly what srt_shade_rays(_range) shades that hit with.  Neither the origin nor
 *               the normal is moved or flipped.
 *   bounce      origin = point; direction r, in f32 without contraction, with N the `normal` output:
 *                   k = (d.x * N.x + d.y * N.y) + d.z * N.z        r_i = d_i - (N_i * k) * 2
 *               glm::reflect's association; the same under N -> -N, so it needs no orientation.  d is not normalised, and neither is r.
 *   A miss:     hit_id -1, t +inf, obj -1, every float output 0, the six of bounce included.  When feeding bounce back into a _range query
 *               give such rays the interval (1, 0): t_min > t_max is a miss by definition.  For the hits, t_min a little above 0 keeps the
 *               ray off the surface it starts on; the origin is not moved.
 *   Degenerate triangles and non-finite rays give whatever the stated arithmetic gives; the call stays memory-safe.
 * out == NULL, or every field of it NULL: the call IS srt_trace_rays_range without bary, and launches that kernel.
 * Flags: 0, SRT_FLAG_COUNT_WORK, SRT_FLAG_SMOOTH_NORMALS or both; SRT_FLAG_SMOOTH_NORMALS on a scene without normals fails as
 * srt_shade_rays does (SRT_ERR_ARG); any other bit: SRT_ERR_ARG.  Errors are checked before anything is touched.
 * DEFINITION (srt_surface_hits).  Row i is a miss row (as above) if hit_id[i] is outside [0, n_tris); otherwise it is the surface of triangle
 * hit_id[i] where the ray o_i + d_i * t[i] meets it, and the fields above.  t is taken as given and not validated (the texel index is
 * clamped into the image, so any t is memory-safe); no node record is read.  Identity: fed the hit_id / t that srt_surface_rays returned for
 * the same rays and flags, every field equals that call's bit for bit.  Flags: 0 or SRT_FLAG_SMOOTH_NORMALS; there is no stats and no
 * counter set.  rays, hit_id or t NULL with n > 0: SRT_ERR_ARG.  One launch; it may be captured into a hipGraph.  With out NULL, or every
 * field of it NULL, the call checks its arguments and launches nothing. */
typedef struct srt_surface_out {   /* device pointers in the _device forms, host pointers in the host forms; any may be NULL */
    int32_t* obj;        /* n      owning object (tri_obj of the hit); -1 on a miss                                    */
    float*   point;      /* n x 3  o + d * t, per component one multiply and one add, no contraction                   */
    float*   normal;     /* n x 3  the normal Phong is given for this hit: the record's face normal                    */
                         /*        (calculateTriangleNormal:32-37), or interpolateNormal's under SRT_FLAG_SMOOTH_NORMALS */
    float*   color;      /* n x 3  the colour shading uses: the object's, or the texel (softShadow:350-361, clamped)   */
    float*   material;   /* n x 3  ambient, specularStrength, shininess of the object                                  */
    float*   bounce;     /* n x 6  the mirrored ray: origin = point, direction = r (above)                             */
} srt_surface_out;
int srt_surface_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                            uint32_t flags, void* stream, int32_t* d_hit_id, float* d_t, const srt_surface_out* out);
int srt_surface_rays(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags,
                     int32_t* hit_id, float* t, const srt_surface_out* out, srt_stats* stats);
int srt_surface_hits_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_hit_id, const float* d_t,
                            uint32_t flags, void* stream, const srt_surface_out* out);
int srt_surface_hits(srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t,
                     uint32_t flags, const srt_surface_out* out);

/* Mirror paths: a ray followed through up to `depth` mirror bounces, every hit shaded, the bounces mixed by a per-object reflectance and the
 * finished pixel written, in ONE launch -- the chain srt_shade_rays_range -> srt_surface_rays (bounce) -> srt_shade_rays_range -> ... with
 * each mirrored ray walked once and nothing of a bounce written for a next launch to read back.
 * Unless said here everything is as for srt_shade_rays_range: the layout of rays and t_range with wide loads where they are 8-byte aligned,
 * a NULL t_range, the params fields read and ignored, the flags, the errors (checked before anything is touched), n == 0, NULL outputs,
 * the one-light-table-per-handle rule, the ordering on `stream`, srt_scene_share, what the host form stages, waits for and copies out.
 * DEFINITION.  A path is a row of SEGMENTS b = 0 .. depth - 1, each a ray with a t interval:
 *   segment 0       the caller's ray and interval.  hit_id, t and rgb_linear are bit for bit what srt_shade_rays_range gives for them, obj
 *                   what srt_surface_rays gives.
 *   segment b + 1   of a ray whose segment b HIT: the ray is the `bounce` row srt_surface_rays defines for segment b's hit under the call's
 *                   flags -- origin o + d * t, not moved; direction r_i = d_i - (N_i * k) * 2 with N the normal shading uses (the smooth one
 *                   under SRT_FLAG_SMOOTH_NORMALS) -- and the interval is (bounce_t_min, +inf); a NaN bounce_t_min bounds nothing.  Its
 *                   outputs are what the same two calls give for that ray and interval.
 *                   of a ray whose segment b MISSED: not walked.  Its rows, and those of every later segment, are miss rows: hit_id -1,
 *                   t +inf, obj -1, rgb_linear (0, 0, 0), a zero ray.
 *   Shadow rays are as in srt_shade_rays: from the segment's hit point, unbounded, with the hit object's tree left out.
 *   The walks are purely geometric: reflectance never ends a path, and no value of it changes which segments are walked.
 *   The mix, in f32 without contraction, from the near end (lin_b = segment b's rgb_linear, obj_b its object):
 *       acc = (0, 0, 0); W = 1
 *       for b = 0 .. depth - 1, while segment b hits:
 *           k = (b + 1 < depth && segment b + 1 hits) ? reflectance[obj_b] : 0          (a NULL table: 0)
 *           a = W * (1 - k);   acc_i = acc_i + a * lin_b_i   (one multiply, then one add);   W = W * k
 *   rgb_linear = acc; rgb8 = the tone map, the quantiser and the background rule on acc: a ray whose segment 0 misses, or a sum that is all
 *   black, gets `background`.  Reflectance values are not validated: NaN, negative values and values above 1 give what the arithmetic gives.
 *   Identities:  depth 1: rgb_linear, rgb8 and row 0 of seg are srt_shade_rays_range's bits for every ray.  A NULL or all-zero table: the
 *                mixed output is segment 0's.  The per-segment rows at depth D are the first D rows of the same call at any larger depth.
 *                Results never depend on the order of the rays.
 * seg (may be NULL, as may any field): per SEGMENT outputs, segment-major -- row b of a field is an n-array laid out like the matching
 * output of srt_shade_rays_range / srt_surface_rays, at element offset b * n (x 3, x 6).
 * Errors beyond those of srt_shade_rays_range, before anything is touched: NULL path, depth == 0: SRT_ERR_ARG; depth > SRT_PATH_DEPTH_MAX:
 * SRT_ERR_LIMIT.  A call with every output NULL returns SRT_OK and launches nothing.
 * The _device form is one kernel launch; it allocates and copies nothing proportional to n; path->reflectance is read from the caller's
 * DEVICE memory (n_objects floats) when the kernel runs.  Without SRT_FLAG_COUNT_WORK, and with the light table already on the device, it may
 * be captured into a hipGraph.
 * The host form stages rays, intervals, the reflectance table and every wanted output through the handle's pinned block and buffers, waits,
 * and fills *stats (may be NULL): primary_rays = n, hit_rays = the hits of all segments together, shadow_rays = hit_rays x n_lights; under
 * SRT_FLAG_COUNT_WORK the four test counters are the sums, over the segments actually walked, of what srt_shade_rays_range reports for that
 * segment's ray and interval. */
#define SRT_PATH_DEPTH_MAX 8
typedef struct srt_path_desc {
    uint32_t     depth;          /* segments per ray, 1 .. SRT_PATH_DEPTH_MAX                                   */
    float        bounce_t_min;   /* a mirrored ray's interval is (bounce_t_min, +inf); NaN bounds nothing        */
    const float* reflectance;    /* n_objects floats or NULL (= all 0); device pointer in the _device form       */
} srt_path_desc;
typedef struct srt_path_out {    /* per SEGMENT, segment-major: row b is an n-array laid out like the matching  */
    int32_t* hit_id;             /* depth x n          output of srt_shade_rays_range / srt_surface_rays;       */
    float*   t;                  /* depth x n          any pointer may be NULL, and so may the struct           */
    int32_t* obj;                /* depth x n                                                                    */
    float*   rgb_linear;         /* depth x n x 3      the segment's own pre-tone-map sum                       */
    float*   rays;               /* depth x n x 6      the ray the segment walked (row 0 = the caller's ray)    */
} srt_path_out;
int srt_shade_paths_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                           const srt_params* p, const srt_path_desc* path, void* stream,
                           float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_shade_paths(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                    const srt_path_desc* path, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);

/* Mirror paths in a frame: srt_shade_paths for the rays of a frame's own pixels, in ONE launch and with no ray array -- a pixel's ray is made
 * on the device, as srt_render_device makes it.  Unless said here everything is as for srt_shade_paths: the definition of a path, the mix,
 * seg, the one-light-table-per-handle rule, the ordering on `stream`, srt_scene_share.
 * PIXELS.  n = srt_rows_owned(p) x srt_cols_owned(p) local pixels, row-major; local pixel <-> image pixel by srt_params' block_rows /
 * block_first / block_stride / block_cols.  rgb_linear (n x 3) and rgb8 (n x 3) are laid out exactly as srt_render_device lays them out;
 * every field of seg is depth x n, segment-major: row b starts at element offset b * n (x 3 for rgb_linear, x 6 for rays).  Padding pixels of
 * a tile deal (image column >= width) are not written in any output.
 * THE RAY of a pixel is the frame's own: direction (i, j, focal) with i = x + (int)(-W / 2), j = y + (int)(-H / 2), plus the sub-pixel
 * offsets for spp > 1; with ray_matrix M the direction is (M[0] * dx + M[1] * dy) + M[2] * dz and the origin M[3].xyz, without it the origin
 * is (0, 0, 0) and the direction (dx, dy, dz) as it stands -- the bits the identity matrix gives.
 * spp == 1: every output of a live pixel is bit for bit what srt_shade_paths gives for that ray with a NULL t_range, the same p (lights,
 * literals, flags) and the same path: the mixed rgb_linear and rgb8 with the background rule, and every row of seg.
 * spp = m x m > 1: sub-sample k has srt_render_device's offsets, ((k % m) + 0.5) / m - 0.5 in x and ((k / m) + 0.5) / m - 0.5 in y, added to
 * dir.xy before the matrix.  The mixed sums acc_k of the sub-samples are added in the order k = 0, 1, ... starting from acc_0, one f32 add a
 * component; each component is divided by (float)spp; tone map, quantiser and the black -> background rule run once on the quotient.  seg
 * reports sub-sample 0.  All sub-samples run in the one launch; there are no accumulation buffers.
 * Identities:  depth 1: rgb_linear and rgb8 are srt_render_device's for the same p, and rows 0 of seg.hit_id / seg.t its hit_id / t -- in
 *              camera mode and without a matrix, at any spp.  A call that owns a share of the frame writes exactly the whole-frame call's
 *              values at its owned pixels.  Results do not depend on how pixels are dealt to waves.
 * Flags: SRT_FLAG_COUNT_WORK and SRT_FLAG_SMOOTH_NORMALS as in srt_shade_paths; SRT_FLAG_NO_TIMING and SRT_FLAG_FRAMES_IN_FLIGHT are accepted
 * and ignored (the call records no events), so that a p prepared for srt_render_device can be reused; any other bit, the variant bits 8..15
 * included: SRT_ERR_ARG.
 * Errors, all before anything is touched: whatever srt_render_device rejects in the frame fields (sizes, block fields, spp), with its codes;
 * whatever srt_shade_paths rejects -- NULL path, depth 0 or above SRT_PATH_DEPTH_MAX, smooth normals on a scene without normals, n_lights > 0
 * with NULL light_pos, n x max(n_lights, 1) >= 2^32.  A call with every output NULL returns SRT_OK and launches nothing.
 * It is a query-family call: it uses the handle's query light table and query counter set, and leaves alone srt_sync, srt_scene_pipeline,
 * the renders' alternating counter sets and their workspaces.  The _device form is one kernel launch; it allocates and copies nothing
 * proportional to n; path->reflectance is read from DEVICE memory.  Without SRT_FLAG_COUNT_WORK, and with the light table already on the
 * device, it may be captured into a hipGraph.
 * The host form stages no rays; the reflectance table and the wanted outputs go through the handle's pinned block and buffers, and the call
 * waits.  *stats (may be NULL): primary_rays = owned image pixels x spp (padding excluded), hit_rays = the hits of all segments of all
 * sub-samples, shadow_rays = hit_rays x n_lights; under SRT_FLAG_COUNT_WORK the four test counters are the sums of what srt_shade_paths
 * reports for those rays. */
int srt_render_paths_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, void* stream,
                            float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_render_paths(srt_scene* s, const srt_params* p, const srt_path_desc* path,
                     float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);

/* Shadow rays with an end: srt_shade_paths / srt_render_paths under a SHADOW RULE -- an interval on every shadow ray, and optionally the hit
 * object's own tree among the occluders.  The shaded calls above keep the reference's rule (shadowIntersection:321-342): a shadow ray runs
 * from the hit point towards the light with t unbounded and the hit object's tree left out.  That suits a far light and convex objects; with a
 * lamp INSIDE the scene an object behind the lamp casts a shadow, and no object ever shadows itself.  A rule cures both.
 * Unless said here everything is as for srt_shade_paths / srt_render_paths: staging, the one-light-table-per-handle rule, the ordering on
 * `stream`, srt_scene_share, ONE kernel launch, hipGraph capture of the _device forms without SRT_FLAG_COUNT_WORK, NULL outputs and n == 0,
 * the frame fields, spp, the tile deals, seg.
 * DEFINITION.  For a hit of object obj on a ray (o, d) at t, and a light sample L:  so = o + d * t (d * t first, then o +, as ever) and
 * sd = L - so.  Under a rule r the sample is SHADOWED iff srt_occluded_range answers 1 for the ray (so, sd), the interval (r.t_min, r.t_max)
 * and skip_obj = (r.flags & SRT_SHADOW_SELF) ? -1 : obj.  So the candidate set is that call's, t is in units of L - so (t = 1 is the light), and
 * in range means !(t < t_min) && !(t > t_max): the interval is closed, a NaN bound bounds nothing, a NaN t is in range, t_min > t_max shadows
 * nothing.  Everything else of the shaded call is unchanged -- the closest hit and its interval, the surface, Phong with the ray's own o and d,
 * the sum in light order with a shadowed sample divided by shadow_div, the mix, tone map, quantiser and background rule.  One rule holds for
 * every segment of a path and every sub-sample of a pixel.
 * Identities (the existing call's bits in every output):  a NULL rule -- this one launches the existing kernels; a rule with flags == 0 whose
 * interval is (0, +inf), (-inf, +inf) or (NaN, NaN): the triangle test returns -inf, -0, a t >= 0 or NaN, never a negative finite t, and the
 * unbounded walk counts every result but -inf.
 * Depth 1 under a rule is srt_shade_rays_range under that rule (in a frame: srt_render_device in camera mode under that rule); there is no
 * further entry point for them.  srt_render_device and srt_render_batch keep the reference's rule: the frame form of a rule is
 * srt_render_paths_shadow.
 * Not validated: SRT_SHADOW_SELF with t_min <= 0 gives what the arithmetic gives -- the hit's own triangle is then a candidate near t = 0, and
 * whether it blocks depends on rounding.  Use a small positive t_min (1e-3 of the way to the light, say) with SRT_SHADOW_SELF.
 * Errors: flags with any bit but SRT_SHADOW_SELF: SRT_ERR_ARG, before anything is touched; every error of the underlying call keeps its code.
 * *stats: primary_rays, hit_rays and shadow_rays = hit_rays x n_lights as before.  Under SRT_FLAG_COUNT_WORK the two primary counters are the
 * NULL-rule call's (the primary walks do not depend on the rule); the two shadow counters count the walk as it runs: objects in order, none
 * skipped under SRT_SHADOW_SELF, one slab test per node met, triangle tests up to and including the first candidate in range. */
#define SRT_SHADOW_SELF 1u       /* the hit object's own tree is walked too */
typedef struct srt_shadow_rule {
    float    t_min, t_max;       /* a shadow ray blocks only inside the closed (t_min, t_max), in units of L - so: t = 1 is the light */
    uint32_t flags;              /* 0 or SRT_SHADOW_SELF */
} srt_shadow_rule;
int srt_shade_paths_shadow_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                  const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */, void* stream,
                                  float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_shade_paths_shadow(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                           const srt_path_desc* path, const srt_shadow_rule* shadow, float* rgb_linear, uint8_t* rgb8,
                           const srt_path_out* seg, srt_stats* stats);
int srt_render_paths_shadow_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                   void* stream, float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */,
                                   const srt_path_out* seg);
int srt_render_paths_shadow(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                            float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);

/* Visibility masks: which objects a walk sees -- per object, per ray, and per ray KIND in the shaded calls.  Every call above sees every
 * object (srt_occluded's skip_obj leaves out one tree); the calls below are their masked forms.
 * OBJECT MASKS.  A scene carries one uint32_t per object, all 0xFFFFFFFF until set.  srt_scene_set_object_masks replaces the table:
 *   masks: host memory, n_objects words; NULL = all ones.  The table belongs to the device records, like the pose source: every handle made
 *   with srt_scene_share sees it, and the ordering rule of srt_scene_update applies (the copy is ordered on `stream`, NULL = the scene's own;
 *   work enqueued earlier on that stream reads the old table, work enqueued later the new one).
 *   The table (4 B an object) is allocated by the first call, which may therefore wait; every call stages through the handle's pinned block.
 *   The masks survive srt_scene_update, _update_frame, _pose and _refit_device: the object count cannot change.
 *   Errors, before anything is touched: a NULL handle: SRT_ERR_ARG; n_objects other than the scene's: SRT_ERR_LAYOUT (the previous table
 *   stays in force).
 *   The table changes no existing call: srt_render* and every query above ignore it entirely.
 * PARTICIPATION.  Object k takes part in the walk of a ray with mask m iff (obj_mask[k] & m) != 0.  A masked walk's candidate set is the
 * unmasked call's, restricted to the triangles of participating objects; everything else holds on that set and keeps its definition -- each
 * candidate's t, the range rule, ties to the lowest id, the +0 / -0 tie, the winner's own t bits.  Triangle ids keep the scene's numbering.
 * Equivalently: the walk is the oracle on the flat scene with the other objects removed, ids mapped back.  A hidden object's tree is not
 * walked: under SRT_FLAG_COUNT_WORK its root is neither tested nor counted, and the counters are those of the unmasked call on that reduced
 * scene.
 * PER-RAY MASKS (srt_trace_rays_masked, srt_occluded_masked).  ray_mask: n words, or NULL = all ones; a pointer that is only 4-byte aligned
 * is fine.  Unless said here everything is as for srt_trace_rays_range / srt_occluded_range: layouts, a NULL t_range, flags, errors, n == 0,
 * a NULL `occluded`, staging (ray_mask goes through the same pinned block as t_range), stats, the private counter set, hipGraph capture of
 * the _device forms without SRT_FLAG_COUNT_WORK (the table is read when the kernel runs), one launch with no allocation and no copy.
 *   skip_obj still applies, on top of the masks.  A ray mask of 0 is a miss / not occluded, and no node is tested for that ray.
 *   Identity: with the table all ones or never set, and ray_mask NULL or all ones, every output has the _range call's bits, and the counters
 *   are equal too.
 * PER RAY KIND (srt_shade_paths_masked, srt_render_paths_masked).  Everything is as for srt_shade_paths_shadow / srt_render_paths_shadow,
 * except which objects a walk sees: segment 0 is walked with vis->primary, every segment b >= 1 with vis->bounce, every shadow ray with
 * vis->shadow.
 *   A segment's hit_id / t are srt_trace_rays_masked's for that segment's ray, interval and mask.  A sample is SHADOWED iff
 *   srt_occluded_masked answers 1 for the shadow ray with mask vis->shadow and the rule's interval and skip; a NULL rule is the reference's:
 *   unbounded, with the hit's object skipped.  The surface, Phong, the sum, the mix, the tone map and the background rule are unchanged.
 *   vis == NULL: the call IS the _shadow call, and launches its kernels.
 *   Identity: a table of all ones with vis = { ~0, ~0, ~0 } gives the _shadow call's bits in every output.
 *   Depth 1 is the masked form of srt_shade_rays_range (in a frame: of srt_render_device in camera mode); there is no further entry point.
 *   *stats: as for the _shadow calls; the primary counters count the masked walks, the shadow counters the walk as it runs -- objects in
 *   order, hidden and skipped objects not entered.
 * So: a pick among selectable objects is a ray mask; an object that casts no shadow has no bit of vis->shadow; a holdout -- hidden from the
 * camera, present in mirrors and shadows -- has no bit of vis->primary; an object is switched off for a frame by a mask of 0 in the table.
 * NOT HERE: masks for srt_trace_rays_multi and srt_surface_rays -- feed a masked trace's hit_id / t to srt_surface_hits instead -- and
 * per-ray masks inside the shaded calls. */
typedef struct srt_visibility { uint32_t primary, bounce, shadow; } srt_visibility;
int srt_scene_set_object_masks(srt_scene* s, uint32_t n_objects, const uint32_t* masks /* host, n_objects; NULL = all ones */, void* stream);
int srt_trace_rays_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                 const uint32_t* d_ray_mask /* n or NULL = all ones */, uint32_t flags, void* stream,
                                 int32_t* d_hit_id, float* d_t, float* d_bary);
int srt_trace_rays_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const uint32_t* ray_mask, uint32_t flags,
                          int32_t* hit_id, float* t, float* bary, srt_stats* stats);
int srt_occluded_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                               const uint32_t* d_ray_mask /* n or NULL = all ones */, const int32_t* d_skip_obj, void* stream,
                               uint8_t* d_occluded);
int srt_occluded_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const uint32_t* ray_mask,
                        const int32_t* skip_obj, uint8_t* occluded);
int srt_shade_paths_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                  const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                  const srt_visibility* vis /* or NULL */, void* stream,
                                  float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_shade_paths_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                           const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis,
                           float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);
int srt_render_paths_masked_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                   const srt_visibility* vis /* or NULL */, void* stream,
                                   float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_render_paths_masked(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                            const srt_visibility* vis, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);

/* Refracting paths: glass objects in srt_shade_paths and srt_render_paths.  Until here the only thing a ray does at a surface is bounce
 * off it; the calls below take one more per-object table, and a hit on a TRANSMITTING object sends the next segment THROUGH the surface,
 * bent by Snell's law.  Unless said here everything is as for srt_shade_paths_masked / srt_render_paths_masked: the rule, vis, seg, staging
 * (ior goes through the pinned block exactly as reflectance does), the one-light-table-per-handle rule, ordering on `stream`,
 * srt_scene_share, ONE kernel launch, hipGraph capture of the _device forms without SRT_FLAG_COUNT_WORK, NULL outputs, n == 0, the frame
 * fields, spp, the tile deals, *stats.
 * THE TABLE.  refr->ior: n_objects floats -- a device pointer in the _device forms, a host pointer in the host forms.  Object k transmits
 * iff ior[k] > 0.0f; with 0, a negative value or NaN it mirrors, as ever.  refr->flags must be 0.
 * THE RAY of segment b + 1 when segment b hit a transmitting object.  d: the direction of segment b; N: the normal shading uses for that
 * hit (the smooth one under SRT_FLAG_SMOOTH_NORMALS); n = ior[obj_b].  f32 without contraction, dot3 = (x + y) + z, correctly rounded
 * square root and divide:
 *   L   = sqrtf(dot3(d, d));   inv = 1.0f / L;   I_i = d_i * inv            (glm::normalize's operations)
 *   c   = dot3(N, I)                                                        (N's components on the left)
 *   entering = c < 0.0f                                                     (N points OUT of the solid: the contract)
 *   Nf  = entering ? N : -N;   dv = entering ? c : -c;   eta = entering ? 1.0f / n : n
 *   k   = 1.0f - (eta * eta) * (1.0f - dv * dv)                             (glm::refract's association)
 *   k < 0.0f  (total internal reflection):   r = the mirrored direction, exactly srt_surface_out.bounce's (d not normalised)
 *   otherwise (k >= 0 or NaN):               s = eta * dv + sqrtf(k);   u_i = eta * I_i - s * Nf_i;   r_i = u_i * L
 *   The origin is o + d * t, not moved, and the interval (bounce_t_min, +inf), as for a mirrored ray.  r is scaled back by L, so t of the
 *   next segment stays in the units of the caller's direction and bounce_t_min means the same on every segment, whichever way the ray went.
 *   The closest-hit walk does not skip the hit's own object: a ray that enters a solid finds its far side.
 * THE MIX is unchanged: reflectance[obj] is the weight of what the NEXT segment brings, whether that segment was reflected or transmitted
 * (a clear glass has a reflectance near 1: most of what one sees on it comes from behind it).
 * SHADING AND SHADOWS are unchanged: every hit is shaded exactly as before, a hit on a back face from the inside included, and a glass
 * object shadows like any other -- unless it has no bit of vis->shadow.  Under SRT_SHADOW_SELF a point inside a solid is shadowed by it.
 * ORIENTATION.  `entering` trusts the normals: a mesh whose normals point inward refracts inside out (it bends rays as a bubble of air in
 * glass would).  Values are not validated: a zero direction, an ior of +inf and the like give what the arithmetic gives; the call stays
 * memory-safe.
 * IDENTITIES, in every output and all four counters: refr == NULL or refr->ior == NULL: the call IS the _masked call and launches its
 * kernels; a table with no entry > 0 gives the _masked call's bits; depth 1 is unchanged by any table.
 * ERRORS: refr->flags != 0: SRT_ERR_ARG before anything is touched; every error of the _masked call keeps its code.
 * NOT HERE: absorption along the way, srt_surface_out reporting a refracted ray.  (A Fresnel split: the _fresnel calls below.) */
typedef struct srt_refraction {
    const float* ior;     /* n_objects floats; object k TRANSMITS iff ior[k] > 0.0f (0, negative, NaN: it mirrors) */
    uint32_t     flags;   /* 0; any other value: SRT_ERR_ARG */
} srt_refraction;
int srt_shade_paths_refract_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                   const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                   const srt_visibility* vis /* or NULL */, const srt_refraction* refr /* or NULL */, void* stream,
                                   float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_shade_paths_refract(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                            const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis, const srt_refraction* refr,
                            float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);
int srt_render_paths_refract_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                    const srt_visibility* vis /* or NULL */, const srt_refraction* refr /* or NULL */, void* stream,
                                    float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_render_paths_refract(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                             const srt_visibility* vis, const srt_refraction* refr, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg,
                             srt_stats* stats);

/* Fresnel split: glass that also reflects.  In the _refract calls the whole weight of what follows a glass hit goes through the surface.
 * The calls below take one more per-object table, f0, the reflectance at normal incidence, and at a hit on an object that SPLITS the path
 * goes on through the glass, as before, while the mirrored ray at that hit is walked once and shaded once -- a depth-1 SIDE RAY -- and its
 * colour enters the mix with Schlick's weight.  A path stays a row, not a tree: a side ray's hit sends no further ray.  Unless said here
 * everything is as for srt_shade_paths_refract / srt_render_paths_refract: the rule, vis, refr and its flags, seg, staging (f0 and the
 * four fields of `out` go through the pinned block and the handle's buffers exactly as ior and seg do), the one-light-table-per-handle
 * rule, ordering on `stream`, srt_scene_share, ONE kernel launch, hipGraph capture of the _device forms without SRT_FLAG_COUNT_WORK, n == 0,
 * the frame fields, spp (`out` reports sub-sample 0), the tile deals (padding pixels are not written in any output).
 * THE TABLE.  fres->f0: n_objects floats -- a device pointer in the _device forms, a host pointer in the host forms.  Object k SPLITS iff
 * ior[k] > 0.0f && f0[k] >= 0.0f; a negative or NaN f0[k] means no split at that object.  fres->flags must be 0.
 * WHEN A SIDE RAY IS WALKED.  The side ray of segment b is walked iff segment b hit an object that splits, b + 1 < depth, and the hit was
 * not totally reflected: !(k < 0.0f) with the k of "Refracting paths" -- a NaN k goes the split way and gives what the arithmetic gives.
 * This is purely geometric: no value of f0 or reflectance changes which rays are walked.
 * THE SIDE RAY is the `bounce` row srt_surface_rays defines for that hit under the call's flags: origin o + d * t, not moved, direction the
 * mirrored one (d not normalised).  Its interval is (bounce_t_min, +inf), it is walked with the mask vis->bounce, and its hit is shaded
 * exactly as a segment's is: the same shadow rule, vis->shadow, lights and literals.  Nothing bounces off its hit; the reflectance of the
 * object it hits is not read.
 * THE WEIGHT.  f32 without contraction, from the intermediates of "Refracting paths" for segment b (entering, dv, k):
 *   x  = entering ? -dv : sqrtf(k)                      (the cosine on the thin side: the incident one going in, the transmitted one going out)
 *   m  = 1.0f - x;   m2 = m * m;   m5 = (m2 * m2) * m
 *   F  = f0[obj] + (1.0f - f0[obj]) * m5                (Schlick's polynomial; nothing is clamped or validated)
 * THE MIX of a segment b with a side ray, in the place of the mix of srt_shade_paths; W: the weight of what follows, nxt: segment b + 1
 * hits, side: the side ray hits, lin_b: segment b's sum, S_b: the side hit's sum:
 *   k  = (nxt || side) ? reflectance[obj_b] : 0         (NULL table: 0)
 *   a  = W * (1 - k);   acc_i = acc_i + a * lin_b_i;   Wk = W * k
 *   Fe = side ? (nxt ? F : 1.0f) : 0.0f                 (a branch that misses gives its share to the other)
 *   if side:  g = Wk * Fe;   acc_i = acc_i + g * S_b_i  (one multiply, then one add)
 *   W  = Wk * (1.0f - Fe)
 * Segments without a side ray mix as before.
 * `out` (may be NULL, and so may any field): per SEGMENT, segment-major like srt_path_out -- row b of hit_id / t / rgb_linear is laid out
 * as seg's hit_id / t / rgb_linear.  Row b reports the side ray of segment b: what it hit and where (the winner's own t bits), the side
 * hit's pre-tone-map sum S_b, and F_b.  Without a side ray: -1, +inf, 0 and 0.  `out` is written by a call that brings both tables.
 * IDENTITIES, in every output and all four counters: fres == NULL or fres->f0 == NULL: the call IS the _refract call and launches its
 * kernels (so does a call without refr->ior: nothing can split); a table under which no object splits gives the _refract call's bits; so
 * does a call in which every side ray misses (Wk * (1.0f - 0.0f) is Wk); depth 1 is unchanged by any table; at depth D the rows b < D - 1
 * of `out` are those rows at any larger depth, and row D - 1 holds no side ray (b + 1 < depth); results never depend on the order of the rays.
 * *stats: primary_rays is unchanged; hit_rays and shadow_rays = hit_rays x n_lights include the side hits.  Under SRT_FLAG_COUNT_WORK the
 * four counters are the _refract call's on the same tables plus, per side ray walked, what the depth-1 _masked call reports for that ray
 * with the interval (bounce_t_min, +inf), vis' = { bounce, bounce, shadow } and the same rule.
 * ERRORS: fres->flags != 0: SRT_ERR_ARG before anything is touched; every error of the _refract call keeps its code.  A call with every
 * output NULL, the fields of `out` included, returns SRT_OK and launches nothing.
 * NOT HERE: a recursive split (a side ray of a side ray), absorption inside a solid. */
typedef struct srt_fresnel_out {   /* per SEGMENT, segment-major like srt_path_out; any pointer may be NULL, and so may the struct */
    int32_t* hit_id;       /* depth x n      the side ray of segment b: what it hit, -1 = miss or no side ray */
    float*   t;            /* depth x n      +inf on a miss or without a side ray                              */
    float*   rgb_linear;   /* depth x n x 3  the side hit's own pre-tone-map sum S_b; 0 otherwise              */
    float*   fresnel;      /* depth x n      F_b where a side ray was walked, else 0                           */
} srt_fresnel_out;
typedef struct srt_fresnel {
    const float*           f0;     /* n_objects floats: reflectance at normal incidence; device pointer in the _device forms */
    uint32_t               flags;  /* 0; any other value: SRT_ERR_ARG */
    const srt_fresnel_out* out;    /* or NULL */
} srt_fresnel;
int srt_shade_paths_fresnel_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */,
                                   const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                   const srt_visibility* vis /* or NULL */, const srt_refraction* refr /* or NULL */,
                                   const srt_fresnel* fres /* or NULL */, void* stream,
                                   float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_shade_paths_fresnel(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p,
                            const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis, const srt_refraction* refr,
                            const srt_fresnel* fres, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats);
int srt_render_paths_fresnel_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow /* or NULL */,
                                    const srt_visibility* vis /* or NULL */, const srt_refraction* refr /* or NULL */,
                                    const srt_fresnel* fres /* or NULL */, void* stream,
                                    float* d_rgb_linear /* n x 3, mixed */, uint8_t* d_rgb8 /* n x 3 */, const srt_path_out* seg);
int srt_render_paths_fresnel(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                             const srt_visibility* vis, const srt_refraction* refr, const srt_fresnel* fres, float* rgb_linear, uint8_t* rgb8,
                             const srt_path_out* seg, srt_stats* stats);

/* Ambient occlusion: how open the surface is at a hit -- the hemisphere visibility behind ambient occlusion, sky visibility and contact
 * shadows -- in ONE launch: the closest hit, the surface there, a tangent frame, n_dirs short occlusion rays from the hit point and their
 * count; the chain srt_surface_rays -> a kernel of the caller's that writes n x n_dirs rays -> srt_occluded_masked -> a reduction, without
 * the rays ever reaching memory.  srt_ao_rays finds the hit itself; srt_ao_hits takes hits the caller already holds (a render's hit_id / t
 * with the frame's rays, any column of srt_trace_rays_multi) and walks no primary ray, as srt_surface_hits relates to srt_surface_rays:
 * an AO pass over a rendered frame needs no second closest-hit walk.
 * Unless said here everything is as for srt_trace_rays_masked / srt_surface_hits: the layout of rays and t_range with wide loads where they
 * are 8-byte aligned, a NULL t_range, the ordering on `stream`, the rules of srt_scene_share, the private counter set, hipGraph capture of
 * the _device forms without SRT_FLAG_COUNT_WORK, ONE launch with nothing allocated and nothing copied.
 * DEFINITION.
 *   The hit     srt_ao_rays: hit_id, t are bit for bit srt_trace_rays_masked's for that ray, interval and the ray mask vis->primary
 *               (vis == NULL: all ones).  srt_ao_hits: row i is a miss row if hit_id[i] is outside [0, n_tris); t is taken as given.
 *               The surface is srt_surface_out's: P = o + d * t (`point`), N the `normal` shading uses for that hit (the smooth one under
 *               SRT_FLAG_SMOOTH_NORMALS).
 *   The frame   all f32, no contraction, no transcendental:
 *                   k  = (d.x * N.x + d.y * N.y) + d.z * N.z              (the dot of srt_surface_out.bounce)
 *                   Nf = k > 0 ? -N : N                                   (the normal that FACES the ray; a NaN or zero k flips nothing)
 *               and with (x, y, z) = Nf:
 *                   s = copysignf(1.0f, z);   a = -1.0f / (s + z);   b = (x * y) * a
 *                   T = ( 1.0f + ((s * x) * x) * a,   s * b,               (-s) * x )
 *                   B = ( b,                          s + (y * y) * a,     -y       )
 *               Nothing is normalised.  For a unit N the three are orthonormal to rounding, also at N = (0, 0, +-1).
 *   The AO ray  j of a hit: origin P, not moved; direction, with (u, v, w) = dirs[j],
 *                   w_i = (T_i * u + B_i * v) + Nf_i * w
 *               so a table lives in the hit's LOCAL frame, z along the facing normal.
 *   Blocked     direction j is blocked iff srt_occluded_masked answers 1 for the ray (P, w) with the interval (ao->t_min, ao->t_max), the ray
 *               mask vis->shadow (vis == NULL: all ones) and skip_obj = (ao->flags & SRT_AO_SKIP_SELF) ? obj : -1.  Every rule of that call
 *               is inherited as it stands: the closed interval in units of w, NaN bounds bounding nothing, a NaN t counting, hidden trees
 *               not being walked.  vis->bounce is ignored.
 *   A miss row  n_occluded 0, ao 1.0f, every word of occ_bits 0.
 * Not validated: t_min <= 0 lets the hit's own triangle block near t = 0, depending on rounding (whole hemispheres then read as closed): use
 * a small positive t_min, as with SRT_SHADOW_SELF.  Directions that are not unit, lie below the horizon, are zero or not finite, NaN and
 * zero normals, degenerate triangles, a valid hit_id with any t (NaN, +-inf, 0, negative, another triangle's), and t_min <= 0 give what the
 * arithmetic of the DEFINITION gives, bit for bit -- pinned by tests/ao_edges.py and tests/test_gpu_ao_edges.py against tests/ao_ref.py --;
 * the call stays memory-safe.
 * Flags: 0, SRT_FLAG_COUNT_WORK, SRT_FLAG_SMOOTH_NORMALS or both; SRT_FLAG_SMOOTH_NORMALS on a scene without normals fails as
 * srt_surface_rays does.
 * Errors, all before anything is touched.  SRT_ERR_ARG: a NULL handle; NULL rays with n > 0; NULL hit_id or t in srt_ao_hits with n > 0; a NULL
 * ao, a NULL ao->dirs or n_dirs == 0; ao->flags with any bit but SRT_AO_SKIP_SELF; any other flag bit.  SRT_ERR_LIMIT: n_dirs >
 * SRT_AO_DIRS_MAX; n * n_dirs >= 2^32.  n == 0: SRT_OK.
 * out == NULL, or every field of it NULL: srt_ao_rays IS srt_trace_rays_masked without bary -- it launches that kernel when vis->primary is
 * all ones or vis is NULL (that call takes its masks per ray, from an array; any other vis->primary runs this call's own kernel without a
 * direction) --; srt_ao_hits launches nothing.
 * Identities: srt_ao_hits fed srt_ao_rays' hit_id / t gives that call's bits in every field; results never depend on the order of the rays;
 * a direction's bit does not depend on the other directions of the table -- the row of a table is the concatenation of the rows of its
 * parts --; vis = { ~0, ~0, ~0 } equals vis == NULL, and with a table of all ones both equal the call on a scene whose masks were never set.
 * The host forms stage rays, t_range, dirs, hit_id / t and the outputs through the handle's pinned block, then wait.  *stats: primary_rays = n,
 * hit_rays, shadow_rays = hit_rays x n_dirs (0 where nothing of srt_ao_out is wanted: no AO ray is walked then); under
 * SRT_FLAG_COUNT_WORK the primary counters are srt_trace_rays_masked's (0 in srt_ao_hits) and the shadow counters count the AO walks as they run -- objects in order, hidden and skipped objects not entered, one slab test per
 * node met, triangle tests up to and including the first candidate in range.
 * NOT HERE: weights per direction (a cosine-distributed table makes the plain count cosine-weighted).  (A per-pixel rotation or jitter
 * of the table, bent normals and a frame form without a ray array: the srt_render_ao calls below, "Ambient occlusion in a frame".) */
#define SRT_AO_DIRS_MAX  1024
#define SRT_AO_SKIP_SELF 1u      /* the hit object's own tree is left out of the AO walks (default: it is walked) */
typedef struct srt_ao_desc {
    uint32_t     n_dirs;         /* 1 .. SRT_AO_DIRS_MAX */
    const float* dirs;           /* n_dirs x 3 (x, y, z) in the hit's LOCAL frame, z along the facing normal; a host pointer in the host forms, a
                                    DEVICE pointer in the _device forms (read when the kernel runs, as path->reflectance is) */
    float        t_min, t_max;   /* every AO ray blocks only inside the closed (t_min, t_max), in units of its direction */
    uint32_t     flags;          /* 0 or SRT_AO_SKIP_SELF */
} srt_ao_desc;
typedef struct srt_ao_out {      /* device pointers in the _device forms, host pointers in the host forms; any may be NULL, and so may the struct */
    uint32_t* n_occluded;        /* n        directions that are blocked */
    float*    ao;                /* n        (float)(n_dirs - n_occluded) / (float)n_dirs: one IEEE divide */
    uint32_t* occ_bits;          /* n x W, W = (n_dirs + 31) / 32: bit (k & 31) of word k >> 5 set iff direction k is blocked; bits >= n_dirs are 0 */
} srt_ao_out;
int srt_ao_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range /* n x 2 or NULL */, uint32_t flags,
                       const srt_ao_desc* ao, const srt_visibility* vis /* or NULL */, void* stream, int32_t* d_hit_id, float* d_t,
                       const srt_ao_out* out);
int srt_ao_rays(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, const srt_ao_desc* ao,
                const srt_visibility* vis, int32_t* hit_id, float* t, const srt_ao_out* out, srt_stats* stats);
int srt_ao_hits_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_hit_id, const float* d_t, uint32_t flags,
                       const srt_ao_desc* ao, const srt_visibility* vis /* or NULL */, void* stream, const srt_ao_out* out);
int srt_ao_hits(srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t, uint32_t flags,
                const srt_ao_desc* ao, const srt_visibility* vis, const srt_ao_out* out, srt_stats* stats);

/* Ambient occlusion in a frame: srt_ao_rays for the rays of a frame's own pixels -- the AO pass over a frame in ONE launch without a ray
 * array (24 B a pixel that srt_ao_rays reads and the caller has to write) -- plus the two things a frame pass needs and a ray batch does
 * not: a rotation of the direction table chosen by the pixel, which turns the banding of a small table into noise a blur removes, and
 * the bent normal.  srt_render_ao finds the hits itself; srt_render_ao_hits takes the hit_id / t of a render of the same frame and walks
 * no primary ray.  They relate to srt_ao_rays / srt_ao_hits as srt_render_paths relates to srt_shade_paths.
 * Unless said here everything is as for srt_ao_rays: ao, vis, flags, the ordering on `stream`, the rules of srt_scene_share, the private
 * counter set (srt_sync, srt_scene_pipeline and the renders' counter sets are left alone), ONE launch with nothing allocated and nothing
 * copied, hipGraph capture of the _device forms without SRT_FLAG_COUNT_WORK.
 * DEFINITION.  Everything is bit for bit; f32 arithmetic is uncontracted and uses no transcendental.
 *   Pixels      exactly as in srt_render_paths: the call writes its n = srt_rows_owned x srt_cols_owned LOCAL pixels, row-major; which image
 *               pixel a local pixel is comes from block_rows / block_first / block_stride / block_cols; the ray of a pixel is
 *               srt_render_device's, in camera mode (ray_matrix) and without a matrix; padding pixels of a tile deal are written in no
 *               output.  Of *p the calls read the frame fields and spp; lights, tone-map literals and background are ignored.
 *   Rotation    with (x, y) the IMAGE pixel of a live pixel -- image coordinates, not local ones, so that a share of a frame agrees with
 *               the whole frame --: (c, s) = rot[((y % rot_h) * rot_w + x % rot_w) * 2 ..], and for (u, v, w) = dirs[j] the pixel's table
 *               entry is
 *                   u' = c * u - s * v      v' = s * u + c * v      w' = w               (each product rounded on its own)
 *               fr == NULL or fr->rot == NULL applies no arithmetic at all (it is not a multiplication by (1, 0)).  (c, s) is neither
 *               validated nor normalised.
 *   The AO      of a pixel: everything of srt_ao_rays for that ray with a NULL t_range, the pixel's table dirs', the same ao->t_min /
 *               t_max / flags, vis and flags.  hit_id, t, n_occluded, ao and occ_bits are that call's bits.
 *   bent        from (+0, +0, +0): for j = 0 .. n_dirs - 1 in ascending order, if direction j is NOT blocked, the AO ray's direction as
 *               walked is added, one f32 add per component.  The sum is not normalised; its order is part of the contract.  A miss row is
 *               (0, 0, 0).
 *   ao8         (uint8_t)(int)(ao * 255.0f + 0.5f), the product and the sum each rounded.  A miss gives 255.
 *   spp = m x m > 1   (srt_render_ao only) the sub-samples run in the one launch with srt_render_device's offsets.  hit_id, t, n_occluded,
 *               occ_bits and bent report sub-sample 0; ao is the sub-samples' ao values added in order starting from sub-sample 0's, then
 *               divided by (float)spp -- a miss counts 1.0f --, and ao8 is taken from that quotient.
 *   srt_render_ao_hits   hit_id and t are laid out as srt_render_device writes them for the same *p.  No primary ray is walked.  Only
 *               sub-sample 0's ray is used -- that is what a render's hits are -- and ao is that sub-sample's value.  An id outside
 *               [0, n_tris) is a miss row; t is taken as given.
 * Identities: with rot NULL and spp 1 the rows equal srt_ao_rays on the frame's rays; srt_render_ao's hit_id / t are srt_render_device's
 * for the same *p when vis is NULL; the _hits form fed those gives the ray form's bits in every field; a call that owns a share of the
 * frame writes the whole-frame call's values at its owned pixels; a direction's bit does not depend on the rest of the table.
 * Flags: SRT_FLAG_COUNT_WORK and SRT_FLAG_SMOOTH_NORMALS as in srt_ao_rays; SRT_FLAG_NO_TIMING and SRT_FLAG_FRAMES_IN_FLIGHT in p->flags are
 * accepted and ignored, as in srt_render_paths (`flags` itself takes the first two only).
 * Errors, all before anything is touched: what srt_render_device rejects in the frame fields, with its codes; what srt_ao_rays rejects in ao
 * and flags; SRT_ERR_ARG for rot non-NULL with rot_w or rot_h 0, for rot NULL with either non-zero, and for a NULL hit_id or t in the _hits
 * forms; SRT_ERR_LIMIT for rot_w or rot_h above SRT_AO_ROT_MAX and for n x n_dirs x spp >= 2^32.
 * out == NULL, or every field of it NULL: the _hits forms launch nothing and return SRT_OK; the ray forms still write hit_id / t.
 * The host forms stage dirs, rot, the given hits and the outputs through the handle's pinned block, then wait.  *stats: primary_rays = owned
 * image pixels x spp (the _hits forms: owned image pixels), hit_rays = the hits of all sub-samples, shadow_rays = hit_rays x n_dirs; under
 * SRT_FLAG_COUNT_WORK the four test counters are the sums of what srt_ao_rays reports for those rays.
 * NOT HERE: weights per direction, as above; a rotation that differs per sub-sample; a blur of the result (a 4 x 4 table wants a 4 x 4 box
 * filter, which is the caller's). */
#define SRT_AO_ROT_MAX 64
typedef struct srt_ao_frame {
    uint32_t     rot_w, rot_h;   /* 0, 0 with rot NULL: no rotation.  Else 1 .. SRT_AO_ROT_MAX each */
    const float* rot;            /* rot_h x rot_w x 2 floats (c, s), row-major; a host pointer in the host forms, a DEVICE pointer in the
                                    _device forms (read when the kernel runs, as ao->dirs is) */
} srt_ao_frame;
typedef struct srt_ao_frame_out {   /* device pointers in the _device forms, host pointers in the host forms; any may be NULL, and so may the
                                       struct; n local pixels, row-major */
    uint32_t* n_occluded;        /* n        directions that are blocked (sub-sample 0) */
    float*    ao;                /* n        srt_ao_out's ao; over the sub-samples where spp > 1 */
    uint32_t* occ_bits;          /* n x W, W = (n_dirs + 31) / 32, as srt_ao_out's (sub-sample 0) */
    float*    bent;              /* n x 3    the sum of the unblocked directions (sub-sample 0) */
    uint8_t*  ao8;               /* n        ao as a byte */
} srt_ao_frame_out;
int srt_render_ao_device(srt_scene* s, const srt_params* p, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr /* or NULL */,
                         const srt_visibility* vis /* or NULL */, void* stream, int32_t* d_hit_id, float* d_t, const srt_ao_frame_out* out);
int srt_render_ao(srt_scene* s, const srt_params* p, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr, const srt_visibility* vis,
                  int32_t* hit_id, float* t, const srt_ao_frame_out* out, srt_stats* stats);
int srt_render_ao_hits_device(srt_scene* s, const srt_params* p, const int32_t* d_hit_id, const float* d_t, uint32_t flags,
                              const srt_ao_desc* ao, const srt_ao_frame* fr /* or NULL */, const srt_visibility* vis /* or NULL */,
                              void* stream, const srt_ao_frame_out* out);
int srt_render_ao_hits(srt_scene* s, const srt_params* p, const int32_t* hit_id, const float* t, uint32_t flags, const srt_ao_desc* ao,
                       const srt_ao_frame* fr, const srt_visibility* vis, const srt_ao_frame_out* out, srt_stats* stats);

/* Device-resident size of the scene records and the per-record algorithmic byte sizes used by
 * the bytes model: 32 B per node test, 36 B per triangle test. */
uint64_t srt_scene_device_bytes(const srt_scene* s);

/* Which kernels the last srt_render* on this scene launched, in order, e.g. "k_trace_nq+k_shade_tile" (DESIGN.md s5 explains
 * how the pipeline is chosen per scene and light-sample count).  The string lives as long as the scene. */
const char* srt_scene_pipeline(const srt_scene* s);

/* Expected slab tests per ray from the surface areas of the scene's node boxes (what decides whether primary rays take the
 * packet walk: hierarchies of heavily overlapping boxes do). */
double srt_scene_overlap_estimate(const srt_scene* s);

/* ---- known-answer entry points: the DEVICE leaf functions on caller vectors (host pointers), so that the
 * reference's known-answer fixtures pin the device code directly.  Layouts as in tests/golden/kat.npz:
 * ray_od = n x (origin xyz, direction xyz); box = n x (min xyz, max xyz); tri_points = n x 3 x xyzw.
 *   srt_kat_ray_aabb      intersectRayAabbNoOrigin (simple_raytracer.cpp:252-293): the literal form, the
 *                         branch-free form and the filtered form (+ its "ambiguous, use the exact form" flag)
 *   srt_kat_ray_triangle  rayTriangleIntersection (:42-75): t, -inf = miss
 *   srt_kat_phong         phongIllumination (:144-200): in28 = ray_od(6) tri(12) light(3) colour(3) ka ks shin t
 *   srt_kat_tonemap       Reinhard + gamma (:391-398) and the quantiser (:447-449)                         */
int srt_kat_ray_aabb(int device, uint32_t n, const float* ray_od, const float* box, uint8_t* exact, uint8_t* branchless,
                     uint8_t* filtered, uint8_t* ambiguous);
int srt_kat_ray_triangle(int device, uint32_t n, const float* ray_od, const float* tri_points, float* t);
/* rayTriangleIntersection for rays FROM THE ORIGIN, as every primary ray runs it: both triangle records are derived as
 * srt_scene_create derives them and the test reads the one that carries tvec and qvec.  dir = n x 3; t as above. */
int srt_kat_ray_triangle_origin(int device, uint32_t n, const float* dir /* n x 3 */, const float* tri_points, float* t);
/* calculateBarycentricCoords (:79-117): in15 = tri_points(12) point(3), out3 = (u, v, w) */
int srt_kat_barycentric(int device, uint32_t n, const float* in15, float* out3);
int srt_kat_phong(int device, uint32_t n, const float* in28, float* rgb);
int srt_kat_interp_normal(int device, uint32_t n, const float* in12 /* 3 normals + barycentrics */, float* out3);   /* interpolateNormal :132-140 */
int srt_kat_pow(int device, uint32_t n, const float* x, const float* y, float* fast, float* lib);   /* the device powf: shipped form vs (float)pow(double) */
int srt_kat_tonemap(int device, uint32_t n, const float* lin, float reinhard, float gamma, float* tone, int32_t* q);
/* The quantised tone map as the shading kernels compute it -- an f32 filter that decides the 8-bit value where a margin allows, the exact
 * functions (srt_kat_tonemap's) where it does not -- for n VALUES (not pixels): q = what a pixel's channel gets, q_filter = the filter's
 * own candidate (-1 where it decided nothing), decided = 1 where the filter alone decided.  q equals srt_kat_tonemap's q on every input. */
int srt_kat_tone_filter(int device, uint32_t n, const float* lin, float reinhard, float gamma, int32_t* q, int32_t* q_filter, uint8_t* decided);
/* The same comparison for every float whose bit pattern lies in [first_bits, last_bits], reduced on the device.  out6: [0] values,
 * [1] undecided by the filter, [2] decided and different from the exact functions, [3] different after the fallback (what a pixel gets),
 * [4] the largest relative deviation of the filter's 255 * tone from the exact one over decided values, [5] the largest of that deviation
 * over the margin the filter allowed for it ([4] and [5] over values whose exact 255 * tone is at least 1e-30). */
int srt_kat_tone_filter_sweep(int device, uint32_t first_bits, uint32_t last_bits, float reinhard, float gamma, double* out6);

/* Measurement hook: the chip's VALU issue rate from independent v_fma_f32 streams at 8 waves per SIMD (the yardstick bench.py's
 * roofline prices the kernels' VALU work against).  out[0] = wave-instructions one SIMD issues per cycle (MI355X: SIMD-32, a wave64
 * instruction over 2 cycles -> 0.5), out[1] = shader clock in GHz during the run, out[2] = the same rate over the whole launch span. */
int srt_debug_valu_rate(int device, uint32_t iters, double* out4);      /* out[3] = waves that shared a SIMD (median) */

/* Test hook: the device records of a scene copied back (any pointer may be NULL): nodes n_nodes x 32 B, tris / tris_o n_tris x 48 B, wide
 * (n_nodes - n_objects) / 2 x 64 B, root_nodes n_objects x 32 B, tri_texcoord n_tris x 6 floats, tri_normals n_tris x 9 floats, tri_tex
 * n_tris ids (the last three only where the scene has them).  Waits for the scene's pending work first.  What srt_scene_update_frame
 * derives on the device is compared, byte for byte, with what srt_scene_create derives on the host. */
int srt_debug_scene_records(srt_scene* s, void* nodes, void* tris, void* tris_o, void* wide, void* root_nodes,
                            float* tri_texcoord, float* tri_normals, int32_t* tri_tex);

/* Test hook: the next n host allocations made on behalf of a caller fail (std::bad_alloc inside the library), so that
 * the SRT_ERR_OOM path can be exercised without exhausting memory.  Not for production use. */
void srt_debug_fail_host_allocs(int n);

const char* srt_strerror(int code);
int         srt_last_hip_error(void);
uint32_t    srt_abi_version(void);

#ifdef __cplusplus
}
#endif

/* Closest-point queries, the nearest triangle within a radius per point, are declared in their own header, which this one brings along:
 * include/srt_points.h states their definition.  SRT_ABI_VERSION is unchanged by them. */
#include "srt_points.h"
#include "srt_nearest.h"      /* the same query with a bound that shrinks: no radius to choose */
#include "srt_signed.h"       /* that distance with a sign, and containment, by winding along a few rays */
#include "srt_points_multi.h" /* the K nearest triangles per point, in either walk: all contacts within a radius */
#include "srt_segments.h"     /* the nearest triangle to a SEGMENT within a radius: swept particles, capsules, clearance along a path */
#endif /* SRT_H */
