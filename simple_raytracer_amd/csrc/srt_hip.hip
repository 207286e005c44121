// srt_hip.hip -- HIP kernels (gfx950) and the extern "C" ABI of include/srt.h.
//
// Path replaced: sendRaysAndIntersectPointsColors -> rayIntersection -> boundingBoxIntersection /
// intersectRayAabbNoOrigin -> rayTriangleIntersection -> softShadow -> shadowIntersection +
// phongIllumination (/root/reference/simple_raytracer.cpp:505-525, 405-457, 296-317, 252-293, 42-75,
// 348-401, 321-342, 144-200).  No CPU fallback exists in this library.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <atomic>
#include <deque>
#include <map>
#include <memory>
#include <new>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/srt.h"
#include "srt_device.h"

using namespace srt;

#include "srt_kernels.h"
#include "srt_packet.h"
#include "srt_query.h"

// =================================================================================================
// Host side of the ABI
// =================================================================================================
static thread_local int g_last_hip = 0;
#define HIP_TRY(expr)                                                  \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) { g_last_hip = (int)e_; return SRT_ERR_DEVICE; } \
    } while (0)

// No C++ exception may cross the extern "C" boundary ("never throws"): every entry point that allocates
// or spawns threads runs its body through guarded().
template <typename F>
static int guarded(F&& body) noexcept {
    try { return body(); }
    catch (const std::bad_alloc&) { return SRT_ERR_OOM; }
    catch (...) { return SRT_ERR_DEVICE; }
}
// Test hook (srt_debug_fail_host_allocs): the next n guarded host allocations throw std::bad_alloc.
static std::atomic<int> g_fail_allocs{0};
static inline void alloc_gate() {
    int n = g_fail_allocs.load(std::memory_order_relaxed);
    while (n > 0 && !g_fail_allocs.compare_exchange_weak(n, n - 1)) {}
    if (n > 0) throw std::bad_alloc();
}

#define SRT_TRY(expr) do { int rc_ = (expr); if (rc_ != SRT_OK) return rc_; } while (0)

constexpr double PACKET_OVERLAP_THRESHOLD = 150.;     // expected slab tests per ray from which primary rays use the packet walk (measured: DESIGN.md s5)
constexpr int RING = 64;         // HIP-event triples kept for per-kernel timing between two srt_sync calls

// ---- owners: whatever a handle or the records allocate is freed by the destructor of one of these, with the device already current ----
// Device (or pinned host) memory of `cap` units of K elements each; reads as a plain T* wherever one is expected.  Grow-only: reserve frees
// first and allocates second, so the peak is the larger block alone, and a failed allocation leaves p null and cap 0 for the next call to
// try again.  The owner knows nothing of enqueued work: whoever grows a buffer that a render may still read waits first (grow, stage_acquire).
template <typename T, size_t K, bool PINNED>
struct Buf {
    T* p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete; Buf& operator=(const Buf&) = delete;
    ~Buf() { release(); }
    operator T*() const { return p; }
    void release() { if (p) { if (PINNED) (void)hipHostFree(p); else (void)hipFree(p); } p = nullptr; cap = 0; }
    hipError_t reserve(size_t n) {
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p, n * K * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, n * K * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
};
template <typename T, size_t K = 1> using DevArray = Buf<T, K, false>;
template <typename T, size_t K = 1> using Pinned = Buf<T, K, true>;

struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete; Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct EventRing {                   // per render: start, closest-hit done, shadow done, shade done; a slot's events are made on first use
    hipEvent_t ev[RING][4] = {};
    EventRing() = default;
    EventRing(const EventRing&) = delete; EventRing& operator=(const EventRing&) = delete;
    ~EventRing() { for (auto& slot : ev) for (hipEvent_t e : slot) if (e) (void)hipEventDestroy(e); }
    hipEvent_t* operator[](size_t i) { return ev[i]; }
};
struct Stream {
    hipStream_t st = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete; Stream& operator=(const Stream&) = delete;
    ~Stream() { if (st) (void)hipStreamDestroy(st); }
    operator hipStream_t() const { return st; }
};

struct Boxes;

// The device records of a scene: owned by the handle that uploaded them and by every handle made from it with srt_scene_share.
struct SceneRecords {
    int device = 0;
    std::deque<DevArray<char>> owned;        // every array below and every array of DevScene: made once, freed with the last handle
    std::vector<uint64_t> tex_off; std::vector<uint32_t> tex_w, tex_h;      // the uploaded texture table (host copy) ...
    uint64_t tex_bytes = 0, tex_hash = 0;                                    // ... and the size and content hash of the uploaded images
    double overlap = 0.;             // expected slab tests per ray (surface-area estimate, see overlap_estimate)
    bool prefer_packet = false;      // hierarchy of heavily overlapping boxes: primary rays take the packet walk too
    bool int_shin = false;           // every object's shininess is an integer in [1, 64]: the shading kernel without the general pow
    // host copies of the static topology (srt_scene_update_frame checks counts against them and re-estimates the overlap from a frame's boxes)
    std::vector<int2> h_ranges; std::vector<int32_t> h_tri_first, h_leaf;
    // host copy of the objects' root boxes (n_objects x 3 each): what a frame's tile spans are computed from (srt_tile_spans.h).  Valid after
    // an upload from the host (create, update, update_frame); a pose or a refit changes the boxes on the device only and makes it invalid
    // -- no culling -- until the next upload.  Part of the records: every handle of srt_scene_share sees the one truth.
    std::vector<float> h_root_min, h_root_max; bool root_boxes_valid = false;
    // The box epoch: a number that every upload, pose and refit of these records raises, and the same number in a word of device memory,
    // written in stream order by the call that changes the boxes.  A frame's tile spans carry the epoch they were made at; a launch
    // captured into a graph compares it with the word at every replay (srt_kernels.h, trace_nq_body) and culls nothing once they differ.
    uint32_t box_epoch = 1; uint32_t* d_box_epoch = nullptr;
    // One of those calls was CAPTURED into a graph: its replays change the boxes on the device with no host code running, so the host
    // copy can be stale at any time from then on, whatever is uploaded later.  Sticky: these records never get tile spans again.
    bool boxes_change_in_replays = false;
    void note_root_boxes(const struct Boxes& box, const int2* ranges, uint32_t n_objects);
    // f1, device half: node -> DevWide index (static), this frame's inputs, the per-triangle attributes in source order
    int32_t* d_widx = nullptr; float4* d_src_points = nullptr; uint32_t* d_order = nullptr; float* d_box_min = nullptr; float* d_box_max = nullptr;
    float* d_src_tc = nullptr; float* d_src_nrm = nullptr; int32_t* d_src_tex = nullptr; bool have_source = false;
    // pose (srt_scene_pose): the points the poses are applied to (visit order), each triangle's own box, this frame's matrices, and the
    // static schedule of the refit -- node heights, the roots of the bottom subtrees, per object the nodes above them sorted by height
    float4* d_pose_points = nullptr; float2* d_tri_box = nullptr; float* d_obj_matrix = nullptr; uint8_t* d_height = nullptr;
    int32_t* d_sub_root = nullptr; int32_t* d_top_nodes = nullptr; int32_t* d_top_off = nullptr; uint32_t n_sub = 0; bool have_pose = false;
    // refit from device points (srt_scene_refit_device): the same schedule, and the index buffer of the indexed form (visit order)
    uint32_t* d_tri_vertex = nullptr; uint32_t refit_verts = 0; bool have_refit = false, have_refit_index = false;
    // visibility masks (srt_scene_set_object_masks): one word an object, made by the first call; null reads as all ones
    uint32_t* d_obj_mask = nullptr;
    ~SceneRecords() { (void)hipSetDevice(device); }      // (the arrays go with `owned`, after this body)
    hipError_t make(void** out, size_t bytes) {
        owned.emplace_back();
        const hipError_t e = owned.back().reserve(bytes ? bytes : 1);
        if (e == hipSuccess) *out = owned.back().p; else owned.pop_back();
        return e;
    }
};

struct srt_scene {
    int device = 0;
    DevScene dev{};
    std::shared_ptr<SceneRecords> rec;
    uint64_t bytes = 0;
    // workspace; capacities count pixels, light samples, words or bytes (K of the owner = elements per unit)
    DevArray<int32_t> ws_hit; DevArray<float> ws_t;
    DevArray<float, 3> ws_lin; DevArray<uint8_t, 3> ws_rgb8;
    DevArray<float, 3> d_lights; Pinned<float, 3> h_lights; uint32_t lights_valid = 0;
    DevArray<unsigned long long> d_counters; Pinned<unsigned long long> h_counters;       // device: two sets used alternately
    unsigned long long* d_ctr_last = nullptr;     // set written by the most recent render
    uint64_t render_seq = 0;
    bool ctr_dirty = false;                       // a render returned an error after its first launch
    char pipeline[96] = "";                       // kernels of the last render, in launch order
    uint32_t n_textures = 0; bool has_tex = false;
    Pinned<char> stage; Event staged;             // pinned staging of srt_scene_update / _update_frame / _pose (stage_acquire)
    Stream stream;                                // the scene's own stream (srt_render, srt_render_async, srt_scene_update with stream NULL)
    DevArray<unsigned long long> ws_shadow;
    DevArray<uint32_t, 3> ws_qlist; DevArray<uint32_t> d_qcount; uint32_t qcap = 0;      // quadrants with hits: 64 shard lists of qcap entries, their counters
    DevArray<float, 3> ws_acc, ws_sub; DevArray<int32_t> ws_sub_hit; DevArray<float> ws_sub_t;
    // ray queries, the host entry points: the device memory of ONE call -- what it brings and what it wants, cut afresh by every
    // query_round_trip (capacity counts bytes).  One block is enough: a host form runs on the scene's own stream and synchronises before it
    // returns, so no call finds another's arrays in use, and no _device entry point reads it.
    DevArray<char> query_block;
    // the counter set private to queries (laid out like a render's), which no render reads, zeroes or reports
    DevArray<unsigned long long> d_qctr;
    // srt_shade_rays: the query's own light table (a render's d_lights may be in use on another stream): the pinned copy, the event behind
    // its last upload, the stream that upload went to, and whether it is known to have arrived
    DevArray<float, 3> d_qlights; Pinned<float, 3> h_qlights; uint32_t qlights_valid = 0;
    Event qlights_sent; hipStream_t qlights_stream = nullptr; bool qlights_settled = true;
    int n_cu = 256;
    EventRing ev;
    uint32_t ring_count = 0;         // renders since the last srt_sync
    hipEvent_t last_done = nullptr;  // ev[..][2] of the most recent render
    hipStream_t last_stream = nullptr;
    bool pending = false;
    srt_stats last{};
};

// Wait for the work of earlier renders before their buffers are reused or freed.
static hipError_t wait_idle(srt_scene* s) {
    if (!s->pending) return hipSuccess;
    return s->last_done ? hipEventSynchronize(s->last_done) : hipStreamSynchronize(s->last_stream);
}

// Workspace that shares a capacity, to n units each: nothing when all of it is that large, else wait for the renders that may still use
// it, free all of it, then allocate all of it.  A failure leaves some of it empty, and the next call starts over.
template <typename... B>
static int grow(srt_scene* s, size_t n, B&... bufs) {
    if (((bufs.cap >= n) && ...)) return SRT_OK;
    HIP_TRY(wait_idle(s));
    (bufs.release(), ...);
    hipError_t e = hipSuccess;
    ((e = e == hipSuccess ? bufs.reserve(n) : e), ...);
    HIP_TRY(e);
    return SRT_OK;
}

// An array of the records that is made on first use (the sources of update_frame and pose): `bytes` of device memory, then src_bytes from src.
template <typename T>
static int lazy_array(srt_scene* s, T** dst, size_t bytes, const void* src = nullptr, size_t src_bytes = 0) {
    if (!*dst) { HIP_TRY(s->rec->make((void**)dst, bytes)); s->bytes += bytes; }
    if (src && src_bytes) HIP_TRY(hipMemcpy(*dst, src, src_bytes, hipMemcpyHostToDevice));
    return SRT_OK;
}

extern "C" {

uint32_t srt_abi_version(void) { return SRT_ABI_VERSION; }
int srt_last_hip_error(void) { return g_last_hip; }

const char* srt_strerror(int code) {
    switch (code) {
    case SRT_OK: return "ok";
    case SRT_ERR_ARG: return "invalid argument";
    case SRT_ERR_LAYOUT: return "scene arrays violate the layout contract of include/srt.h";
    case SRT_ERR_DEVICE: return "HIP runtime error (see srt_last_hip_error)";
    case SRT_ERR_NO_GPU: return "no HIP device: this library has no CPU fallback";
    case SRT_ERR_TEXTURE: return "triangle references a texture that does not exist";
    case SRT_ERR_LIMIT: return "size exceeds an implementation limit";
    case SRT_ERR_OOM: return "out of host memory";
    default: return "unknown error";
    }
}

void srt_params_default(srt_params* p, uint32_t width, uint32_t height) {
    std::memset(p, 0, sizeof(*p));
    p->width = width; p->height = height;
    p->block_rows = height; p->block_first = 0; p->block_stride = 1; p->block_cols = 0;
    p->focal = 400.0f;                 // simple_raytracer.cpp:506
    p->n_lights = 1;                   // :445
    p->light_pos = nullptr;
    p->ray_matrix = nullptr;           // the reference's frame: scene in camera space, rays from the origin
    p->shadow_div = 5.0f;              // :369
    p->reinhard = 0.5f;                // :391
    p->gamma = 1.1f;                   // :396
    p->background[0] = 173; p->background[1] = 216; p->background[2] = 230;   // :476
    p->spp = 1; p->flags = 0;
}

void srt_light_staircase(const float base[3], uint32_t n, float* out) {
    float L[3] = { base[0], base[1], base[2] };          // softShadow:363
    for (uint32_t i = 0; i < n; i++) {
        out[i * 3] = L[0]; out[i * 3 + 1] = L[1]; out[i * 3 + 2] = L[2];
        L[i % 3] += 3.0f;                                 // :372-382
    }
}

uint32_t srt_cols_owned(const srt_params* p) {
    if (!p || !p->block_stride) return 0;
    if (!p->block_cols) return p->width;
    const uint32_t n_bx = (p->width + p->block_cols - 1) / p->block_cols;
    return (n_bx + p->block_stride - 1) / p->block_stride * p->block_cols;      // padded: every block row has the same local width
}

// pixels of the image a call with these params renders (padding of a tile deal excluded)
static uint64_t pixels_owned(const srt_params* p) {
    if (!p->block_cols) return (uint64_t)p->width * srt_rows_owned(p);
    const uint32_t n_bx = (p->width + p->block_cols - 1) / p->block_cols, n_by = (p->height + p->block_rows - 1) / p->block_rows;
    uint64_t n = 0;
    for (uint32_t by = 0; by < n_by; by++) {
        const uint32_t h = (by + 1) * p->block_rows <= p->height ? p->block_rows : p->height - by * p->block_rows;
        for (uint32_t bx = (p->block_first + p->block_stride - by % p->block_stride) % p->block_stride; bx < n_bx; bx += p->block_stride) {
            const uint32_t w = (bx + 1) * p->block_cols <= p->width ? p->block_cols : p->width - bx * p->block_cols;
            n += (uint64_t)w * h;
        }
    }
    return n;
}

uint32_t srt_rows_owned(const srt_params* p) {
    if (!p || !p->block_rows || !p->block_stride) return 0;
    if (p->block_cols) return p->block_first < p->block_stride ? p->height : 0;      // tiles dealt in two dimensions: tiles in every row
    const uint32_t nblocks = (p->height + p->block_rows - 1) / p->block_rows;
    uint32_t rows = 0;
    for (uint32_t b = p->block_first; b < nblocks; b += p->block_stride) {
        const uint32_t y0 = b * p->block_rows;
        uint32_t y1 = y0 + p->block_rows;
        if (y1 > p->height) y1 = p->height;
        rows += y1 - y0;
    }
    return rows;
}

int srt_scene_destroy(srt_scene* s) {
    if (!s) return SRT_ERR_ARG;
    (void)hipSetDevice(s->device);
    (void)wait_idle(s);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;                            // the owners free what the handle holds; the records go with their last handle
    return SRT_OK;
}

// Validate the layout contract and rewrite the trees in DFS pre-order with skip links: nodes[n_nodes], ranges[n_objects].
static int build_device_records(const srt_scene_desc* d, DevNode* nodes, int2* ranges) {
    const uint32_t N = d->n_nodes;
    std::vector<uint8_t> seen(N, 0);
    int64_t tri_cursor = 0;
    uint32_t cursor = 0;                   // nodes emitted so far
    // explicit DFS stack: state 0 = emit node, 1 = left subtree done, 2 = right subtree done
    struct Item { int32_t orig; int32_t emitted; int state; };
    std::vector<Item> st;
    for (uint32_t k = 0; k < d->n_objects; k++) {
        const uint32_t root = d->obj_root[k];
        if (root >= N) return SRT_ERR_LAYOUT;
        ranges[k].x = (int32_t)cursor;
        st.clear(); st.push_back({ (int32_t)root, -1, 0 });
        while (!st.empty()) {
            Item& it = st.back();        // not used after a push_back below
            if (it.state == 0) {
                if (it.orig < 0 || (uint32_t)it.orig >= N || seen[it.orig] || cursor >= N) return SRT_ERR_LAYOUT;
                seen[it.orig] = 1;
                const int32_t l = d->node_left[it.orig], r = d->node_right[it.orig];
                DevNode dn;
                dn.minx = d->node_min[3 * (size_t)it.orig]; dn.miny = d->node_min[3 * (size_t)it.orig + 1]; dn.minz = d->node_min[3 * (size_t)it.orig + 2];
                dn.maxx = d->node_max[3 * (size_t)it.orig]; dn.maxy = d->node_max[3 * (size_t)it.orig + 1]; dn.maxz = d->node_max[3 * (size_t)it.orig + 2];
                dn.skip = -1; dn.leaf = -1;
                it.emitted = (int32_t)cursor;
                if (l < 0 && r < 0) {
                    const int32_t first = d->node_first[it.orig], cnt = d->node_count[it.orig];
                    if (cnt < 0 || (cnt > 0 && first != tri_cursor) || tri_cursor + cnt > (int64_t)d->n_tris) return SRT_ERR_LAYOUT;
                    if (cnt > LEAF_MAX) return SRT_ERR_LIMIT;
                    for (int32_t j = 0; j < cnt; j++) if (d->tri_obj[tri_cursor + j] != (int32_t)k) return SRT_ERR_LAYOUT;
                    dn.leaf = (int32_t)((tri_cursor << LEAF_SHIFT) | cnt);
                    tri_cursor += cnt;
                    dn.skip = it.emitted + 1;
                    nodes[cursor++] = dn;
                    st.pop_back();
                } else {
                    if (l < 0 || r < 0) return SRT_ERR_LAYOUT;      // the reference's trees are full binary
                    nodes[cursor++] = dn;
                    it.state = 1;
                    st.push_back({ l, -1, 0 });
                }
            } else if (it.state == 1) {
                it.state = 2;
                const int32_t r = d->node_right[it.orig];
                nodes[it.emitted].leaf = ~(int32_t)cursor;           // inner node: ~(pre-order index of the right child) < 0
                st.push_back({ r, -1, 0 });
            } else {
                nodes[it.emitted].skip = (int32_t)cursor;
                st.pop_back();
            }
        }
        ranges[k].y = (int32_t)cursor;
    }
    if (cursor != N || tri_cursor != (int64_t)d->n_tris) return SRT_ERR_LAYOUT;
    return SRT_OK;
}

// The inner nodes as the node-queue kernels read them (DevWide, srt_device.h): both children's boxes in the parent's record, records
// numbered in pre-order over the inner nodes.  wide[n_wide], root_info[n_objects]; n_wide = (n_nodes - n_objects) / 2 for full binary
// trees, which build_device_records has checked.  widx is scratch (n_nodes words).
static uint32_t wide_count(uint32_t n_nodes, uint32_t n_objects) { return (n_nodes - n_objects) / 2; }
static void build_wide_records(const DevNode* nodes, uint32_t n_nodes, const int2* ranges, uint32_t n_objects, DevWide* wide, int32_t* root_info, int32_t* widx) {
    int32_t w = 0;
    for (uint32_t i = 0; i < n_nodes; i++) widx[i] = nodes[i].leaf < 0 ? w++ : -1;
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (nodes[i].leaf >= 0) continue;
        const DevNode& l = nodes[i + 1];
        const int32_t ri = ~nodes[i].leaf;
        const DevNode& r = nodes[ri];
        DevWide& q = wide[widx[i]];
        q.lminx = l.minx; q.lminy = l.miny; q.lminz = l.minz; q.lmaxx = l.maxx; q.lmaxy = l.maxy; q.lmaxz = l.maxz;
        q.rminx = r.minx; q.rminy = r.miny; q.rminz = r.minz; q.rmaxx = r.maxx; q.rmaxy = r.maxy; q.rmaxz = r.maxz;
        q.linfo = l.leaf >= 0 ? l.leaf : ~widx[i + 1];
        q.rinfo = r.leaf >= 0 ? r.leaf : ~widx[ri];
        q.node = (int32_t)i; q.rnode = ri;
    }
    for (uint32_t k = 0; k < n_objects; k++) {
        const int32_t root = ranges[k].x;
        root_info[k] = nodes[root].leaf >= 0 ? nodes[root].leaf : ~widx[root];
    }
}

// Boxes by node index, from either form the host has them in: the records, or the min / max arrays of a frame (srt_frame_geometry).
struct Boxes {
    const DevNode* nodes; const float* bmin; const float* bmax;
    explicit Boxes(const DevNode* nodes_) : nodes(nodes_), bmin(nullptr), bmax(nullptr) {}
    Boxes(const float* bmin_, const float* bmax_) : nodes(nullptr), bmin(bmin_), bmax(bmax_) {}
    void operator()(size_t i, float* mn, float* mx) const {
        if (nodes) { const DevNode& n = nodes[i]; mn[0] = n.minx; mn[1] = n.miny; mn[2] = n.minz; mx[0] = n.maxx; mx[1] = n.maxy; mx[2] = n.maxz; }
        else for (int a = 0; a < 3; a++) { mn[a] = bmin[3 * i + a]; mx[a] = bmax[3 * i + a]; }
    }
};

void SceneRecords::note_root_boxes(const Boxes& box, const int2* ranges, uint32_t n_objects) {
    root_boxes_valid = false;
    h_root_min.resize(3 * (size_t)n_objects); h_root_max.resize(3 * (size_t)n_objects);
    for (uint32_t k = 0; k < n_objects; k++) box((size_t)ranges[k].x, h_root_min.data() + 3 * k, h_root_max.data() + 3 * k);
    root_boxes_valid = true;
}

// the union of the objects' root boxes, in a node's box layout (min.xyz max.x | max.yz 0 0): what a tile's rays are tested against
// before the roots themselves in scenes of several objects (srt_kernels.h background_test_wave)
static void union_of_roots(const Boxes& box, const int2* ranges, uint32_t n_objects, float* out8) {
    float lo[3] = { FLT_MAX, FLT_MAX, FLT_MAX }, hi[3] = { -FLT_MAX, -FLT_MAX, -FLT_MAX };
    for (uint32_t k = 0; k < n_objects; k++) {
        float mn[3], mx[3];
        box((size_t)ranges[k].x, mn, mx);
        for (int a = 0; a < 3; a++) { if (mn[a] < lo[a]) lo[a] = mn[a]; if (mx[a] > hi[a]) hi[a] = mx[a]; }
    }
    out8[0] = lo[0]; out8[1] = lo[1]; out8[2] = lo[2]; out8[3] = hi[0]; out8[4] = hi[1]; out8[5] = hi[2]; out8[6] = 0.f; out8[7] = 0.f;
}

// 64-bit content hash of a byte range (texture images: srt_scene_update re-uploads them only when it changes).  Eight independent
// multiply-xor lanes over 64-byte blocks: memory-bound on one core.
static uint64_t content_hash(const uint8_t* p, size_t n) {
    uint64_t h[8];
    for (int k = 0; k < 8; k++) h[k] = 0x9e3779b97f4a7c15ull * (uint64_t)(k + 1) ^ (uint64_t)n;
    size_t i = 0;
    for (; i + 64 <= n; i += 64) {
        uint64_t w[8];
        std::memcpy(w, p + i, 64);
        for (int k = 0; k < 8; k++) { h[k] = (h[k] ^ w[k]) * 0xff51afd7ed558ccdull; h[k] ^= h[k] >> 29; }
    }
    uint64_t tail[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    if (i < n) { std::memcpy(tail, p + i, n - i); for (int k = 0; k < 8; k++) { h[k] = (h[k] ^ tail[k]) * 0xff51afd7ed558ccdull; h[k] ^= h[k] >> 29; } }
    uint64_t r = 0xc4ceb9fe1a85ec53ull;
    for (int k = 0; k < 8; k++) { r = (r ^ h[k]) * 0xff51afd7ed558ccdull; r ^= r >> 32; }
    return r;
}

// How many slab tests does a ray cost?  Surface-area estimate: a random line that crosses the scene's bounds crosses a convex
// box inside them with probability area(box) / area(bounds), and a node is tested when its parent's box is crossed.  A good
// hierarchy gives a few dozen (bunny: boxes shrink with depth); a median split by first vertex of a random soup gives hundreds
// to thousands (boxes stay as wide as the scene in two axes).  In the second case neighbouring rays test nearly the same nodes
// and the packet walk (srt_packet.h) wins for primary rays as well.
// leaf[i] < 0: node i is an inner node (DevNode::leaf, SceneRecords::h_leaf).  The sum runs over the inner nodes in index order.
static double overlap_estimate(const Boxes& box, const int32_t* leaf, uint32_t n_nodes, const int2* ranges, uint32_t n_objects) {
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    auto area = [](const float* a, const float* b) -> double {
        const double x = (double)b[0] - a[0], y = (double)b[1] - a[1], z = (double)b[2] - a[2];
        return (x < 0 || y < 0 || z < 0) ? 0. : x * y + y * z + z * x;
    };
    float mn[3], mx[3];
    for (uint32_t k = 0; k < n_objects; k++) {
        box((size_t)ranges[k].x, mn, mx);
        if (area(mn, mx) <= 0.) continue;
        for (int a = 0; a < 3; a++) { lo[a] = mn[a] < lo[a] ? mn[a] : lo[a]; hi[a] = mx[a] > hi[a] ? mx[a] : hi[a]; }
    }
    const double total = area(lo, hi);
    if (!(total > 0.)) return 0.;
    double sum = 0.;
    for (uint32_t i = 0; i < n_nodes; i++) {
        if (leaf[i] >= 0) continue;                      // the children of an inner node are tested when its box is crossed
        box(i, mn, mx);
        sum += 2. * area(mn, mx);
    }
    return (double)n_objects + sum / total;              // + every root
}

// per-triangle records: independent, so big scenes are cut over a few host threads (a scene made per frame by a drop-in
// caller spends more time here than in the render)
static void derive_triangles(const srt_scene_desc* d, DevTri* tris, DevTriO* tris_o) {
    auto derive_range = [&](uint32_t b, uint32_t e) {
        for (uint32_t i = b; i < e; i++) { tris[i] = derive_triangle(d->tri_points + 12 * (size_t)i); tris_o[i] = derive_triangle_origin(tris[i]); }
    };
    const uint32_t n = d->n_tris;
    unsigned hc = std::thread::hardware_concurrency();
    const uint32_t T = n < 32768 ? 1u : (hc >= 8 ? 8u : (hc >= 2 ? hc : 1u));
    if (T == 1) { derive_range(0, n); return; }
    // a thread that cannot be started (std::system_error) must not take the process down with joinable threads in a dying vector:
    // the ranges that got no thread are derived inline, and every started thread is joined
    std::vector<std::thread> th;
    th.reserve(T);
    const uint32_t step = (n + T - 1) / T;
    uint32_t started = 1;                                  // ranges [1, started) have a thread
    try {
        for (; started < T; started++) th.emplace_back(derive_range, started * step < n ? started * step : n, (started + 1) * step < n ? (started + 1) * step : n);
    } catch (...) { }
    derive_range(0, step < n ? step : n);
    for (uint32_t k = started; k < T; k++) derive_range(k * step < n ? k * step : n, (k + 1) * step < n ? (k + 1) * step : n);
    for (std::thread& t : th) t.join();
}

// first triangle of each object (the layout contract makes tri_obj non-decreasing): first[n_objects + 1]
static void derive_tri_first(const srt_scene_desc* d, int32_t* first) {
    for (uint32_t k = 0; k <= d->n_objects; k++) first[k] = (int32_t)d->n_tris;
    for (uint32_t i = d->n_tris; i-- > 0;) first[d->tri_obj[i]] = (int32_t)i;
    for (uint32_t k = d->n_objects; k-- > 0;) if (first[k] > first[k + 1]) first[k] = first[k + 1];      // objects without triangles
}

static bool all_integer_shininess(const float* obj_material, uint32_t n_objects) {
    for (uint32_t k = 0; k < n_objects; k++) {
        const float sh = obj_material[3 * (size_t)k + 2];
        if (!(sh >= 1.0f && sh <= 64.0f && sh == std::trunc(sh))) return false;
    }
    return true;
}

static int check_desc(const srt_scene_desc* d) {
    if (!d->n_objects || !d->n_nodes || !d->node_min || !d->node_max || !d->node_left || !d->node_right ||
        !d->node_first || !d->node_count || !d->obj_root || !d->obj_color || !d->obj_material) return SRT_ERR_ARG;
    if (d->n_tris && (!d->tri_points || !d->tri_obj)) return SRT_ERR_ARG;
    // queue entries of the node-queue kernels pack (node << 6 | ray lane) into 32 bits; a leaf word packs (first << 5 | count)
    static_assert(NODE_INDEX_BITS + 6 == 32, "node-queue entry = node index + 6-bit lane");
    if (d->n_tris >= (1u << (31 - LEAF_SHIFT)) || d->n_nodes >= (1u << NODE_INDEX_BITS)) return SRT_ERR_LIMIT;
    if (d->n_textures && (!d->tex_rgb || !d->tex_off || !d->tex_w || !d->tex_h || !d->tri_tex || !d->tri_texcoord)) return SRT_ERR_ARG;
    for (uint32_t i = 0; i < d->n_tris; i++) {
        if (d->tri_obj[i] < 0 || (uint32_t)d->tri_obj[i] >= d->n_objects) return SRT_ERR_LAYOUT;
        if (d->tri_tex && d->tri_tex[i] >= (int32_t)d->n_textures) return SRT_ERR_TEXTURE;
    }
    return SRT_OK;
}

static bool any_textured(const srt_scene_desc* d) {
    bool any_tex = false;
    if (d->n_textures && d->tri_tex) for (uint32_t i = 0; i < d->n_tris; i++) any_tex |= d->tri_tex[i] >= 0;
    return any_tex;
}

// What every handle has of its own besides the records: the two counter sets, the quadrant-list counters, the pinned counter image.
static hipError_t init_handle_state(srt_scene* s) {
    hipError_t e = s->d_counters.reserve(2 * NCTR);
    if (e == hipSuccess) e = hipMemset(s->d_counters, 0, 2 * NCTR * sizeof(unsigned long long));
    if (e == hipSuccess) e = s->d_qcount.reserve(QL_COUNTERS * QL_STRIDE);
    if (e == hipSuccess) e = hipMemset(s->d_qcount, 0, QL_COUNTERS * QL_STRIDE * sizeof(uint32_t));
    if (e == hipSuccess) e = s->h_counters.reserve(NCTR);
    if (e == hipSuccess) e = s->d_qctr.reserve(NCTR);
    if (e == hipSuccess) e = hipMemset(s->d_qctr, 0, NCTR * sizeof(unsigned long long));
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, s->device);
    if (e == hipSuccess && prop.multiProcessorCount > 0) s->n_cu = prop.multiProcessorCount;
    return e;
}

// ---- the record arrays of a scene, stated once -----------------------------------------------------------------------------------
// One row per array that srt_scene_create allocates and fills and srt_scene_update fills again, numbered in the order of the device
// allocations.  elem x n is the array's size (an array of no elements still gets an allocation of one); elem = 0: not in this scene, or
// not in this call.  src: the caller's array when it goes to the device as it is, null when derive_records writes it.  off: its place in
// the host block the rows are derived and staged in.  A new array is a new row here (and its derivation, if it has one).
enum RecordId { R_NODES, R_WIDE, R_ROOT_INFO, R_ROOTS, R_SCENE_BOX, R_TRIS, R_TRIS_O, R_TRI_OBJ, R_RANGES, R_TRI_FIRST, R_COLOR, R_MAT, R_NORMALS,
                R_TRI_TEX, R_TRI_TC, R_TEX, R_TEX_OFF, R_TEX_SIZE, R_TEX_W, R_TEX_H, R_WIDX, R_COUNT };
struct RecordArray { void** dev; size_t elem, n; const void* src; size_t off; size_t bytes() const { return elem * n; } };
using RecordList = std::array<RecordArray, R_COUNT>;

// tex_bytes: the texture images' size when they are to be uploaded, else 0; tex_table: offsets and sizes too (they never change after
// srt_scene_create).  stage_sources: the host block has room for the caller's arrays as well (pinned staging), not only for the derived ones.
static RecordList record_list(DevScene& v, SceneRecords& r, const srt_scene_desc* d, bool any_tex, size_t tex_bytes, bool tex_table, bool stage_sources, size_t* host_bytes) {
    const size_t nN = d->n_nodes, nT = d->n_tris, nO = d->n_objects, nX = d->n_textures;
    const size_t nrm = d->tri_normals && nT ? 1 : 0, tex = any_tex ? 1 : 0, img = tex_bytes ? 1 : 0, tab = any_tex && tex_table ? 1 : 0;
    RecordList l{};
    #define ROW(id, ptr, elem, n, src) l[id] = RecordArray{ (void**)&(ptr), (elem), (n), (src), 0 }
    ROW(R_NODES, v.nodes, sizeof(DevNode), nN, nullptr);
    ROW(R_WIDE, v.wide, sizeof(DevWide), wide_count(d->n_nodes, d->n_objects), nullptr);
    ROW(R_ROOT_INFO, v.obj_root_info, 4, nO, nullptr);
    ROW(R_ROOTS, v.root_nodes, sizeof(DevNode), nO, nullptr);
    ROW(R_SCENE_BOX, v.scene_box, 4, 8, nullptr);
    ROW(R_TRIS, v.tris, sizeof(DevTri), nT, nullptr);
    ROW(R_TRIS_O, v.tris_o, sizeof(DevTriO), nT, nullptr);
    ROW(R_TRI_OBJ, v.tri_obj, 4, nT, d->tri_obj);
    ROW(R_RANGES, v.obj_range, sizeof(int2), nO, nullptr);
    ROW(R_TRI_FIRST, v.obj_tri_first, 4, nO + 1, nullptr);
    ROW(R_COLOR, v.obj_color, 4, nO * 3, d->obj_color);
    ROW(R_MAT, v.obj_mat, 4, nO * 3, d->obj_material);
    ROW(R_NORMALS, v.tri_normals, nrm * 4, nT * 9, d->tri_normals);
    ROW(R_TRI_TEX, v.tri_tex, tex * 4, nT, d->tri_tex);
    ROW(R_TRI_TC, v.tri_tc, tex * 4, nT * 6, d->tri_texcoord);
    ROW(R_TEX, v.tex, img, tex_bytes, d->tex_rgb);
    ROW(R_TEX_OFF, v.tex_off, tab * 8, nX, nullptr);
    ROW(R_TEX_SIZE, v.tex_size, tab * 8, nX, nullptr);
    ROW(R_TEX_W, v.tex_w, tab * 4, nX, d->tex_w);
    ROW(R_TEX_H, v.tex_h, tab * 4, nX, d->tex_h);
    ROW(R_WIDX, r.d_widx, 4, nN, nullptr);
    #undef ROW
    size_t off = 0;
    for (RecordArray& a : l) { a.off = off; if (a.elem && (stage_sources || !a.src)) off += (a.bytes() + 255) & ~(size_t)255; }
    *host_bytes = off;
    return l;
}

// Every row without a source, derived into its place in the host block h -- a vector when a scene is created, the pinned staging
// block when it is updated.  Validates the layout contract on the way (build_device_records).
static int derive_records(const srt_scene_desc* d, const RecordList& l, char* h) {
    DevNode* nodes = (DevNode*)(h + l[R_NODES].off); int2* ranges = (int2*)(h + l[R_RANGES].off); DevNode* roots = (DevNode*)(h + l[R_ROOTS].off);
    SRT_TRY(build_device_records(d, nodes, ranges));
    build_wide_records(nodes, d->n_nodes, ranges, d->n_objects, (DevWide*)(h + l[R_WIDE].off), (int32_t*)(h + l[R_ROOT_INFO].off), (int32_t*)(h + l[R_WIDX].off));
    for (uint32_t k = 0; k < d->n_objects; k++) roots[k] = nodes[ranges[k].x];
    union_of_roots(Boxes(nodes), ranges, d->n_objects, (float*)(h + l[R_SCENE_BOX].off));
    derive_triangles(d, (DevTri*)(h + l[R_TRIS].off), (DevTriO*)(h + l[R_TRIS_O].off));
    derive_tri_first(d, (int32_t*)(h + l[R_TRI_FIRST].off));
    if (l[R_TEX_OFF].elem) {
        unsigned long long* off = (unsigned long long*)(h + l[R_TEX_OFF].off); unsigned long long* size = (unsigned long long*)(h + l[R_TEX_SIZE].off);
        for (uint32_t k = 0; k < d->n_textures; k++) { off[k] = d->tex_off[k]; size[k] = (unsigned long long)d->tex_w[k] * d->tex_h[k] * 3; }
    }
    return SRT_OK;
}

// What the host keeps of the records in h: the estimates that steer the pipeline, and the topology srt_scene_update_frame and
// srt_scene_set_pose_source rely on (after an update it may differ from the previous contents': same counts, other trees).
static void note_records(SceneRecords& r, const srt_scene_desc* d, const RecordList& l, const char* h) {
    const DevNode* nodes = (const DevNode*)(h + l[R_NODES].off); const int2* ranges = (const int2*)(h + l[R_RANGES].off);
    const int32_t* first = (const int32_t*)(h + l[R_TRI_FIRST].off);
    r.h_ranges.assign(ranges, ranges + d->n_objects);
    r.h_tri_first.assign(first, first + d->n_objects + 1);
    r.h_leaf.resize(d->n_nodes); for (uint32_t i = 0; i < d->n_nodes; i++) r.h_leaf[i] = nodes[i].leaf;
    r.overlap = overlap_estimate(Boxes(nodes), r.h_leaf.data(), d->n_nodes, ranges, d->n_objects);
    r.prefer_packet = r.overlap > PACKET_OVERLAP_THRESHOLD;
    r.int_shin = all_integer_shininess(d->obj_material, d->n_objects);
    r.note_root_boxes(Boxes(nodes), ranges, d->n_objects);
    r.have_source = false;               // attributes in source order belong to the previous contents
    r.have_pose = false;                 // ... and so do the pose source's order and the refit's schedule
    r.have_refit = r.have_refit_index = false;
}

static int scene_create_impl(int device, const srt_scene_desc* d, srt_scene** out) {
    if (!d || !out) return SRT_ERR_ARG;
    *out = nullptr;
    SRT_TRY(check_desc(d));
    const bool any_tex = any_textured(d);
    unsigned long long tex_total = 0;
    bool tex_empty = false;
    if (any_tex) for (uint32_t k = 0; k < d->n_textures; k++) {
        const unsigned long long size = (unsigned long long)d->tex_w[k] * d->tex_h[k] * 3;
        tex_empty |= size < 3;
        if (d->tex_off[k] + size > tex_total) tex_total = d->tex_off[k] + size;
    }
    // host-side records first (validates the layout contract; pure CPU work), then the device
    alloc_gate();
    std::unique_ptr<srt_scene> s(new srt_scene());       // (a failed create has enqueued nothing: the owners free what it got so far)
    s->rec = std::make_shared<SceneRecords>();
    SceneRecords& r = *s->rec;
    size_t host_bytes = 0;
    const RecordList l = record_list(s->dev, r, d, any_tex, (size_t)tex_total, true, false, &host_bytes);
    std::vector<char> host(host_bytes);
    SRT_TRY(derive_records(d, l, host.data()));
    note_records(r, d, l, host.data());

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SRT_ERR_NO_GPU;
    if (device < 0 || device >= ndev) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    if (tex_empty) return SRT_ERR_TEXTURE;
    s->device = device; r.device = device;
    for (const RecordArray& a : l) {     // one allocation per array, in the list's order
        if (!a.elem) continue;
        const size_t cap = a.elem * (a.n ? a.n : 1);
        HIP_TRY(r.make(a.dev, cap));
        s->bytes += cap;
        if (a.n) HIP_TRY(hipMemcpy(*a.dev, a.src ? a.src : host.data() + a.off, a.bytes(), hipMemcpyHostToDevice));
    }
    if (any_tex) {
        r.tex_off.assign(d->tex_off, d->tex_off + d->n_textures);
        r.tex_w.assign(d->tex_w, d->tex_w + d->n_textures); r.tex_h.assign(d->tex_h, d->tex_h + d->n_textures);
        r.tex_bytes = tex_total; r.tex_hash = content_hash(d->tex_rgb, (size_t)tex_total);
    }
    s->dev.n_nodes = d->n_nodes; s->dev.n_tris = d->n_tris; s->dev.n_objects = d->n_objects;
    s->n_textures = d->n_textures; s->has_tex = any_tex;
    HIP_TRY(r.make((void**)&r.d_box_epoch, sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(r.d_box_epoch, &r.box_epoch, sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(init_handle_state(s.get()));
    *out = s.release();
    return SRT_OK;
}

// A second handle on the SAME device records: its own workspace, counters, stream and statistics, no copy of the geometry.
static int scene_share_impl(srt_scene* src, srt_scene** out) {
    if (!src || !out) return SRT_ERR_ARG;
    *out = nullptr;
    HIP_TRY(hipSetDevice(src->device));
    alloc_gate();
    std::unique_ptr<srt_scene> s(new srt_scene());
    s->device = src->device; s->dev = src->dev; s->rec = src->rec; s->bytes = src->bytes;
    s->n_textures = src->n_textures; s->has_tex = src->has_tex;
    HIP_TRY(init_handle_state(s.get()));
    *out = s.release();
    return SRT_OK;
}

int srt_scene_share(srt_scene* src, srt_scene** out) {
    return guarded([&] { return scene_share_impl(src, out); });
}

int srt_scene_create(int device, const srt_scene_desc* d, srt_scene** out) {
    return guarded([&] { return scene_create_impl(device, d, out); });
}

// The scene's own stream: srt_render / srt_render_async / srt_scene_update(stream = NULL) are ordered on it.
static void bump_box_epoch(srt_scene* s, hipStream_t stream);

static int own_stream(srt_scene* s, hipStream_t* out) {
    if (!s->stream) HIP_TRY(hipStreamCreateWithFlags(&s->stream.st, hipStreamNonBlocking));
    *out = s->stream;
    return SRT_OK;
}

// The pinned staging block of srt_scene_update, srt_scene_update_frame and srt_scene_pose, at least `bytes` large and free to be written:
// the copies the previous call enqueued out of it have left it (the event `staged`).  For that to hold, EVERY copy out of the block is
// enqueued BEFORE its caller records `staged` on the stream -- a copy behind the event could still be reading what the next call writes.
static int stage_acquire(srt_scene* s, size_t bytes, char** out) {
    if (!s->staged) HIP_TRY(hipEventCreateWithFlags(&s->staged.e, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(s->staged));
    HIP_TRY(s->stage.reserve(bytes));
    *out = s->stage;
    return SRT_OK;
}

// New geometry into the EXISTING device allocations: the reference re-transforms every triangle and rebuilds every hierarchy per
// frame (simple_raytracer.cpp:534-618), so a drop-in caller hands over a new flat scene per frame -- with the same counts (the
// builder's tree shape depends only on the triangle count).  Records are derived straight into one pinned staging block and go
// to the device with asynchronous copies on `stream`: no hipMalloc / hipFree, no pageable copy, no synchronisation with the
// renders already enqueued on that stream (the copies are ordered behind them).
static int scene_update_impl(srt_scene* s, const srt_scene_desc* d, hipStream_t stream) {
    if (!s || !d) return SRT_ERR_ARG;
    SRT_TRY(check_desc(d));
    if (!stream) SRT_TRY(own_stream(s, &stream));
    const bool any_tex = any_textured(d);
    if (d->n_objects != s->dev.n_objects || d->n_nodes != s->dev.n_nodes || d->n_tris != s->dev.n_tris || d->n_textures != s->n_textures ||
        any_tex != s->has_tex || (d->tri_normals != nullptr) != (s->dev.tri_normals != nullptr)) return SRT_ERR_LAYOUT;      // counts differ: create a new scene
    // Texture images: the table (offsets, sizes) must be the uploaded one -- the kernels index with the uploaded tex_w / tex_off --
    // and the image bytes are uploaded again when their content hash differs from what is on the device.  (A second scene with the
    // same counts but other pictures, handed to a renderer that keeps one device scene, must not be shaded with the first one's.)
    SceneRecords& r = *s->rec;
    size_t tex_total = 0;
    bool tex_changed = false;
    uint64_t tex_hash_new = 0;
    if (any_tex) {
        for (uint32_t k = 0; k < d->n_textures; k++) {
            if (d->tex_off[k] != r.tex_off[k] || d->tex_w[k] != r.tex_w[k] || d->tex_h[k] != r.tex_h[k]) return SRT_ERR_LAYOUT;      // another table: create a new scene
            const size_t end = (size_t)d->tex_off[k] + (size_t)d->tex_w[k] * d->tex_h[k] * 3;
            if (end > tex_total) tex_total = end;
        }
        if (tex_total != r.tex_bytes) return SRT_ERR_LAYOUT;
        tex_hash_new = content_hash(d->tex_rgb, tex_total);
        tex_changed = tex_hash_new != r.tex_hash;
    }
    HIP_TRY(hipSetDevice(s->device));
    size_t stage_bytes = 0;
    const RecordList l = record_list(s->dev, r, d, any_tex, tex_changed ? tex_total : 0, false, true, &stage_bytes);
    char* h = nullptr;
    SRT_TRY(stage_acquire(s, stage_bytes, &h));
    SRT_TRY(derive_records(d, l, h));
    for (const RecordArray& a : l) {
        if (!a.bytes()) continue;
        if (a.src) std::memcpy(h + a.off, a.src, a.bytes());
        HIP_TRY(hipMemcpyAsync(*a.dev, h + a.off, a.bytes(), hipMemcpyHostToDevice, stream));
    }
    HIP_TRY(hipEventRecord(s->staged, stream));
    bump_box_epoch(s, stream);
    if (tex_changed) r.tex_hash = tex_hash_new;
    note_records(r, d, l, h);
    return SRT_OK;
}

// Raises the records' box epoch and writes it to the device word in stream order (SceneRecords::box_epoch).  A call captured into a
// graph writes, at every replay, the number it was captured with: never a number that a table made from the host copy carries after it,
// since every later upload has a higher one.
static void bump_box_epoch(srt_scene* s, hipStream_t stream) {
    SceneRecords& r = *s->rec;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }      // (not known: as if it were)
    if (cs != hipStreamCaptureStatusNone) r.boxes_change_in_replays = true;
    r.box_epoch++;
    hipLaunchKernelGGL(k_set_box_epoch, dim3(1), dim3(64), 0, stream, r.d_box_epoch, r.box_epoch);
}
// ---- f1, device half -------------------------------------------------------------------------------------------------------------
static int scene_set_source_impl(srt_scene* s, const float* tri_texcoord, const float* tri_normals, const int32_t* tri_tex) {
    if (!s) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    const size_t nT = s->dev.n_tris;
    if (s->has_tex && (!tri_texcoord || !tri_tex)) return SRT_ERR_ARG;
    if (s->dev.tri_normals && !tri_normals) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(wait_idle(s));
    if (s->has_tex) { SRT_TRY(lazy_array(s, &r.d_src_tc, nT * 24, tri_texcoord, nT * 24)); SRT_TRY(lazy_array(s, &r.d_src_tex, nT * 4, tri_tex, nT * 4)); }
    if (s->dev.tri_normals) SRT_TRY(lazy_array(s, &r.d_src_nrm, nT * 36, tri_normals, nT * 36));
    r.have_source = true;
    return SRT_OK;
}

int srt_scene_set_source(srt_scene* s, const float* tri_texcoord, const float* tri_normals, const int32_t* tri_tex) {
    return guarded([&] { return scene_set_source_impl(s, tri_texcoord, tri_normals, tri_tex); });
}

static int scene_update_frame_impl(srt_scene* s, const srt_frame_geometry* g, hipStream_t stream) {
    if (!s || !g || !g->obj_n_tris || !g->obj_n_nodes || !g->obj_points || !g->obj_order || !g->obj_node_min || !g->obj_node_max) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    const uint32_t nO = s->dev.n_objects;
    if (g->n_objects != nO) return SRT_ERR_LAYOUT;
    for (uint32_t k = 0; k < nO; k++) {
        if ((int32_t)g->obj_n_tris[k] != r.h_tri_first[k + 1] - r.h_tri_first[k] || (int32_t)g->obj_n_nodes[k] != r.h_ranges[k].y - r.h_ranges[k].x) return SRT_ERR_LAYOUT;
        if (g->obj_n_tris[k] && (!g->obj_points[k] || !g->obj_order[k])) return SRT_ERR_ARG;
        if (!g->obj_node_min[k] || !g->obj_node_max[k]) return SRT_ERR_ARG;
    }
    if ((s->has_tex || s->dev.tri_normals) && !r.have_source) return SRT_ERR_ARG;       // attributes cannot be permuted without their source order
    if (!stream) SRT_TRY(own_stream(s, &stream));
    HIP_TRY(hipSetDevice(s->device));
    const size_t nN = s->dev.n_nodes, nT = s->dev.n_tris;
    // the device side of the staging, once
    SRT_TRY(lazy_array(s, &r.d_src_points, nT * 48)); SRT_TRY(lazy_array(s, &r.d_order, nT * 4));
    SRT_TRY(lazy_array(s, &r.d_box_min, nN * 12)); SRT_TRY(lazy_array(s, &r.d_box_max, nN * 12));
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_pts = 0, o_ord = o_pts + pad(nT * 48), o_bmin = o_ord + pad(nT * 4), o_bmax = o_bmin + pad(nN * 12), o_col = o_bmax + pad(nN * 12),
                 o_mat = o_col + pad(nO * 12), o_ubox = o_mat + pad(nO * 12), total = o_ubox + pad(32);
    char* h = nullptr;
    SRT_TRY(stage_acquire(s, total, &h));
    for (uint32_t k = 0; k < nO; k++) {
        const size_t t0 = (size_t)r.h_tri_first[k], nt = g->obj_n_tris[k], n0 = (size_t)r.h_ranges[k].x, nn = g->obj_n_nodes[k];
        if (nt) { std::memcpy(h + o_pts + t0 * 48, g->obj_points[k], nt * 48); std::memcpy(h + o_ord + t0 * 4, g->obj_order[k], nt * 4); }
        std::memcpy(h + o_bmin + n0 * 12, g->obj_node_min[k], nn * 12); std::memcpy(h + o_bmax + n0 * 12, g->obj_node_max[k], nn * 12);
        const uint32_t* ord = g->obj_order[k];
        for (size_t i = 0; i < nt; i += 4099) if (ord[i] >= nt) return SRT_ERR_LAYOUT;       // (spot check: an index outside the object would read another object's points)
    }
    #define CP(dst, off, bytes) do { if (bytes) HIP_TRY(hipMemcpyAsync((void*)(dst), h + (off), (bytes), hipMemcpyHostToDevice, stream)); } while (0)
    const Boxes boxes((const float*)(h + o_bmin), (const float*)(h + o_bmax));      // this frame's
    union_of_roots(boxes, r.h_ranges.data(), nO, (float*)(h + o_ubox));
    CP(r.d_src_points, o_pts, nT * 48); CP(r.d_order, o_ord, nT * 4); CP(r.d_box_min, o_bmin, nN * 12); CP(r.d_box_max, o_bmax, nN * 12);
    CP(s->dev.scene_box, o_ubox, 32);
    if (g->obj_color) { std::memcpy(h + o_col, g->obj_color, nO * 12); CP(s->dev.obj_color, o_col, nO * 12); }
    if (g->obj_material) {
        std::memcpy(h + o_mat, g->obj_material, nO * 12); CP(s->dev.obj_mat, o_mat, nO * 12);
        r.int_shin = all_integer_shininess(g->obj_material, nO);
    }
    #undef CP
    HIP_TRY(hipEventRecord(s->staged, stream));
    const dim3 block(256);
    if (nT) hipLaunchKernelGGL(k_update_tris, dim3((uint32_t)((nT + 255) / 256)), block, 0, stream, (uint32_t)nT, s->dev.tri_obj, s->dev.obj_tri_first,
                               (const float4*)r.d_src_points, (const uint32_t*)r.d_order, const_cast<DevTri*>(s->dev.tris), const_cast<DevTriO*>(s->dev.tris_o),
                               (const float*)r.d_src_tc, const_cast<float*>(s->dev.tri_tc), (const float*)r.d_src_nrm, const_cast<float*>(s->dev.tri_normals),
                               (const int32_t*)r.d_src_tex, s->has_tex ? const_cast<int32_t*>(s->dev.tri_tex) : nullptr);
    hipLaunchKernelGGL(k_update_nodes, dim3((uint32_t)((nN + 255) / 256)), block, 0, stream, (uint32_t)nN, (const float*)r.d_box_min, (const float*)r.d_box_max,
                       const_cast<DevNode*>(s->dev.nodes), const_cast<DevWide*>(s->dev.wide), (const int32_t*)r.d_widx);
    hipLaunchKernelGGL(k_update_roots, dim3((nO + 63) / 64), dim3(64), 0, stream, nO, s->dev.obj_range, (const float*)r.d_box_min, (const float*)r.d_box_max,
                       s->dev.nodes, const_cast<DevNode*>(s->dev.root_nodes));
    bump_box_epoch(s, stream);
    HIP_TRY(hipGetLastError());
    r.have_pose = false;                                        // another visit order: the pose source is no longer these triangles
    r.have_refit = r.have_refit_index = false;                  // ... nor are the refit's indices
    r.overlap = overlap_estimate(boxes, r.h_leaf.data(), (uint32_t)nN, r.h_ranges.data(), nO);      // expected slab tests per ray, from this frame's boxes
    r.prefer_packet = r.overlap > PACKET_OVERLAP_THRESHOLD;
    r.note_root_boxes(boxes, r.h_ranges.data(), nO);
    return SRT_OK;
}

// ---- pose and refit: the hierarchy refitted on the device (srt_kernels.h, "Pose") -------------------------------------------------
// The refit's static schedule, derived from the tree's shape: node heights, the roots of the bottom subtrees, per object the nodes
// above them sorted by height.  Nothing is touched before the tree is known to be within the limit.
struct RefitSchedule {
    std::vector<uint8_t> height; std::vector<int32_t> sub_root, top_nodes, top_off;
};
static int refit_schedule(const SceneRecords& r, size_t nN, size_t nO, RefitSchedule* out) {
    // height of every node (children follow their parent in pre-order); bottom subtrees = maximal subtrees of height <= POSE_SUB_HEIGHT
    alloc_gate();
    std::vector<uint8_t>& height = out->height; std::vector<int32_t>& sub_root = out->sub_root; std::vector<int32_t>& top_nodes = out->top_nodes;
    std::vector<int32_t>& top_off = out->top_off;
    height.assign(nN, 0); top_off.assign(nO + 1, 0);
    std::vector<int32_t> parent(nN, -1);
    for (size_t i = nN; i-- > 0;) {
        if (r.h_leaf[i] >= 0) continue;
        const size_t l = i + 1, rr = (size_t)(~r.h_leaf[i]);
        if (l >= nN || rr >= nN || rr <= l) return SRT_ERR_LAYOUT;                 // (build_device_records has made this impossible)
        const int h = 1 + std::max((int)height[l], (int)height[rr]);
        if (h > 255) return SRT_ERR_LIMIT;
        height[i] = (uint8_t)h; parent[l] = (int32_t)i; parent[rr] = (int32_t)i;
    }
    for (size_t k = 0; k < nO; k++) {
        top_off[k] = (int32_t)top_nodes.size();
        for (int32_t i = r.h_ranges[k].x; i < r.h_ranges[k].y; i++) {
            if (height[i] > POSE_SUB_HEIGHT) top_nodes.push_back(i);
            else if (parent[i] < 0 || height[parent[i]] > POSE_SUB_HEIGHT) sub_root.push_back(i);
        }
        std::stable_sort(top_nodes.begin() + top_off[k], top_nodes.end(), [&](int32_t a, int32_t b) { return height[a] < height[b]; });
    }
    top_off[nO] = (int32_t)top_nodes.size();
    return SRT_OK;
}

// The schedule on the device, with the arrays the refit writes between its launches (each triangle's own box, the box arrays).  The
// device is idle (the caller has waited): no earlier pose or refit still reads what this replaces.
static int refit_schedule_upload(srt_scene* s, const RefitSchedule& c) {
    SceneRecords& r = *s->rec;
    const size_t nN = s->dev.n_nodes, nT = s->dev.n_tris, nO = s->dev.n_objects;
    SRT_TRY(lazy_array(s, &r.d_tri_box, nT * 24));
    SRT_TRY(lazy_array(s, &r.d_height, nN, c.height.data(), nN));
    SRT_TRY(lazy_array(s, &r.d_sub_root, nN * 4, c.sub_root.data(), c.sub_root.size() * 4));      // (capacities for any tree of these counts)
    SRT_TRY(lazy_array(s, &r.d_top_nodes, nN * 4, c.top_nodes.data(), c.top_nodes.size() * 4));
    SRT_TRY(lazy_array(s, &r.d_top_off, (nO + 1) * 4, c.top_off.data(), (nO + 1) * 4));
    SRT_TRY(lazy_array(s, &r.d_box_min, nN * 12));
    SRT_TRY(lazy_array(s, &r.d_box_max, nN * 12));
    r.n_sub = (uint32_t)c.sub_root.size();
    return SRT_OK;
}

// Everything behind the per-triangle launch of a pose or a refit: the boxes from the triangles' own boxes up to the roots, into the
// 32 B, 64 B and root records, and the scene box.  Five launches and the one store of the records' box epoch (bump_box_epoch).
static void enqueue_refit_boxes(srt_scene* s, hipStream_t stream) {
    SceneRecords& r = *s->rec;
    const uint32_t nO = s->dev.n_objects; const size_t nN = s->dev.n_nodes;
    r.root_boxes_valid = false;      // the root boxes change on the device only: no tile spans until the next upload from the host
    bump_box_epoch(s, stream);
    hipLaunchKernelGGL(k_pose_boxes, dim3(r.n_sub), dim3(128), 0, stream, (const int32_t*)r.d_sub_root, s->dev.nodes, (const uint8_t*)r.d_height,
                       (const float2*)r.d_tri_box, r.d_box_min, r.d_box_max);
    hipLaunchKernelGGL(k_pose_top, dim3(nO), dim3(256), 0, stream, (const int32_t*)r.d_top_off, (const int32_t*)r.d_top_nodes, s->dev.nodes,
                       (const uint8_t*)r.d_height, r.d_box_min, r.d_box_max);
    hipLaunchKernelGGL(k_update_nodes, dim3((uint32_t)((nN + 255) / 256)), dim3(256), 0, stream, (uint32_t)nN, (const float*)r.d_box_min, (const float*)r.d_box_max,
                       const_cast<DevNode*>(s->dev.nodes), const_cast<DevWide*>(s->dev.wide), (const int32_t*)r.d_widx);
    hipLaunchKernelGGL(k_update_roots, dim3((nO + 63) / 64), dim3(64), 0, stream, nO, s->dev.obj_range, (const float*)r.d_box_min, (const float*)r.d_box_max,
                       s->dev.nodes, const_cast<DevNode*>(s->dev.root_nodes));
    hipLaunchKernelGGL(k_pose_scene_box, dim3(1), dim3(256), 0, stream, nO, s->dev.obj_range, (const float*)r.d_box_min, (const float*)r.d_box_max,
                       const_cast<float*>(s->dev.scene_box));
}

// Everything proportional to triangles or nodes happens HERE, once: the points go to the device and the refit's static schedule is
// derived from the tree's shape.  Synchronous (a set-up call): waits for the device, so that no earlier pose still reads what it replaces.
static int scene_set_pose_source_impl(srt_scene* s, const float* tri_points) {
    if (!s || !tri_points) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    const size_t nN = s->dev.n_nodes, nT = s->dev.n_tris, nO = s->dev.n_objects;
    RefitSchedule c;
    SRT_TRY(refit_schedule(r, nN, nO, &c));
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(lazy_array(s, &r.d_pose_points, nT * 48, tri_points, nT * 48));
    SRT_TRY(lazy_array(s, &r.d_obj_matrix, nO * 64));
    SRT_TRY(refit_schedule_upload(s, c));
    r.have_pose = true;
    return SRT_OK;
}

int srt_scene_set_pose_source(srt_scene* s, const float* tri_points) {
    return guarded([&] { return scene_set_pose_source_impl(s, tri_points); });
}

// Per frame the host copies 64 bytes an object (+ 24 for colours and materials) into the staging block and enqueues seven launches (the seventh a single store, the records' box epoch); it
// neither looks at a triangle or a node nor waits for the device (but for the staging block's previous use, as srt_scene_update_frame).
static int scene_pose_impl(srt_scene* s, uint32_t n_objects, const float* obj_matrix, const float* obj_color, const float* obj_material, hipStream_t stream) {
    if (!s || !obj_matrix) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    if (!r.have_pose) return SRT_ERR_ARG;
    const uint32_t nO = s->dev.n_objects;
    if (n_objects != nO) return SRT_ERR_LAYOUT;
    if (!stream) SRT_TRY(own_stream(s, &stream));
    HIP_TRY(hipSetDevice(s->device));
    const size_t nT = s->dev.n_tris;
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_mtx = 0, o_col = o_mtx + pad((size_t)nO * 64), o_mat = o_col + pad((size_t)nO * 12), total = o_mat + pad((size_t)nO * 12);
    char* h = nullptr;
    SRT_TRY(stage_acquire(s, total, &h));
    std::memcpy(h + o_mtx, obj_matrix, (size_t)nO * 64);
    HIP_TRY(hipMemcpyAsync(r.d_obj_matrix, h + o_mtx, (size_t)nO * 64, hipMemcpyHostToDevice, stream));
    if (obj_color) { std::memcpy(h + o_col, obj_color, (size_t)nO * 12); HIP_TRY(hipMemcpyAsync((void*)s->dev.obj_color, h + o_col, (size_t)nO * 12, hipMemcpyHostToDevice, stream)); }
    if (obj_material) { std::memcpy(h + o_mat, obj_material, (size_t)nO * 12); HIP_TRY(hipMemcpyAsync((void*)s->dev.obj_mat, h + o_mat, (size_t)nO * 12, hipMemcpyHostToDevice, stream)); }
    HIP_TRY(hipEventRecord(s->staged, stream));
    if (obj_material) r.int_shin = all_integer_shininess(obj_material, nO);
    if (nT) hipLaunchKernelGGL(k_pose_tris, dim3((uint32_t)((nT + 255) / 256)), dim3(256), 0, stream, (uint32_t)nT, s->dev.tri_obj, (const float*)r.d_obj_matrix,
                               (const float4*)r.d_pose_points, const_cast<DevTri*>(s->dev.tris), const_cast<DevTriO*>(s->dev.tris_o), r.d_tri_box);
    enqueue_refit_boxes(s, stream);
    HIP_TRY(hipGetLastError());
    return SRT_OK;
}

int srt_scene_pose(srt_scene* s, uint32_t n_objects, const float* obj_matrix, const float* obj_color, const float* obj_material, void* stream) {
    return guarded([&] { return scene_pose_impl(s, n_objects, obj_matrix, obj_color, obj_material, (hipStream_t)stream); });
}

// ---- visibility masks: the scene's table (include/srt.h, "Visibility masks") ------------------------------------------------------------
// The table is part of the records, so every handle made with srt_scene_share reads it.  The first call makes it (hipMalloc may wait);
// every call writes it through the pinned staging block with a copy ordered on `stream`, as srt_scene_pose writes its matrices.  Nothing
// else of the scene is touched, and no update, pose or refit touches the table.
static int scene_set_object_masks_impl(srt_scene* s, uint32_t n_objects, const uint32_t* masks, hipStream_t stream) {
    if (!s) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    const uint32_t nO = s->dev.n_objects;
    if (n_objects != nO) return SRT_ERR_LAYOUT;
    if (!masks && !r.d_obj_mask) return SRT_OK;      // never set, and set to all ones: the same table
    if (!stream) SRT_TRY(own_stream(s, &stream));
    HIP_TRY(hipSetDevice(s->device));
    char* h = nullptr;
    SRT_TRY(stage_acquire(s, (size_t)nO * 4, &h));
    if (masks) std::memcpy(h, masks, (size_t)nO * 4);
    else std::memset(h, 0xFF, (size_t)nO * 4);
    uint32_t* table = r.d_obj_mask;
    if (!table) SRT_TRY(lazy_array(s, &table, (size_t)nO * 4));
    if (nO) HIP_TRY(hipMemcpyAsync(table, h, (size_t)nO * 4, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->staged, stream));
    r.d_obj_mask = table;      // (only now: a failed first call leaves the scene without a table, i.e. all ones)
    return SRT_OK;
}

int srt_scene_set_object_masks(srt_scene* s, uint32_t n_objects, const uint32_t* masks, void* stream) {
    return guarded([&] { return scene_set_object_masks_impl(s, n_objects, masks, (hipStream_t)stream); });
}

// ---- refit from device points: the caller's vertex buffer in, the same refit behind it (include/srt.h, REFIT) ------------------------
// The set-up call: the schedule, and for the indexed form the indices -- validated here, every one, so that the kernel can gather
// without a compare -- copied to the records once.  Synchronous, as srt_scene_set_pose_source.
static int scene_refit_prepare_impl(srt_scene* s, uint32_t n_verts, const uint32_t* tri_vertex) {
    if (!s) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    const size_t nN = s->dev.n_nodes, nT = s->dev.n_tris, nO = s->dev.n_objects;
    if (tri_vertex) for (size_t i = 0; i < 3 * nT; i++) if (tri_vertex[i] >= n_verts) return SRT_ERR_LAYOUT;
    RefitSchedule c;
    SRT_TRY(refit_schedule(r, nN, nO, &c));
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(refit_schedule_upload(s, c));
    r.have_refit = true; r.have_refit_index = false; r.refit_verts = 0;
    if (tri_vertex) {
        SRT_TRY(lazy_array(s, &r.d_tri_vertex, nT * 12, tri_vertex, nT * 12));
        r.have_refit_index = true; r.refit_verts = n_verts;
    }
    return SRT_OK;
}

int srt_scene_refit_prepare(srt_scene* s, uint32_t n_verts, const uint32_t* tri_vertex) {
    return guarded([&] { return scene_refit_prepare_impl(s, n_verts, tri_vertex); });
}

extern "C++" template <bool INDEXED, bool STRIDE4, bool WIDE>
static void launch_refit_tris(srt_scene* s, const srt_refit_desc* g, hipStream_t stream) {
    SceneRecords& r = *s->rec;
    const uint32_t nT = s->dev.n_tris;
    const dim3 grid((nT + 255) / 256), block(256);
    if (g->d_normals)
        hipLaunchKernelGGL((k_refit_tris<INDEXED, STRIDE4, WIDE, true>), grid, block, 0, stream, nT, g->d_points, (const uint32_t*)r.d_tri_vertex, g->d_normals,
                           const_cast<DevTri*>(s->dev.tris), const_cast<DevTriO*>(s->dev.tris_o), r.d_tri_box, const_cast<float*>(s->dev.tri_normals));
    else
        hipLaunchKernelGGL((k_refit_tris<INDEXED, STRIDE4, WIDE, false>), grid, block, 0, stream, nT, g->d_points, (const uint32_t*)r.d_tri_vertex, (const float*)nullptr,
                           const_cast<DevTri*>(s->dev.tris), const_cast<DevTriO*>(s->dev.tris_o), r.d_tri_box, (float*)nullptr);
}

// Per frame: seven launches (the seventh a single store, the records' box epoch) and nothing else -- no allocation, no copy, no staging, no look at a triangle or a node, no wait.
static int scene_refit_device_impl(srt_scene* s, const srt_refit_desc* g, hipStream_t stream) {
    if (!s || !g || !g->d_points) return SRT_ERR_ARG;
    if (g->stride != 3 && g->stride != 4) return SRT_ERR_ARG;
    SceneRecords& r = *s->rec;
    if (!r.have_refit) return SRT_ERR_ARG;
    const bool indexed = g->n_verts != 0;
    if (indexed && !r.have_refit_index) return SRT_ERR_ARG;
    if (g->d_normals && !s->dev.tri_normals) return SRT_ERR_ARG;
    if (indexed && g->n_verts != r.refit_verts) return SRT_ERR_LAYOUT;
    if (!stream) SRT_TRY(own_stream(s, &stream));
    HIP_TRY(hipSetDevice(s->device));
    const bool s4 = g->stride == 4, wide = s4 && ((uintptr_t)g->d_points & 15) == 0;
    if (s->dev.n_tris) {
        if (indexed) { if (wide) launch_refit_tris<true, true, true>(s, g, stream); else if (s4) launch_refit_tris<true, true, false>(s, g, stream); else launch_refit_tris<true, false, false>(s, g, stream); }
        else { if (wide) launch_refit_tris<false, true, true>(s, g, stream); else if (s4) launch_refit_tris<false, true, false>(s, g, stream); else launch_refit_tris<false, false, false>(s, g, stream); }
    }
    enqueue_refit_boxes(s, stream);
    HIP_TRY(hipGetLastError());
    return SRT_OK;
}

int srt_scene_refit_device(srt_scene* s, const srt_refit_desc* g, void* stream) {
    return guarded([&] { return scene_refit_device_impl(s, g, (hipStream_t)stream); });
}

int srt_scene_update_frame(srt_scene* s, const srt_frame_geometry* g, void* stream) {
    return guarded([&] { return scene_update_frame_impl(s, g, (hipStream_t)stream); });
}

int srt_scene_update(srt_scene* s, const srt_scene_desc* d, void* stream) {
    return guarded([&] { return scene_update_impl(s, d, (hipStream_t)stream); });
}

void srt_debug_fail_host_allocs(int n) { g_fail_allocs.store(n < 0 ? 0 : n); }

int srt_debug_scene_records(srt_scene* s, void* nodes, void* tris, void* tris_o, void* wide, void* root_nodes,
                            float* tri_texcoord, float* tri_normals, int32_t* tri_tex) {
    if (!s) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(s->device));
    if (s->stream) HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipDeviceSynchronize());
    const size_t nN = s->dev.n_nodes, nT = s->dev.n_tris, nO = s->dev.n_objects, nW = (nN - nO) / 2;
    #define DOWN(dst, src, bytes) do { if ((dst) && (src) && (bytes)) HIP_TRY(hipMemcpy((dst), (src), (bytes), hipMemcpyDeviceToHost)); } while (0)
    DOWN(nodes, s->dev.nodes, nN * sizeof(DevNode)); DOWN(tris, s->dev.tris, nT * sizeof(DevTri)); DOWN(tris_o, s->dev.tris_o, nT * sizeof(DevTriO));
    DOWN(wide, s->dev.wide, nW * sizeof(DevWide)); DOWN(root_nodes, s->dev.root_nodes, nO * sizeof(DevNode));
    DOWN(tri_texcoord, s->dev.tri_tc, nT * 24); DOWN(tri_normals, s->dev.tri_normals, nT * 36); DOWN(tri_tex, s->dev.tri_tex, nT * 4);
    #undef DOWN
    return SRT_OK;
}

uint64_t srt_scene_device_bytes(const srt_scene* s) { return s ? s->bytes : 0; }
const char* srt_scene_pipeline(const srt_scene* s) { return s ? s->pipeline : ""; }
double srt_scene_overlap_estimate(const srt_scene* s) { return s ? s->rec->overlap : 0.; }

// ---- which kernels a frame runs ---------------------------------------------------------------------------------------------
// srt_params.flags bits 8..15 select a kernel variant.  This is the list of the numbers (include/srt.h and DESIGN.md s5 point here): 0 is
// what ships, every other number computes the same frame with older or differently configured kernels -- the independent
// implementations the parity tests pin the shipped kernels with, and the A/B measurements of DESIGN.md s5.
enum Variant : uint32_t {
    V_SHIPPED = 0,                // the pipeline plan_frame picks per scene and light-sample count
    V_REFERENCE = 1,              // the first kernels: a ray per lane with an inline triangle loop, per-pixel shading (no workspaces, no smooth normals)
    V_TRI_QUEUE = 2,              // a ray per lane with a wave triangle queue, then the node-queue shadow kernel
    V_NQ_TINY = 3,                // unfused node-queue kernels, 160-entry queue and exact divides: the stackless overflow walk
    V_NQ_EXACT = 4,               // unfused node-queue kernels, shipped geometry with exact divides only
    V_NQ_8X4 = 5,                 // unfused, 8x4 pixels per wave and a 1024-entry queue (tile-size experiment)
    V_NQ_TINY_FILTER = 6,         // unfused, 160-entry queue with the filtered slab test: the overflow walk as shipped
    V_UNFUSED = 10,               // the shipped node-queue kernels unfused (closest hit, then shadow)
    V_FUSED_5_WAVES = 11,         // the fused kernel built for 5 waves per SIMD
    V_FUSED_ROOTS_AGAIN = 12,     // the fused kernel with the roots re-tested by every wave (round-1 form)
    V_FUSED_HALF = 13,            // the fused kernel's half-tile form (two waves of 8x4 pixels per tile) also without SRT_FLAG_FRAMES_IN_FLIGHT
    V_FUSED_HALF_TINY = 14,       // the half-tile form with a 160-entry node queue: the stackless overflow walk at 32 rays per wave
    V_FUSED_HALF_1024 = 15,       // the half-tile form with a 1024-entry node queue (15,240 B of LDS: ten workgroups per CU)
    V_FUSED_HALF_32_RAYS = 16,    // the half-tile form with 32 shadow rays in flight per wave
    V_FUSED_64_RAYS = 17,         // the fused kernel with 64 shadow rays in flight per wave
    V_XCD_ROWS = 18,              // whole tile rows dealt to XCDs (what records beyond 32 MiB get), forced
    V_FUSED_HALF_6_WAVES = 19,    // the half-tile form built for 6 waves per SIMD: twelve workgroups per CU by VGPRs (the LDS overlay without its residency)
    V_CHUNKED = 20,               // never fused; 8+ samples: node-queue shadow kernel, samples cut into chunks over blockIdx.z (round-1 form)
    V_NQ_PK = 21,                 // node-queue closest hit + packet shadow kernel at any sample count
    V_PK_PK = 22,                 // packet closest hit + packet shadow kernel
    V_PK_NQ = 23,                 // packet closest hit + node-queue shadow kernel
    V_NO_PACKET = 24,             // the shipped choice for a scene WITHOUT the packet preference (A/B on soups)
    V_PK_WINDOWS = 25,            // shipped choice, the packet shadow kernel reading its records through LDS windows
    V_COARSE_GRID = 27,           // shipped choice, 2 x 2 tiles per workgroup in the unfused closest-hit launch
    V_TRACE_SHADE = 28,           // the fused kernel shades its tiles itself: the frame in one launch (below 64 samples, no XCD rows)
    V_PK_ENTRY_ORDER = 29,        // shipped choice, the packet shadow kernel's units in entry order
    V_FUSED_HALF_8_WAVES = 30,    // the half-tile form's eight-wave build (384-entry queue, no packed f32 operations) also without SRT_FLAG_FRAMES_IN_FLIGHT, as 13 is the seven-wave one
    V_WAVE_8 = 31,                // 0 in everything but the in-flight hint's part in the trace kernel: the eight-wave build, and over tile spans its one-wave workgroups, also without SRT_FLAG_FRAMES_IN_FLIGHT
    V_WAVE_8_ADJACENT = 32,       // 0 in everything but the dispatch order of the one-wave workgroups: a tile's halves next to each other (on neighbouring XCDs), at every light-sample count (measured, not shipped)
    V_CAMERA_PK = 35,             // shipped choice, camera mode on the packet closest-hit kernel at every sample count
    V_ROUND2_FORM = 40,           // shipped choice, the round-2 form everywhere: 32 B node records, queue pushes in lane order
    V_ALL_WIDE = 41,              // shipped choice, 64 B node records in every node-queue kernel
    V_ALL_NARROW = 42,            // shipped choice, 32 B node records in every node-queue kernel
    V_LANE_ORDER = 43,            // shipped choice, queue pushes in lane order
    V_GENERAL_SHADE = 44,         // shipped choice, the general shading kernel where the integer-shininess one would run
    V_ROOT_LOOP = 45,             // shipped choice, a tile's root tests by the round-2 loop of dependent loads
    V_NO_UNION_BOX = 46,          // shipped choice, without the test against the union of the root boxes
    V_WIDE_STEP_COUNTERS = 47,    // shipped choice, diagnostic counters of the wide shadow kernel's steps
    V_HIT_6_WAVES = 53,           // shipped choice, the unfused closest-hit kernel without the 7-wave bound
    V_FUSED_6_WAVES = 54,         // shipped choice, the fused kernel built for 6 waves per SIMD
    V_PK_AHEAD = 55,              // shipped choice, packet shadow walk with the record of i + 1 requested ahead
    V_PK_AHEAD_SKIP = 56,         // shipped choice, ... and skip[i] / the leaf's first triangle
    V_PK_PLAIN = 57,              // shipped choice, the plain packet shadow walk under a number (never the heavy lists)
    V_PK_CLOCKS = 58,             // shipped choice, the plain walk with per-wave clock stamps (SRT_DIAG_COUNTERS)
    V_FUSED_FOUR_WAVES = 59,      // shipped choice, the fused kernel as four waves of 4x4 pixels per tile where the half-tile form would run
    V_SHADOW_PLAIN_ROWS = 62,     // shipped choice, the node-queue shadow kernel in plain tile order where XCD rows are on
    V_EXACT_TONE = 63,            // shipped choice, every pixel's tone map by the exact functions (no f32 filter: EXP_EXACT_TONE)
    V_FULL_GRID = 64,             // 0 in everything (batch hold-back, heavy lists, camera build included) but the tile spans: off, every tile gets its workgroup
    V_HALF_7_WAVES = 65,          // 0 in everything (tile spans included) but the half-tile form's build: the seven-wave one with its 512-entry queue, as before the eight-wave build
    V_HALF_8_WAVES_256 = 66,      // 0 in everything but the half-tile form's node queue: the eight-wave build with 256 entries (eight LDS granules as well: what the smaller queue costs)
    V_HALF_8_TWO_WAVES = 67,      // 0 in everything but the workgroups of the eight-wave build over tile spans: two waves a tile (k_trace_nq_half8_spans), as before the one-wave workgroups
    V_WAVE_8_GENERAL = 68,        // 0 in everything but the one-wave workgroups' kernels: the general frame's (k_trace_nq_wave8_spans, k_shade_tile_spans), as before the whole-frame form
};
// Numbers without a name keep two fallbacks: 7..9 run the unfused node-queue chain of the shipped kernels, any other number a
// configuration of the fused kernel (the shipped one) at every sample count.
static inline uint32_t variant_of(const srt_params* p) { return (p->flags >> 8) & 0xffu; }
// 64 .. 68, 31 and 32 are 0 with one thing of the shipped frame switched: every rule that asks for 0 holds for them.
static inline uint32_t variant_or_shipped(const srt_params* p) { const uint32_t v = variant_of(p); return (v >= V_FULL_GRID && v <= V_WAVE_8_GENERAL) || v == V_WAVE_8 || v == V_WAVE_8_ADJACENT ? (uint32_t)V_SHIPPED : v; }
// These run the pipeline the dispatcher picks for 0.  They are NOT 0 for what only the shipped frame gets: the batch hold-back, the
// chunked launch for scenes of few nodes, the heavy-quadrant lists and the camera build of the fused kernel.  28 is deliberately not
// among them: it is a configuration of the fused kernel (fused_config in plan_frame) and takes the fused launch at every sample count.
static inline bool shipped_choice(uint32_t v) {
    return v == V_SHIPPED || v == V_NO_PACKET || v == V_PK_WINDOWS || v == V_COARSE_GRID || v == V_PK_ENTRY_ORDER || v == V_CAMERA_PK ||
           (v >= V_ROUND2_FORM && v <= V_SHADOW_PLAIN_ROWS) || v == V_EXACT_TONE;
}

// Kernels of one argument list have one type: a plan names the instantiation as a value, one statement per list launches it.
using RefHitFn = decltype(&k_closest_hit<false>);
using RefShadeFn = decltype(&k_shade<false>);
using QHitFn = decltype(&k_closest_hit_q<false>);
using NqHitFn = decltype(&k_closest_hit_nq<false, 512, 2, 2, true>);
using PkHitFn = decltype(&k_closest_hit_pk<false, true, false>);
using TraceFn = decltype(&k_trace_nq<false, 512, true, 7, 16>);
using TraceShadeFn = decltype(&k_trace_shade_nq<512, true, 6, 16>);
using ShadowPkFn = decltype(&k_shadow_pk<false, true, false>);
using ShadowNqFn = decltype(&k_shadow_nq<false, 512, true, 16, 6>);
using ShadeTileFn = decltype(&k_shade_tile<0>);
using TraceSpansFn = decltype(&k_trace_nq_spans<512, true, 7, 16>);
using ShadeTileSpansFn = decltype(&k_shade_tile_spans<0>);

// CONSTRAINT on plan_frame and the batch launches below: every kernel is named in a chain of plain assignments, in this order.  The
// compiler emits the instantiations in the order it meets them, and ?: chains are met last operand first: reordering the statements
// or folding them into ?: changes no behaviour, but the code object's layout, and with it tools/kernel_regs.py --digest, the check
// that a host-only change left the kernels alone.

enum BatchState { NOT_BATCHED, BATCH_FITS, BATCH_OTHER_SIZE };      // srt_render_device_batch is collecting, and this frame has the size of the frames it holds (or not)
enum Hold { HOLD_NONE, HOLD_FUSED, HOLD_PK };                       // the two classes of frames a batch call launches together

// What the choice of a frame's kernels depends on besides the caller's params: estimates and sizes of the scene, the device's CU
// count, the process's environment.
struct SceneFacts {
    bool prefer_packet, int_shin, normals; double overlap; uint64_t bytes; uint32_t n_cu;
    uint32_t heavy_steps, pk_units, pk_take;      // SRT_HEAVY_STEPS, SRT_PK_UNITS, SRT_PK_TAKE (read once per process)
    // the host copy of the root boxes (n_objects x 3 floats each) where it is valid, else null: what the tile spans are made from
    uint32_t n_objects; const float* root_min; const float* root_max; uint32_t box_epoch;
};
static SceneFacts scene_facts(const srt_scene* s) {
    static const auto env = [](const char* name, uint32_t dflt) { const char* e = std::getenv(name); return e ? (uint32_t)std::strtoul(e, nullptr, 10) : dflt; };
    static const uint32_t heavy_steps = env("SRT_HEAVY_STEPS", 64u);      // walks of this many node steps make a quadrant a heavy one (0 = off)
    static const uint32_t pk_units = env("SRT_PK_UNITS", 64u), pk_take = env("SRT_PK_TAKE", 4u);
    const bool boxes_known = s->rec->root_boxes_valid && !s->rec->boxes_change_in_replays;
    return SceneFacts{s->rec->prefer_packet, s->rec->int_shin, s->dev.tri_normals != nullptr, s->rec->overlap, s->bytes, (uint32_t)s->n_cu,
                      heavy_steps, pk_units, pk_take, s->dev.n_objects,
                      boxes_known ? s->rec->h_root_min.data() : nullptr, boxes_known ? s->rec->h_root_max.data() : nullptr, s->rec->box_epoch};
}

// Every check of a render's arguments: before any state of the handle changes (counter sets, pending work).
static int check_frame(const SceneFacts& f, const srt_params* p) {
    if (!p || !p->width || !p->height || !p->block_rows || !p->block_stride) return SRT_ERR_ARG;
    const uint32_t v = variant_or_shipped(p);
    if (p->ray_matrix && v != V_SHIPPED && v != V_PK_PK && v != V_CAMERA_PK) return SRT_ERR_ARG;      // camera mode: shipped pipelines only
    if (p->n_lights && !p->light_pos) return SRT_ERR_ARG;
    if (p->block_cols && ((p->block_cols & 7u) || (p->block_rows & 7u) || p->block_first >= p->block_stride)) return SRT_ERR_ARG;   // tiles of whole 8x8 pixel blocks
    if (p->spp < 1 || p->spp > 4096) return SRT_ERR_ARG;
    { const uint32_t n = (uint32_t)std::lround(std::sqrt((double)p->spp)); if (n * n != p->spp) return SRT_ERR_ARG; }   // n x n sub-pixel grid
    if ((uint64_t)p->width * p->height >= (1ull << 31)) return SRT_ERR_LIMIT;
    if ((uint64_t)p->width * p->height * (p->n_lights ? p->n_lights : 1) >= (1ull << 32)) return SRT_ERR_LIMIT;   // 32-bit work-item index
    if (p->spp > 1 && (uint64_t)srt_cols_owned(p) * srt_rows_owned(p) * 3 >= (1ull << 32)) return SRT_ERR_LIMIT;   // the accumulation buffer's 32-bit float index
    return (p->flags & SRT_FLAG_SMOOTH_NORMALS) && (!f.normals || v == V_REFERENCE) ? SRT_ERR_ARG : SRT_OK;   // needs vertex normals
}

// One render's launches.  Pipelines (variant 0 picks per scene and light count; the numbered variants force one):
//   fused        k_trace_nq (node-queue closest hit + shadow rays in one launch): 1..7 light samples
//   nq + pk      node-queue closest hit, then the packet shadow kernel over the list of quadrants with hits: 8+ light samples
//                (the samples of a pixel walk the other objects' trees in lock step), or variant 21 at any count
//   pk + nq      packet closest hit, then the node-queue shadow kernel: hierarchies of heavily overlapping boxes (the 1 M soup:
//                neighbouring primary rays test the same ~2,500 nodes, while the shadow rays of a tile start all over the
//                scene), 1..7 light samples, or variant 23
//   pk + pk      both packet kernels: such scenes with 8+ light samples, or variant 22
//   nq chunked   k_shadow_nq with 64 rays in flight and the samples cut over blockIdx.z: 8..15 samples on scenes of few nodes, or variant 20
// camera mode (rays that do not start at the origin): the fused node-queue kernel has a build for rays with an origin (1..7
// samples, variant 0); everything else in camera mode goes through the packet closest-hit kernel, which takes a general ray.  The
// shadow kernels start from the hit point either way.
struct FramePlan {
    // stage 1, closest hit or the fused trace: one of these
    RefHitFn ref_hit = nullptr; QHitFn q_hit = nullptr; NqHitFn nq_hit = nullptr; PkHitFn pk_hit = nullptr; TraceFn trace = nullptr; TraceShadeFn trace_shade = nullptr;
    // stage 2, shadow rays: at most one (none without light samples and behind a trace kernel); l_chunk: k_shadow_nq's light samples per blockIdx.z
    ShadowPkFn shadow_pk = nullptr; ShadowNqFn shadow_nq = nullptr; uint32_t l_chunk = 0xffffffffu;
    // stage 3, shading: one of these (none behind k_trace_shade_nq)
    RefShadeFn ref_shade = nullptr; ShadeTileFn shade_tile = nullptr;
    dim3 grid_hit, grid_shadow, grid_shade;
    uint32_t block_hit = 256;                     // threads per workgroup of stage 1 (the half-tile trace kernel: 128, its one-wave workgroups over tile spans: 64); every other launch has 256
    // the DevParams fields that belong to the choice (dev_params copies them); xcd_rows as the shadow stage sees it, shadow_px_major as
    // the shading stage does
    uint32_t exp = 0, heavy_steps = 0, pk_units = 0, pk_take = 1, xcd_rows = 0, shadow_xcd_rows = 0, shadow_px_major = 0;
    // workspaces
    size_t shadow_words = 0; uint32_t qcap_need = 0;      // shadow bits; entries per shard of the quadrant list.  0: none (variant 1 only -- a
                                                          // frame that owns a row owns a tile, so every other plan needs at least one word and one entry)
    bool quadrants_consumed = false;              // the closest-hit kernel fills the quadrant list only for a consumer
    Hold hold = HOLD_NONE;                        // held back for the batch call's launches: no stage kernel is set
    char pipeline[96] = "";                       // srt_scene_pipeline
    // the frame's tile spans (srt_tile_spans.h).  on: trace_spans and shade_tile_spans take the places of trace and shade_tile -- the same
    // bodies with the table as their last argument --, grid_hit is (widest span, live tile rows), and the shading launch fills the tiles
    // outside the spans with background
    TileSpans spans{}; TraceSpansFn trace_spans = nullptr; ShadeTileSpansFn shade_tile_spans = nullptr;
    dim3 grid_hit_full;                           // with spans: the frame's whole grid, which a launch that is being captured into a graph keeps
};

// Decides a render: touches nothing, calls nothing of HIP.  p has passed check_frame and owns at least one row.
static FramePlan plan_frame(const SceneFacts& f, const srt_params* p, BatchState batch) {
    FramePlan pl;
    const bool full_grid = variant_of(p) == V_FULL_GRID;
    const uint32_t v = variant_or_shipped(p), L = p->n_lights, wl = srt_cols_owned(p), rows = srt_rows_owned(p);
    const bool count = (p->flags & SRT_FLAG_COUNT_WORK) != 0, in_flight = (p->flags & SRT_FLAG_FRAMES_IN_FLIGHT) != 0, cam = p->ray_matrix != nullptr, shipped = shipped_choice(v);
    const dim3 grid16((wl + 15) / 16, (rows + 15) / 16), grid8((wl + 7) / 8, (rows + 7) / 8);      // grid8: 8x8 pixels per workgroup, 4 waves x (4x4 pixels)
    const auto xcd_pad = [](uint32_t y) { return (y + 7) / 8 * 8; };      // whole tile rows per XCD: y padded to 8 rows
    const size_t n_tiles = (size_t)grid8.x * grid8.y, pixels = (size_t)wl * rows;

    pl.exp = ((v == V_ROUND2_FORM || v == V_LANE_ORDER) ? 1u : 0u) | (v == V_ROOT_LOOP ? 2u : 0u) | (v == V_WIDE_STEP_COUNTERS ? 4u : 0u) | (v == V_NO_UNION_BOX ? 8u : 0u) |
             (v == V_EXACT_TONE ? EXP_EXACT_TONE : 0u) | ((v == V_TRACE_SHADE || v == V_TRI_QUEUE) ? 32u : 0u);      // (32: the kernel counts the hits itself -- the hit statistic is not the shading kernel's)
    pl.xcd_rows = (f.bytes > (32ull << 20) || v == V_XCD_ROWS) ? 1u : 0u;      // records far beyond one XCD's 4 MiB L2
    pl.pk_units = in_flight ? f.pk_units : 0u; pl.pk_take = in_flight && f.pk_take ? f.pk_take : 1u;
    pl.grid_shade = grid16;

    if (v == V_REFERENCE) {
        if (count) pl.ref_hit = &k_closest_hit<true>; else pl.ref_hit = &k_closest_hit<false>;
        if (count) pl.ref_shade = &k_shade<true>; else pl.ref_shade = &k_shade<false>;
        pl.grid_hit = grid16;
        std::snprintf(pl.pipeline, sizeof(pl.pipeline), "k_closest_hit+k_shade");
        return pl;
    }
    // workspace of the tile pipeline.  Shadow bits: tile-major (one 64-bit word per 8x8 tile and light sample, node-queue kernels) or
    // pixel-major (one word per pixel and 64 light samples, packet shadow kernel): room for either.  Quadrant list: a shard gets
    // every 64th tile, four quadrants each
    const size_t words_tile = n_tiles * (L ? L : 1), words_px = pixels * ((L + 63) / 64);
    pl.shadow_words = words_tile > words_px ? words_tile : words_px;
    pl.qcap_need = (uint32_t)((n_tiles + QL_SHARDS - 1) / QL_SHARDS) * 4u;

    // (check_frame: camera mode takes 0, 22 and 35)
    const bool cam_nq = cam && v == V_SHIPPED && !count && !f.prefer_packet && L >= 1 && L < 8 && !pl.xcd_rows;
    const bool pk_closest = (cam && !cam_nq) || v == V_PK_PK || v == V_PK_NQ || (shipped && f.prefer_packet && v != V_NO_PACKET);
    // 8 .. 15 samples on a scene whose rays test few nodes (expected slab tests per ray < 14: cube scenes 3-6, bunny over a slab 12):
    // the node-queue shadow kernel with the samples cut over blockIdx.z beats the packet walk since round 3's queue order (K3 with
    // 8 / 12 samples 0.212 / 0.281 ms against 0.254 / 0.321, cube over ground with 8: 0.107 against 0.197); the composite scene
    // (seven objects, tree crowns; estimate 17+) and 16+ samples stay with the packet walk (K4 with 8 / 12: 0.390 / 0.473 against 0.416 / 0.621)
    const bool few_nodes_mid = v == V_SHIPPED && !count && !cam && L >= 8 && L < 16 && f.overlap < 14.0 && !f.prefer_packet;
    const bool pk_shadow = L && (v == V_NQ_PK || v == V_PK_PK || (shipped && L >= 8 && !few_nodes_mid));
    const bool chunked = L >= 8 && !count && (v == V_CHUNKED || few_nodes_mid);
    // The two fallback rows for numbers without a name.  Above 10: a configuration of the fused kernel at every sample count, as the
    // named 11 .. 18 and 28 (20 .. 23 force a pipeline through chunked / pk_shadow / pk_closest).  7 .. 9: neither row below, so
    // the unfused chain of the `default` branch -- the 7-wave closest-hit build, then k_shadow_nq.
    const bool fused_config = !shipped && v > 10 && v != V_CHUNKED;
    const bool fused = L && (shipped || fused_config) && !chunked && !pk_shadow && !pk_closest;
    pl.quadrants_consumed = pk_shadow; pl.shadow_px_major = pk_shadow ? 1u : 0u;

    // held back: the batch call launches this frame together with the others (same kernels, same arguments)
    const bool holdable = batch == BATCH_FITS && v == V_SHIPPED && !count && p->spp == 1 && !pk_closest;
    if (holdable && (fused ? !pl.xcd_rows && !cam : pk_shadow)) {
        // 8+ light samples (HOLD_PK): node-queue closest hit, packet shadow kernel and shading of the batch's frames in three launches.
        // Packet shadow walks of heavy_steps node steps put their quadrant on the heavy list of the next frame (srt_kernels.h): the
        // shadow rays of a batch are ONE launch and its tail is idle machine (a K4 step of eight share-frames 2.24 -> 1.73 ms).
        // pk_take: unit numbers four at a time, fewer same-address atomics (srt_packet.h).  pk_units 0: the frames of a batch share the
        // machine, every frame keeps its part of the grid (K3 with 16 samples, an eighth: 0.45 ms per step against 0.68 with surplus waves leaving)
        pl.hold = fused ? HOLD_FUSED : HOLD_PK;
        if (!fused) { pl.heavy_steps = f.heavy_steps; pl.pk_take = f.pk_take ? f.pk_take : 1u; pl.pk_units = 0u; }
        std::snprintf(pl.pipeline, sizeof(pl.pipeline), fused ? "k_trace_nq+k_shade_tile (batched)" : "k_closest_hit_nq+k_shadow_pk+k_shade_tile (batched)");
        return pl;
    }
    // A frame that has the device to itself (no in-flight hint, not part of a batch call): quadrants whose walks were long in this
    // handle's previous frame are dealt early (srt_kernels.h) -- nothing else fills the slots the launch's tail frees.  Same box:
    // K3 with 16 samples on one stream 4.04 -> 3.70 ms per 8 frames, K4 11.89 -> 11.72.  Frames launched one by one on several streams
    // pipeline -- the next frame's closest-hit launch fills the slots a tail frees -- and the lists LOSE (K4 on four streams 9.41 ->
    // 9.64, the reference's main() scene 6.55 -> 6.91), so the hint turns them off.
    if (pk_shadow && v == V_SHIPPED && !count && !in_flight && batch == NOT_BATCHED) pl.heavy_steps = f.heavy_steps;

    // stage 1
    // closest-hit kernel: CAP = node queue entries, TWL/THL = log2 tile size per wave, FILTER = filtered slab test
    #define NQ_HIT(CAP, TWL, THL, FILTER) do { \
        if (count) pl.nq_hit = &k_closest_hit_nq<true, CAP, TWL, THL, FILTER>; else pl.nq_hit = &k_closest_hit_nq<false, CAP, TWL, THL, FILTER>; \
        pl.grid_hit = dim3((wl + (2u << TWL) - 1) / (2u << TWL), (rows + (2u << THL) - 1) / (2u << THL)); } while (0)
    pl.grid_hit = grid8;
    switch (v) {
    case V_TRI_QUEUE:
        if (count) pl.q_hit = &k_closest_hit_q<true>; else pl.q_hit = &k_closest_hit_q<false>;
        pl.grid_hit = grid16; break;
    case V_NQ_TINY:        NQ_HIT(160, 2, 2, false); break;
    case V_NQ_EXACT:       NQ_HIT(512, 2, 2, false); break;
    case V_NQ_TINY_FILTER: NQ_HIT(160, 2, 2, true); break;
    case V_NQ_8X4:         NQ_HIT(1024, 3, 2, false); break;
    case V_UNFUSED:        NQ_HIT(512, 2, 2, true); break;
    default:
        if (pk_closest) {              // one wavefront per 8x8 tile walks the trees in lock step; a workgroup = 2 x 2 tiles
            const bool xcd = pl.xcd_rows && !cam && !count;
            if (cam && count)  pl.pk_hit = &k_closest_hit_pk<true, true, false, true>;
            else if (cam)      pl.pk_hit = &k_closest_hit_pk<false, true, false, true>;
            else if (count)    pl.pk_hit = &k_closest_hit_pk<true, true, false>;
            else if (xcd)      pl.pk_hit = &k_closest_hit_pk<false, true, true>;
            else               pl.pk_hit = &k_closest_hit_pk<false, true, false>;
            pl.grid_hit = dim3((grid8.x + 1) / 2, xcd ? xcd_pad((grid8.y + 1) / 2) : (grid8.y + 1) / 2);
        } else if (fused && v == V_TRACE_SHADE && !count && !pl.xcd_rows && L < 64) {
            pl.trace_shade = &k_trace_shade_nq<512, true, 6, 16>;
        } else if (fused) {            // closest hit + shadow rays in one launch
            // Two waves of 8x4 pixels per tile where frames are in flight on several streams: half the waves hold a CU's wave slots for the
            // same pairs, and the next frame's launch fills the tail that a wave living twice as long leaves (36 frames on four streams
            // 4.13 -> 3.37 ms).  A frame that has the device to itself pays for that tail -- the launch alone 0.108 -> 0.136 ms
            // -- and keeps four waves per tile, as do the camera, counting and XCD-row builds below.  The build for seven waves per SIMD
            // (the closest-hit phase's dir[] and best[] over the shadow phase's LDS: fourteen workgroups per CU instead of twelve) takes the
            // 36 frames from 3.37 to 3.23 ms; 19 keeps the six-wave build of the same body.  The build for eight waves per SIMD (no packed f32
            // operations: 64 VGPRs without scratch; 384 queue entries: eight LDS granules, sixteen workgroups per CU) takes them from 3.03 to
            // 2.67 ms; 65 keeps the seven-wave build in its place, 66 runs the eight-wave one with 256 entries, 30 forces it without the hint.
            // Over tile spans the eight-wave build runs as workgroups of ONE wave, a half tile each (k_trace_nq_wave8_spans, chosen with the
            // spans below) up to four light samples; 67 keeps the two-wave workgroups, 31 takes the eight-wave build and its one-wave workgroups
            // without the hint and at every sample count.
            const bool hinted = in_flight || variant_of(p) == V_WAVE_8;
            const bool half_tile = (v == V_SHIPPED && hinted) || v == V_FUSED_HALF;
            const bool half_eight = (v == V_SHIPPED && hinted && variant_of(p) != V_HALF_7_WAVES) || v == V_FUSED_HALF_8_WAVES;      // (13 keeps the seven-wave build)
            if (cam_nq)                        pl.trace = &k_trace_nq<false, 512, true, 5, 16, false, false, true>;      // camera mode on the node queues
            else if (count)                    pl.trace = &k_trace_nq<true, 512, true, 5, 16>;
            else if (v == V_FUSED_5_WAVES)     pl.trace = &k_trace_nq<false, 512, true, 5, 16>;
            else if (v == V_FUSED_ROOTS_AGAIN) pl.trace = &k_trace_nq<false, 512, true, 6, 16, false, true>;
            else if (v == V_FUSED_64_RAYS)     pl.trace = &k_trace_nq<false, 512, true, 5, 64>;
            else if (v == V_FUSED_6_WAVES)     pl.trace = &k_trace_nq<false, 512, true, 6, 16>;
            else if (v == V_ALL_WIDE)          pl.trace = &k_trace_nq<false, 512, true, 6, 16, false, false, false, true>;
            else if (pl.xcd_rows)            { pl.trace = &k_trace_nq<false, 512, true, 6, 16, true>; pl.grid_hit.y = xcd_pad(grid8.y); }
            else if (v == V_FUSED_HALF_TINY) { pl.trace = &k_trace_nq_half<160, true, 6, 16>; pl.block_hit = 128; }
            else if (v == V_FUSED_HALF_1024) { pl.trace = &k_trace_nq_half<1024, true, 5, 16>; pl.block_hit = 128; }
            else if (v == V_FUSED_HALF_32_RAYS) { pl.trace = &k_trace_nq_half<512, true, 6, 32>; pl.block_hit = 128; }
            else if (v == V_FUSED_HALF_6_WAVES) { pl.trace = &k_trace_nq_half<512, true, 6, 16>; pl.block_hit = 128; }      // 73 VGPRs: twelve workgroups and 24 waves per CU, as before the LDS overlay
            else if (half_eight && variant_of(p) == V_HALF_8_WAVES_256) { pl.trace = &k_trace_nq_half8<256, true, 16>; pl.block_hit = 128; }      // 9,096 B: eight granules too, the same sixteen workgroups
            else if (half_eight)             { pl.trace = &k_trace_nq_half8<384, true, 16>; pl.block_hit = 128; }      // built without packed f32 operations: 64 VGPRs and no scratch; 384 queue entries: 10,120 B of LDS, eight granules -- sixteen workgroups and 32 waves per CU
            else if (half_tile)              { pl.trace = &k_trace_nq_half<512, true, 7, 16>; pl.block_hit = 128; }      // two waves of 8x4 pixels per tile: 11,144 B of LDS (HalfTileLds) and 72 VGPRs, fourteen workgroups and 28 waves per CU
            else                               pl.trace = &k_trace_nq<false, 512, true, 7, 16>;      // 72 VGPRs, no scratch, 7 waves per SIMD (lane-derived addresses are formed where they are used: lane_again, srt_kernels.h); with 14 spilled registers it was already 3 % ahead of the 6-wave build since the node-major order
        } else if (!count && v == V_COARSE_GRID) {
            // 2 x 2 tiles per workgroup (a quarter of the workgroups for frames that are mostly background).  Measured and NOT
            // shipped: K4 closest hit 0.44 ms against 0.29 with one tile per workgroup, K3 0.22 against 0.10 -- the launch is not
            // dispatch-bound, and a workgroup that walks its live tiles one after the other is a longer tail
            pl.nq_hit = &k_closest_hit_nq<false, 512, 2, 2, true, true>;
            pl.grid_hit = dim3((grid8.x + 1) / 2, (grid8.y + 1) / 2);
        } else if (!count && v == V_ALL_WIDE) {
            pl.nq_hit = &k_closest_hit_nq<false, 512, 2, 2, true, false, true>;
        } else if (!count && v != V_HIT_6_WAVES) {
            // built for 7 waves per SIMD (72 VGPRs, 5 spills; 76 without the bound: 6 waves): a frame of mostly background tiles is a stream
            // of short workgroups, and one more resident per SIMD is worth the spills -- K4 closest hit 0.234 -> 0.223 ms, frame 1.285 -> 1.236
            pl.nq_hit = &k_closest_hit_nq<false, 512, 2, 2, true, false, false, 7>;
        } else {
            NQ_HIT(512, 2, 2, true);
        }
    }
    #undef NQ_HIT
    // stage 2
    if (pk_shadow) {
        // a fixed number of waves pull units (the shadow rays of 64 / n_lights pixels) from the quadrant list: no grid over the image
        const uint64_t max_units = (uint64_t)n_tiles * 4u * 2u * ((L + 7) / 8);
        pl.grid_shadow = dim3((uint32_t)(max_units / 4 + 1 < (uint64_t)f.n_cu * 8 ? max_units / 4 + 1 : (uint64_t)f.n_cu * 8));      // (8 per CU: every wave slot; fewer was measured)
        if (count)                       pl.shadow_pk = &k_shadow_pk<true, true, false>;
        else if (v == V_PK_ENTRY_ORDER)  pl.shadow_pk = &k_shadow_pk<false, true, false, true>;
        else if (v == V_PK_AHEAD)        pl.shadow_pk = &k_shadow_pk<false, true, false, false, 1>;
        else if (v == V_PK_AHEAD_SKIP)   pl.shadow_pk = &k_shadow_pk<false, true, false, false, 2>;
        else if (pl.heavy_steps)         pl.shadow_pk = &k_shadow_pk<false, true, false, false, 0, true>;      // heavy quadrants dealt early (a frame alone on the device)
        else if (v == V_PK_CLOCKS)       pl.shadow_pk = &k_shadow_pk<false, true, false, false, -1>;
        else if (v == V_PK_PLAIN)        pl.shadow_pk = &k_shadow_pk<false, true, false, false, 0>;
        else if (v == V_PK_WINDOWS)      pl.shadow_pk = &k_shadow_pk<false, true, true>;
        else                             pl.shadow_pk = &k_shadow_pk<false, true, false>;
    } else if (L && !fused) {
        // scenes far bigger than an L2 (xcd_rows): whole tile rows per XCD for the shadow rays too
        pl.shadow_xcd_rows = v == V_SHADOW_PLAIN_ROWS ? 0u : pl.xcd_rows;
        if (chunked) pl.l_chunk = L / 4 > 4 ? (L + 3) / 4 : 4;
        pl.grid_shadow = dim3(grid8.x, pl.shadow_xcd_rows ? xcd_pad(grid8.y) : grid8.y, chunked ? (L + pl.l_chunk - 1) / pl.l_chunk : 1);
        if (chunked)                                       pl.shadow_nq = &k_shadow_nq<false, 512, true, 64, 6>;
        else if (count)                                    pl.shadow_nq = &k_shadow_nq<true, 512, false>;
        else if (v == V_NQ_TINY)                           pl.shadow_nq = &k_shadow_nq<false, 160, false>;
        else if (v == V_NQ_TINY_FILTER)                    pl.shadow_nq = &k_shadow_nq<false, 160, true>;
        else if (v == V_NQ_EXACT)                          pl.shadow_nq = &k_shadow_nq<false, 512, false>;
        else if (v == V_ROUND2_FORM || v == V_ALL_NARROW)  pl.shadow_nq = &k_shadow_nq<false, 512, true, 16, 6, false>;
        else                                               pl.shadow_nq = &k_shadow_nq<false, 512, true, 16, 6>;      // 80 VGPRs: six waves per SIMD (86 without the bound: five)
    }
    // stage 3
    if (pl.trace_shade) { std::snprintf(pl.pipeline, sizeof(pl.pipeline), "k_trace_shade_nq"); return pl; }
    if (f.int_shin && v != V_GENERAL_SHADE) pl.shade_tile = &k_shade_tile<1>; else pl.shade_tile = &k_shade_tile<0>;
    // Tile spans: the shipped fused frame only, whole and in the reference's ray form -- the kernels' tile arithmetic under a camera
    // matrix, the XCD-row deal, column tiles and scanline blocks of a split is not the table's, a counting build counts every tile, a
    // supersampled frame moves its rays, and the frames of a batch call keep their one grid.  Not the 8+-sample pipelines: their
    // shadow kernels run between the closest-hit launch and the shading and read the hit id of every tile.
    if (pl.trace && v == V_SHIPPED && !full_grid && !cam && !count && !pl.xcd_rows && !p->block_cols && p->block_stride == 1 && p->block_first == 0 &&
        p->spp == 1 && batch == NOT_BATCHED && f.root_min && wl == p->width && rows == p->height &&
        tile_spans(f.root_min, f.root_max, f.n_objects, p->width, p->height, (int)(-(float)p->width / 2), (int)(-(float)p->height / 2), p->focal, &pl.spans))
    {
        pl.spans.epoch = f.box_epoch;
        if (pl.block_hit == 128) pl.trace_spans = &k_trace_nq_half_spans<512, true, 7, 16>; else pl.trace_spans = &k_trace_nq_spans<512, true, 7, 16>;
        if (pl.trace == &k_trace_nq_half8<384, true, 16>) pl.trace_spans = &k_trace_nq_half8_spans<384, true, 16>;      // the twin of the build chosen above
        if (pl.trace == &k_trace_nq_half8<256, true, 16>) pl.trace_spans = &k_trace_nq_half8_spans<256, true, 16>;
        // One wave per workgroup where it was measured ahead: 1 .. 4 light samples (-3.2 % of the headline step at 1, -2.0 % at 4; level at
        // 5 and 6, +0.5 % at 7 -- longer shadow phases, and the two-wave workgroups stay there).  31 and 32 take it at every count.
        const bool one_wave = pl.trace == &k_trace_nq_half8<384, true, 16> && variant_of(p) != V_HALF_8_TWO_WAVES &&
                              (L <= 4 || variant_of(p) == V_WAVE_8 || variant_of(p) == V_WAVE_8_ADJACENT);
        const bool xcd_pairs = one_wave && variant_of(p) != V_WAVE_8_ADJACENT;      // a tile's halves eight workgroups apart, on one XCD: the order shipped
        if (one_wave) { pl.trace_spans = &k_trace_nq_wave8_spans<384, true, 16, false>; pl.block_hit = 64; }      // 5,056 B of LDS, four granules: thirty-two workgroups of one wave per CU
        if (xcd_pairs) pl.trace_spans = &k_trace_nq_wave8_spans<384, true, 16, true>;
        if (pl.shade_tile == &k_shade_tile<1>) pl.shade_tile_spans = &k_shade_tile_spans<1>; else pl.shade_tile_spans = &k_shade_tile_spans<0>;
        // The whole-frame form (srt_kernels.h, whole_frame_params) where variant 0 names the one-wave workgroups in the shipped order: 1 .. 4
        // light samples under the in-flight hint.  Its kernels hold as constants what the condition above asks of the frame; said once
        // more here, so that a change to that condition cannot launch them on a frame they do not fit.  68 keeps the general frame's kernels.
        if (xcd_pairs && variant_of(p) == V_SHIPPED) {
            const bool whole = !cam && !count && !pl.xcd_rows && !pl.exp && !p->ray_matrix && p->block_cols == 0 && p->block_stride == 1 && p->block_first == 0 &&
                               p->spp == 1 && wl == p->width && rows == p->height;
            if (whole) {
                pl.trace_spans = &k_trace_nq_whole8_spans<384, true, 16, true>;
                if (pl.shade_tile == &k_shade_tile<1>) pl.shade_tile_spans = &k_shade_tile_whole_spans<1>; else pl.shade_tile_spans = &k_shade_tile_whole_spans<0>;
            }
        }
        pl.grid_hit_full = grid8;
        pl.grid_hit = dim3(tile_spans_max_n(pl.spans), pl.spans.n_rows);
        if (xcd_pairs) { pl.grid_hit_full.x = (pl.grid_hit_full.x + 7u) / 8u * 8u; pl.grid_hit.x = (pl.grid_hit.x + 7u) / 8u * 8u; }      // (groups of eight tiles: upper halves, then lower halves)
        if (one_wave) { pl.grid_hit_full.x *= 2u; pl.grid_hit.x *= 2u; }      // two workgroups a tile; the table stays in tiles
    } else {
        pl.spans.on = 0u;
    }
    std::snprintf(pl.pipeline, sizeof(pl.pipeline), "%s%s+k_shade_tile", fused ? "k_trace_nq" : (pk_closest ? "k_closest_hit_pk" : "k_closest_hit_nq"),
                  fused || !L ? "" : (pk_shadow ? "+k_shadow_pk" : "+k_shadow_nq"));
    return pl;
}

// A frame's kernel parameters: geometry and literals from the caller's params, the rest from the plan.
struct FrameParams {
    DevParams hit, shadow, shade;      // per stage: the same but for xcd_rows (shadow) and shadow_px_major (shade)
    void sub_pixel(float x, float y) { hit.sub_x = shadow.sub_x = shade.sub_x = x; hit.sub_y = shadow.sub_y = shade.sub_y = y; }
};
static FrameParams dev_params(const srt_scene* s, const srt_params* p, const FramePlan& pl) {
    DevParams dp;
    dp.smooth = (p->flags & SRT_FLAG_SMOOTH_NORMALS) ? 1u : 0u; dp.shadow_px_major = 0u;
    dp.cam = p->ray_matrix ? 1u : 0u;
    for (int c = 0; c < 4; c++) for (int r3 = 0; r3 < 3; r3++) dp.cm[c * 3 + r3] = p->ray_matrix ? p->ray_matrix[c * 4 + r3] : 0.0f;
    dp.W = srt_cols_owned(p); dp.Wimg = p->width; dp.col_block = p->block_cols; dp.H = p->height; dp.rows = srt_rows_owned(p);
    dp.block_rows = p->block_rows; dp.block_first = p->block_first; dp.block_stride = p->block_stride;
    dp.i0 = (int)(-(float)p->width / 2); dp.j0 = (int)(-(float)p->height / 2);       // :511,513
    dp.sub_x = 0.0f; dp.sub_y = 0.0f;                                                 // rayXY = (0, 0), :507,514-515
    dp.focal = p->focal; dp.n_lights = p->n_lights; dp.lights = s->d_lights;
    dp.shadow_div = p->shadow_div; dp.reinhard = p->reinhard; dp.gamma = p->gamma;
    dp.bg = (uint32_t)p->background[0] | ((uint32_t)p->background[1] << 8) | ((uint32_t)p->background[2] << 16);
    dp.xcd_rows = pl.xcd_rows; dp.exp = pl.exp; dp.heavy_steps = pl.heavy_steps; dp.pk_units = pl.pk_units; dp.pk_take = pl.pk_take;
    FrameParams fp{dp, dp, dp};
    fp.shadow.xcd_rows = pl.shadow_xcd_rows; fp.shade.shadow_px_major = pl.shadow_px_major;
    return fp;
}

// Frames whose launches srt_render_device_batch holds back to issue them as one grid (k_trace_nq_batch + k_shade_tile_batch).
struct BatchCollector {
    std::vector<FrameItem> items;        // frames of the fused pipeline (1..7 light samples): k_trace_nq_batch + k_shade_tile_batch
    std::vector<FrameItem> items_pk;     // frames of the 8+-sample pipeline: k_closest_hit_nq_batch + k_shadow_pk_batch + k_shade_tile_batch
    uint32_t wl = 0, rows = 0, max_lights = 0;      // every held frame writes the same local width and row count: one grid fits all
    bool fits(uint32_t w, uint32_t r) const { return (items.empty() && items_pk.empty()) || (w == wl && r == rows); }
};

// One pass of a plan over this call's pixels: closest hit (+ shadow rays) and shading, the event records between them.
static int launch_stages(srt_scene* s, const FramePlan& pl, const FrameParams& fp, hipStream_t stream, int32_t* o_hit, float* o_t, float* o_lin, uint8_t* o_rgb8, unsigned long long* ctr, unsigned long long* zero_next, hipEvent_t* ev) {
    const dim3 block(256), block_hit(pl.block_hit);
    uint32_t* const ql = pl.quadrants_consumed ? s->ws_qlist.p : nullptr, * const ql_cnt = pl.quadrants_consumed ? s->d_qcount.p : nullptr;
    // Tile spans in a launch that is being captured into a graph: the replay may come after the boxes have changed, so the launch keeps
    // the whole grid and the kernels cull only while the records' epoch word is the table's (srt_kernels.h, trace_nq_body)
    const TileSpans* spans = &pl.spans; TileSpans spans_whole; const uint32_t* box_epoch = nullptr; dim3 grid_hit = pl.grid_hit;
    if (pl.trace_spans) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }      // (not known: as if it were)
        if (cs != hipStreamCaptureStatusNone) {
            spans_whole = tile_spans_from_row_zero(pl.spans); spans = &spans_whole;
            box_epoch = s->rec->d_box_epoch; grid_hit = pl.grid_hit_full;
        }
    }
    if (pl.ref_hit)          hipLaunchKernelGGL(pl.ref_hit, pl.grid_hit, block, 0, stream, s->dev, fp.hit, o_hit, o_t, ctr);
    else if (pl.q_hit)       hipLaunchKernelGGL(pl.q_hit, pl.grid_hit, block, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, ctr);
    else if (pl.nq_hit)      hipLaunchKernelGGL(pl.nq_hit, pl.grid_hit, block, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, ctr, ql_cnt, ql, s->qcap);
    else if (pl.pk_hit)      hipLaunchKernelGGL(pl.pk_hit, pl.grid_hit, block, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, ql_cnt, ql, s->qcap, ctr);
    else if (pl.trace_spans) hipLaunchKernelGGL(pl.trace_spans, grid_hit, block_hit, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, s->ws_shadow, ctr, box_epoch, *spans);
    else if (pl.trace)       hipLaunchKernelGGL(pl.trace, pl.grid_hit, block_hit, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, s->ws_shadow, ctr);
    else                     hipLaunchKernelGGL(pl.trace_shade, pl.grid_hit, block, 0, stream, s->dev, fp.hit, o_hit, o_t, o_lin, o_rgb8, ctr, zero_next, s->d_qcount);
    HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev[1], stream));
    if (pl.shadow_pk)        hipLaunchKernelGGL(pl.shadow_pk, pl.grid_shadow, block, 0, stream, s->dev, fp.hit, o_hit, o_t, s->d_qcount, s->ws_qlist, s->qcap, s->ws_shadow, ctr);
    else if (pl.shadow_nq)   hipLaunchKernelGGL(pl.shadow_nq, pl.grid_shadow, block, 0, stream, s->dev, fp.shadow, o_hit, o_t, s->ws_shadow, ctr, pl.l_chunk);
    if (pl.shadow_pk || pl.shadow_nq) HIP_TRY(hipGetLastError());
    if (ev) HIP_TRY(hipEventRecord(ev[2], stream));
    if (pl.ref_shade)        hipLaunchKernelGGL(pl.ref_shade, pl.grid_shade, block, 0, stream, s->dev, fp.shade, o_hit, o_t, o_lin, o_rgb8, ctr, zero_next);
    else if (pl.shade_tile_spans) hipLaunchKernelGGL(pl.shade_tile_spans, pl.grid_shade, block, 0, stream, s->dev, fp.shade, o_hit, o_t, s->ws_shadow, o_lin, o_rgb8, zero_next, s->d_qcount, ctr, box_epoch, *spans);
    else if (pl.shade_tile)  hipLaunchKernelGGL(pl.shade_tile, pl.grid_shade, block, 0, stream, s->dev, fp.shade, o_hit, o_t, s->ws_shadow, o_lin, o_rgb8, zero_next, s->d_qcount, ctr);
    if (pl.ref_shade || pl.shade_tile) HIP_TRY(hipGetLastError());
    std::snprintf(s->pipeline, sizeof(s->pipeline), "%s", pl.pipeline);
    return SRT_OK;
}

static int render_device_impl(srt_scene* s, const srt_params* p, void* stream_, int32_t* d_hit_id, float* d_t,
                              float* d_rgb_linear, uint8_t* d_rgb8, BatchCollector* bc = nullptr) {
    if (!s) return SRT_ERR_ARG;
    const SceneFacts facts = scene_facts(s);
    SRT_TRY(check_frame(facts, p));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipSetDevice(s->device));
    const uint32_t rows = srt_rows_owned(p), wl = srt_cols_owned(p);      // wl: width of the rows this call writes
    if (!rows) {                              // nothing to launch; work of an earlier render stays pending
        if (!s->pending) std::memset(&s->last, 0, sizeof(s->last));
        return SRT_OK;
    }
    const FramePlan plan = plan_frame(facts, p, !bc ? NOT_BATCHED : bc->fits(wl, rows) ? BATCH_FITS : BATCH_OTHER_SIZE);
    std::memset(&s->last, 0, sizeof(s->last));
    s->last.rows = rows;
    s->last.primary_rays = pixels_owned(p);
    const size_t pixels = (size_t)wl * rows;
    // workspace for hit ids / t when the caller does not want them (the shade kernel does)
    if (!d_hit_id || !d_t) SRT_TRY(grow(s, pixels, s->ws_hit, s->ws_t));
    if (!d_hit_id) d_hit_id = s->ws_hit; if (!d_t) d_t = s->ws_t;
    if (p->n_lights > s->d_lights.cap || p->n_lights > s->h_lights.cap) {
        s->lights_valid = 0;               // new buffers: nothing of the old contents is on the device
        SRT_TRY(grow(s, p->n_lights, s->d_lights, s->h_lights));
    }
    const size_t light_bytes = (size_t)p->n_lights * 3 * sizeof(float);
    if (p->n_lights && !(s->lights_valid == p->n_lights && std::memcmp(s->h_lights, p->light_pos, light_bytes) == 0)) {
        HIP_TRY(wait_idle(s));     // staging buffer still in flight
        std::memcpy(s->h_lights, p->light_pos, light_bytes);
        HIP_TRY(hipMemcpyAsync(s->d_lights, s->h_lights, light_bytes, hipMemcpyHostToDevice, stream));
        s->lights_valid = p->n_lights;
    }
    // Work / hit counters: two sets used alternately.  The last kernel of a render zeroes the set the NEXT
    // render will use, so no memset or copy is enqueued per frame; srt_sync reads the last set.
    unsigned long long* ctr = s->d_counters + (s->render_seq & 1) * NCTR;
    unsigned long long* ctr_next = s->d_counters + ((s->render_seq + 1) & 1) * NCTR;
    // a render that failed half-way may have left either set dirty: clear both before the next one
    if (s->ctr_dirty) {
        HIP_TRY(hipMemsetAsync(s->d_counters, 0, 2 * NCTR * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(s->d_qcount, 0, QL_COUNTERS * QL_STRIDE * sizeof(uint32_t), stream));
    }
    s->ctr_dirty = true;
    // a counting run must not inherit whatever replayed graphs left in the set (their frames use fixed sets)
    if (p->flags & SRT_FLAG_COUNT_WORK) HIP_TRY(hipMemsetAsync(ctr, 0, NCTR * sizeof(unsigned long long), stream));

    // the workspaces the plan needs: all of them before the first launch
    if (plan.shadow_words) SRT_TRY(grow(s, plan.shadow_words, s->ws_shadow));
    if (s->qcap < plan.qcap_need) {
        // per shard entry three words: two for the entry, and behind the lists one word per quadrant, the cost map the shadow kernel leaves
        // for the next frame's list -- which starts empty
        s->qcap = 0;
        SRT_TRY(grow(s, (size_t)QL_SHARDS * plan.qcap_need, s->ws_qlist));
        HIP_TRY(hipMemset(s->ws_qlist + (size_t)QL_SHARDS * plan.qcap_need * 2, 0, (size_t)QL_SHARDS * plan.qcap_need * sizeof(uint32_t)));
        s->qcap = plan.qcap_need;
    }
    const uint32_t spp = p->spp;
    if (spp > 1) SRT_TRY(grow(s, pixels, s->ws_acc, s->ws_sub, s->ws_sub_hit, s->ws_sub_t));      // supersampling extension: accumulation buffers
    FrameParams fp = dev_params(s, p, plan);      // (after the lights' buffer has its size)

    // SRT_FLAG_NO_TIMING: no event records (a caller capturing the launches into a hipGraph)
    hipEvent_t* ev = ((p->flags & SRT_FLAG_NO_TIMING) || bc) ? nullptr : s->ev[s->ring_count % RING];      // (a batch has no per-frame times)
    if (ev && !ev[0]) for (int i = 0; i < 4; i++) HIP_TRY(hipEventCreate(&ev[i]));      // a ring slot's events are made on first use
    if (ev) HIP_TRY(hipEventRecord(ev[0], stream));
    if (plan.hold != HOLD_NONE) {
        // the batch call launches this frame with the others of its class; the shading stage's parameters are the whole frame's
        if (bc->items.empty() && bc->items_pk.empty()) { bc->wl = wl; bc->rows = rows; }
        const FrameItem it{s->dev, fp.shade, d_hit_id, d_t, d_rgb_linear, d_rgb8, s->ws_shadow, ctr, ctr_next, s->d_qcount,
                           plan.hold == HOLD_PK ? s->ws_qlist.p : nullptr, plan.hold == HOLD_PK ? s->qcap : 0u, 0u};
        (plan.hold == HOLD_PK ? bc->items_pk : bc->items).push_back(it);
        if (plan.hold == HOLD_PK && p->n_lights > bc->max_lights) bc->max_lights = p->n_lights;
        std::snprintf(s->pipeline, sizeof(s->pipeline), "%s", plan.pipeline);
    } else if (spp == 1) {
        SRT_TRY(launch_stages(s, plan, fp, stream, d_hit_id, d_t, d_rgb_linear, d_rgb8, ctr, ctr_next, ev));
    } else {
        // Supersampling (extension): n x n regular sub-pixel grid, offsets (k+0.5)/n - 0.5 added to
        // dir.xy; the pre-tone-map sums are added in sub-sample order, divided by spp, then tone-mapped once.
        // hit_id / t report sub-sample 0.  Per-kernel times are those of the last sub-frame.
        const uint32_t n = (uint32_t)std::lround(std::sqrt((double)spp)), gq = (uint32_t)((pixels * 3 + 255) / 256);
        const dim3 block(256); const DevParams dp = fp.hit;
        for (uint32_t k = 0; k < spp; k++) {
            fp.sub_pixel(((float)(k % n) + 0.5f) / (float)n - 0.5f, ((float)(k / n) + 0.5f) / (float)n - 0.5f);
            SRT_TRY(launch_stages(s, plan, fp, stream, k == 0 ? d_hit_id : s->ws_sub_hit.p, k == 0 ? d_t : s->ws_sub_t.p, s->ws_sub, nullptr, ctr, nullptr,
                                  (k == spp - 1) ? ev : nullptr));
            hipLaunchKernelGGL(k_accumulate, dim3(gq), block, 0, stream, dp, s->ws_acc, s->ws_sub, (uint32_t)(pixels * 3), k == 0 ? 1 : 0);      // (< 2^32: check_frame)
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_resolve, dim3((uint32_t)((pixels + 255) / 256)), block, 0, stream, dp, s->ws_acc, (float)spp, (uint32_t)pixels,
                           d_rgb_linear, d_rgb8, ctr_next);
        HIP_TRY(hipGetLastError());
    }
    if (ev) {
        HIP_TRY(hipEventRecord(ev[3], stream));
        s->last_done = ev[3];
        s->ring_count++;
    } else {
        s->last_done = nullptr;
    }
    s->render_seq++;                          // the sets only swap once every launch of this render is enqueued
    s->d_ctr_last = ctr;
    s->ctr_dirty = false;
    s->last_stream = stream;
    s->pending = true;
    s->last.primary_rays = pixels_owned(p) * spp;
    s->last.shadow_rays = p->n_lights;     // multiplied by hit count in srt_sync
    return SRT_OK;
}

int srt_render_device(srt_scene* s, const srt_params* p, void* stream, int32_t* d_hit_id, float* d_t, float* d_rgb_linear, uint8_t* d_rgb8) {
    return guarded([&] { return render_device_impl(s, p, stream, d_hit_id, d_t, d_rgb_linear, d_rgb8); });
}

// The frames of a step in as few launches as their arguments fit (srt.h).  Every frame goes through render_device_impl -- the same
// checks, workspaces, light upload and counter sets as a single render; frames that plan_frame puts into one of the two held classes
// at one size are held back and launched together, the others (another pipeline, counting build, supersampling, a different size)
// are launched as they come.
static int render_device_batch_impl(uint32_t n, srt_scene* const* scenes, const srt_params* params, void* stream_,
                                    int32_t* const* d_hit_id, float* const* d_t, float* const* d_rgb_linear, uint8_t* const* d_rgb8) {
    if (!n) return SRT_OK;
    if (!scenes || !params) return SRT_ERR_ARG;
    if (n > 65535u) return SRT_ERR_LIMIT;                     // the frame is a grid dimension
    for (uint32_t i = 0; i < n; i++) {
        if (!scenes[i] || scenes[i]->device != scenes[0]->device) return SRT_ERR_ARG;
        for (uint32_t k = 0; k < i; k++) if (scenes[k] == scenes[i]) return SRT_ERR_ARG;      // a handle's workspace serves one frame at a time
        SRT_TRY(check_frame(scene_facts(scenes[i]), &params[i]));                              // nothing is enqueued if any frame is malformed
    }
    hipStream_t stream = (hipStream_t)stream_;
    bool batch_int_shin = true;                               // the specialised shading kernel only if every scene of the batch qualifies
    for (uint32_t i = 0; i < n; i++) batch_int_shin = batch_int_shin && scenes[i]->rec->int_shin;
    BatchCollector bc;
    for (uint32_t i = 0; i < n; i++) {
        const int rc = render_device_impl(scenes[i], &params[i], stream_, d_hit_id ? d_hit_id[i] : nullptr, d_t ? d_t[i] : nullptr,
                                          d_rgb_linear ? d_rgb_linear[i] : nullptr, d_rgb8 ? d_rgb8[i] : nullptr, &bc);
        if (rc != SRT_OK) { for (uint32_t k = 0; k <= i; k++) scenes[k]->ctr_dirty = true; return rc; }   // held frames are dropped: their counter sets may be half-used
    }
    // The held frames, class by class in the launches of their class, FRAME_TAB_MAX at a time: their arguments by value in the launch
    // (srt_kernels.h: FrameTab)
    int rc = SRT_OK;
    const dim3 block(256), g8((bc.wl + 7) / 8, (bc.rows + 7) / 8), g16((bc.wl + 15) / 16, (bc.rows + 15) / 16);
    for (const Hold cls : {HOLD_PK, HOLD_FUSED}) {
        const std::vector<FrameItem>& items = cls == HOLD_PK ? bc.items_pk : bc.items;
        for (size_t first = 0; first < items.size() && rc == SRT_OK; first += FRAME_TAB_MAX) {
            const uint32_t held = (uint32_t)std::min<size_t>(FRAME_TAB_MAX, items.size() - first);
            FrameTab tab;
            std::memset(&tab, 0, sizeof(tab));
            std::memcpy(tab.it, items.data() + first, held * sizeof(FrameItem));
            // grid = (tiles per row, frames, tile rows): the same tile row of all the frames is in flight together (srt_kernels.h)
            if (cls == HOLD_PK) {
                const uint64_t n_tiles = (uint64_t)g8.x * g8.y, max_units = n_tiles * 4u * 2u * ((bc.max_lights + 7) / 8);
                const uint64_t wgs_all = (uint64_t)scenes[0]->n_cu * 8;         // the chip's worth of waves, shared by the frames
                uint32_t wgs = (uint32_t)((wgs_all + held - 1) / held);
                if ((uint64_t)wgs > max_units / 4 + 1) wgs = (uint32_t)(max_units / 4 + 1);
                hipLaunchKernelGGL((k_closest_hit_nq_batch<512, true, true>), dim3(g8.x, held, g8.y), block, 0, stream, tab);
                hipLaunchKernelGGL((k_shadow_pk_batch<true>), dim3(wgs, held), block, 0, stream, tab);
            }
            decltype(&k_shade_tile_batch<0>) shade;
            if (batch_int_shin) shade = &k_shade_tile_batch<1>; else shade = &k_shade_tile_batch<0>;
            if (cls == HOLD_FUSED) hipLaunchKernelGGL((k_trace_nq_batch<512, true, 7, 16, true>), dim3(g8.x, held, g8.y), block, 0, stream, tab);
            hipLaunchKernelGGL(shade, dim3(g16.x, g16.y, held), block, 0, stream, tab);
            if (hipGetLastError() != hipSuccess) rc = SRT_ERR_DEVICE;
        }
    }
    if (rc != SRT_OK) for (uint32_t k = 0; k < n; k++) scenes[k]->ctr_dirty = true;       // the set the shading would have zeroed
    return rc;
}

int srt_render_device_batch(uint32_t n, srt_scene* const* scenes, const srt_params* params, void* stream,
                            int32_t* const* d_hit_id, float* const* d_t, float* const* d_rgb_linear, uint8_t* const* d_rgb8) {
    return guarded([&] { return render_device_batch_impl(n, scenes, params, stream, d_hit_id, d_t, d_rgb_linear, d_rgb8); });
}

int srt_sync(srt_scene* s, srt_stats* stats) {
    if (!s) return SRT_ERR_ARG;
    if (s->pending) {
        HIP_TRY(hipSetDevice(s->device));
        HIP_TRY(hipStreamSynchronize(s->last_stream));
        const uint32_t n = s->ring_count < RING ? s->ring_count : RING;
        double a = 0., b = 0., c = 0., sh = 0.;
        if (n == 0) { s->last.ms_primary = s->last.ms_shadow = s->last.ms_shade = s->last.ms_total = 0.f; }
        for (uint32_t k = 0; k < n; k++) {
            hipEvent_t* ev = s->ev[(s->ring_count - 1 - k) % RING];
            float x = 0.f, y = 0.f, z = 0.f, w = 0.f;
            HIP_TRY(hipEventElapsedTime(&x, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&y, ev[1], ev[2]));
            HIP_TRY(hipEventElapsedTime(&w, ev[2], ev[3]));
            HIP_TRY(hipEventElapsedTime(&z, ev[0], ev[3]));
            a += x; b += y; c += z; sh += w;
        }
        if (n) {
            s->last.ms_primary = (float)(a / n); s->last.ms_shadow = (float)(b / n); s->last.ms_shade = (float)(sh / n);
            s->last.ms_total = (float)(c / n);
        }
        s->last.launches = n;
        s->ring_count = 0;
        HIP_TRY(hipMemcpy(s->h_counters, s->d_ctr_last, NCTR * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        unsigned long long hits = 0;
        for (int k = 0; k < 64; k++) hits += s->h_counters[8 + 8 * k];
        s->last.hit_rays = hits;
        s->last.shadow_rays = s->last.shadow_rays * hits;
        s->last.node_tests_primary = s->h_counters[1];
        s->last.tri_tests_primary = s->h_counters[2];
        s->last.node_tests_shadow = s->h_counters[3];
        s->last.tri_tests_shadow = s->h_counters[4];
        if (std::getenv("SRT_DIAG_COUNTERS"))      // counting build of the packet shadow kernel: shape of its walks
            std::fprintf(stderr, "srt diag: walks %llu steps %llu node-window loads %llu triangle iterations %llu | lane tests: nodes %llu tris %llu\n",
                         s->h_counters[0], s->h_counters[5], s->h_counters[6], s->h_counters[7], s->h_counters[3], s->h_counters[4]);
        if (std::getenv("SRT_DIAG_COUNTERS") && s->h_counters[17]) {
            const double span = (double)(s->h_counters[10] - ((1ull << 62) - s->h_counters[11])) * 0.01;      // us
            std::fprintf(stderr, "srt diag: packet shadow kernel: %llu waves, first start to last end %.1f us, mean wave busy %.1f us (%.0f %%), longest walk %.1f us, "
                                 "most steps in a walk %llu, walks of > 256 steps %llu (mean %.1f us)\n",
                         s->h_counters[17], span, (double)s->h_counters[9] * 0.01 / (double)s->h_counters[17],
                         span > 0 ? 100.0 * (double)s->h_counters[9] * 0.01 / (double)s->h_counters[17] / span : 0.0, (double)s->h_counters[12] * 0.01,
                         s->h_counters[13], s->h_counters[14], s->h_counters[14] ? (double)s->h_counters[15] * 0.01 / (double)s->h_counters[14] : 0.0);
            std::fprintf(stderr, "srt diag: walks of 100 us and more: %llu\n", s->h_counters[18]);
        }
        s->pending = false;
    }
    if (stats) *stats = s->last;
    return SRT_OK;
}

static int render_async_impl(srt_scene* s, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8, bool wait, srt_stats* stats) {
    if (!s) return SRT_ERR_ARG;
    int rc = check_frame(scene_facts(s), p);
    if (rc != SRT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st;
    rc = own_stream(s, &st);
    if (rc != SRT_OK) return rc;
    const uint32_t rows = srt_rows_owned(p);
    const size_t pixels = (size_t)srt_cols_owned(p) * rows;
    SRT_TRY(grow(s, pixels, s->ws_lin, s->ws_rgb8));
    rc = render_device_impl(s, p, st, nullptr, nullptr, rgb_linear ? s->ws_lin : nullptr, rgb8 ? s->ws_rgb8 : nullptr);
    if (rc != SRT_OK) return rc;
    if (wait) {        // srt_render: the caller's buffers are ordinary (pageable) memory as a rule, where a synchronous copy is the fast one
        rc = srt_sync(s, stats);
        if (rc != SRT_OK) return rc;
        if (pixels) {
            if (hit_id) HIP_TRY(hipMemcpy(hit_id, s->ws_hit, pixels * sizeof(int32_t), hipMemcpyDeviceToHost));
            if (t) HIP_TRY(hipMemcpy(t, s->ws_t, pixels * sizeof(float), hipMemcpyDeviceToHost));
            if (rgb_linear) HIP_TRY(hipMemcpy(rgb_linear, s->ws_lin, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
            if (rgb8) HIP_TRY(hipMemcpy(rgb8, s->ws_rgb8, pixels * 3, hipMemcpyDeviceToHost));
        }
        return SRT_OK;
    }
    if (pixels) {      // device -> host behind the kernels; truly asynchronous into pinned memory (srt_host_alloc)
        if (hit_id) HIP_TRY(hipMemcpyAsync(hit_id, s->ws_hit, pixels * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        if (t) HIP_TRY(hipMemcpyAsync(t, s->ws_t, pixels * sizeof(float), hipMemcpyDeviceToHost, st));
        if (rgb_linear) HIP_TRY(hipMemcpyAsync(rgb_linear, s->ws_lin, pixels * 3 * sizeof(float), hipMemcpyDeviceToHost, st));
        if (rgb8) HIP_TRY(hipMemcpyAsync(rgb8, s->ws_rgb8, pixels * 3, hipMemcpyDeviceToHost, st));
    }
    return SRT_OK;
}

int srt_render_async(srt_scene* s, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8) {
    return guarded([&] { return render_async_impl(s, p, hit_id, t, rgb_linear, rgb8, false, nullptr); });
}

int srt_render(srt_scene* s, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8, srt_stats* stats) {
    return guarded([&] { return render_async_impl(s, p, hit_id, t, rgb_linear, rgb8, true, stats); });
}

// ---- ray queries (include/srt.h, RAY QUERIES; kernels in srt_query.h) ------------------------------------------------------------
// The device entry points enqueue and return: the light table when it changed (srt_shade_rays), a memset of the private counter set when it
// is used, one launch.  They touch neither the render counters nor the state srt_sync reports from (pending, the event ring, the pipeline
// string).  Every check runs before anything is touched.
static int check_query(const srt_scene* s, uint32_t n, const float* rays, uint32_t flags) {
    if (!s || (n && !rays) || (flags & ~(uint32_t)SRT_FLAG_COUNT_WORK)) return SRT_ERR_ARG;
    return SRT_OK;
}
static int check_shade(const srt_scene* s, uint32_t n, const float* rays, const srt_params* p) {
    if (!s || !p || (n && !rays) || (p->n_lights && !p->light_pos)) return SRT_ERR_ARG;
    if (p->flags & ~(uint32_t)(SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS)) return SRT_ERR_ARG;
    if ((p->flags & SRT_FLAG_SMOOTH_NORMALS) && !s->dev.tri_normals) return SRT_ERR_ARG;      // needs vertex normals, as check_frame
    if ((uint64_t)n * (p->n_lights ? p->n_lights : 1) >= (1ull << 32)) return SRT_ERR_LIMIT;
    return SRT_OK;
}

static inline uint32_t rays_wide(const float* d_rays) { return ((uintptr_t)d_rays & 7u) == 0 ? 1u : 0u; }      // srt_query.h load_ray
static inline QueryRange query_range(const float* d_t_range) { return QueryRange{ d_t_range, rays_wide(d_t_range) }; }      // srt_query.h load_range

// The light table of a query, as a render sends its own: through a pinned copy, again only when the bytes differ from what the device
// holds.  The upload is ordered on `stream`; a later call with the same table on ANOTHER stream is ordered behind it by the event.
static int query_lights(srt_scene* s, const srt_params* p, hipStream_t stream) {
    const uint32_t L = p->n_lights;
    if (!L) return SRT_OK;
    const size_t bytes = (size_t)L * 3 * sizeof(float);
    if (s->qlights_valid == L && L <= s->h_qlights.cap && std::memcmp(s->h_qlights, p->light_pos, bytes) == 0) {
        if (!s->qlights_settled && stream != s->qlights_stream) {
            // has the upload arrived?  Then it never needs waiting for again; else this stream waits behind it
            const hipError_t e = hipEventQuery(s->qlights_sent);
            if (e == hipSuccess) s->qlights_settled = true;
            else if (e == hipErrorNotReady) HIP_TRY(hipStreamWaitEvent(stream, s->qlights_sent, 0));
            else HIP_TRY(e);
        }
        return SRT_OK;
    }
    if (!s->qlights_sent) HIP_TRY(hipEventCreateWithFlags(&s->qlights_sent.e, hipEventDisableTiming));
    else if (!s->qlights_settled) HIP_TRY(hipEventSynchronize(s->qlights_sent));      // the pinned copy may still be read
    s->qlights_settled = true;
    s->qlights_valid = 0;
    if (L > s->d_qlights.cap) HIP_TRY(s->d_qlights.reserve(L));      // (hipFree waits for whatever still reads the old block)
    HIP_TRY(s->h_qlights.reserve(L));
    std::memcpy(s->h_qlights, p->light_pos, bytes);
    HIP_TRY(hipMemcpyAsync(s->d_qlights, s->h_qlights, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(s->qlights_sent, stream));
    s->qlights_valid = L; s->qlights_stream = stream; s->qlights_settled = false;
    return SRT_OK;
}

// What every device entry point does before its launch: the device, the stream (the scene's own where the caller names none), the light
// table of a shading query, the private counter set -- cleared on that stream when the call uses it -- and the grid of one lane per ray.
struct QueryLaunch { hipStream_t stream; unsigned long long* ctr; dim3 grid; };
static int query_prologue(srt_scene* s, uint32_t n, hipStream_t stream, const srt_params* shade, bool use_counters, QueryLaunch* q) {
    HIP_TRY(hipSetDevice(s->device));
    if (!stream) SRT_TRY(own_stream(s, &stream));
    if (shade) SRT_TRY(query_lights(s, shade, stream));
    q->stream = stream;
    q->ctr = use_counters ? s->d_qctr.p : nullptr;
    if (q->ctr) HIP_TRY(hipMemsetAsync(q->ctr, 0, NCTR * sizeof(unsigned long long), stream));
    q->grid = dim3((uint32_t)(((uint64_t)n + 255u) / 256u));
    return SRT_OK;
}

extern "C++" {
// Which build of a kernel family a call launches.  BUILDS_n(family) lists the 2^n builds of a family of n flags in the order of build_index:
// bit k of the index is the family's template argument k, the first argument being bit 0.  What follows the family's name goes behind
// the flags (the slot count of k_query_multi).  A table is a std::array over such a list, so a family is named once where it is chosen from.
#define BUILDS_1(K, ...) &K<false __VA_ARGS__>, &K<true __VA_ARGS__>
#define BUILDS_2(K, ...) BUILDS_1(K, , false __VA_ARGS__), BUILDS_1(K, , true __VA_ARGS__)
#define BUILDS_3(K, ...) BUILDS_2(K, , false __VA_ARGS__), BUILDS_2(K, , true __VA_ARGS__)
#define BUILDS_4(K, ...) BUILDS_3(K, , false __VA_ARGS__), BUILDS_3(K, , true __VA_ARGS__)
template <typename... B>
static inline size_t build_index(B... flag) {      // the flags in the order of the family's template arguments; a pointer: whether it is there
    size_t i = 0, bit = 1;
    ((i |= flag ? bit : 0, bit <<= 1), ...);
    return i;
}

// One launch of workgroups of 256 lanes, and whether it was taken
template <typename... P, typename... A>
static int launch_query(void (*kernel)(P...), dim3 grid, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, args...);
    HIP_TRY(hipGetLastError());
    return SRT_OK;
}
}      // extern "C++"

// The masks of a masked call as its kernels take them: the scene's table as it stands in the records now, the call's per-ray masks, or
// the three masks per ray kind.
static inline QueryMask query_mask(const srt_scene* s, const uint32_t* d_ray_mask) { return QueryMask{ s->rec->d_obj_mask, d_ray_mask, ~0u, ~0u, ~0u }; }
static inline QueryMask query_mask(const srt_scene* s, const srt_visibility* v) { return QueryMask{ s->rec->d_obj_mask, nullptr, v->primary, v->bounce, v->shadow }; }
// Whether a closest-hit or occlusion call is srt_*_masked, and its per-ray masks (NULL: all ones): host words in a host form, device words
// in a device form.
struct RayMask { bool masked = false; const uint32_t* words = nullptr; };

// d_t_range: the rays' t intervals (srt_*_range), or null: nothing bounds t, and the kernels are the ones without the interval.
// count_hits: the host entry point wants hit_rays also without SRT_FLAG_COUNT_WORK
// mask: a call that is not masked launches k_query_closest; a masked one the MASK build of the same choice of COUNT and BARY
static int trace_rays_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t flags, hipStream_t stream, int32_t* d_hit_id,
                                  float* d_t, float* d_bary, bool count_hits, const RayMask& mask) {
    SRT_TRY(check_query(s, n, d_rays, flags));
    if (!n) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { BUILDS_3(k_query_closest) };
    static const std::array masked_builds = { BUILDS_2(k_query_closest_masked) };
    if (mask.masked)
        return launch_query(masked_builds[build_index(count, d_bary)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_hit_id, d_t, d_bary, q.ctr,
                            query_range(d_t_range), query_mask(s, mask.words));
    return launch_query(builds[build_index(count, d_bary, d_t_range)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_hit_id, d_t, d_bary, q.ctr,
                        query_range(d_t_range));
}

// srt_trace_rays_multi: the k nearest hits per ray in one walk (k_query_multi); the build reserves 4, 8 or 16 slots a ray
static int check_multi(const srt_scene* s, uint32_t n, const float* rays, uint32_t k, uint32_t flags) {
    SRT_TRY(check_query(s, n, rays, flags));
    if (k == 0) return SRT_ERR_ARG;
    if (k > SRT_MULTI_HIT_MAX) return SRT_ERR_LIMIT;
    return SRT_OK;
}
static int trace_rays_multi_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t k, uint32_t flags, hipStream_t stream,
                                        uint32_t* d_n_hits, int32_t* d_hit_id, float* d_t, float* d_bary, bool count_hits) {
    SRT_TRY(check_multi(s, n, d_rays, k, flags));
    if (!n || (!count_hits && !d_n_hits && !d_hit_id && !d_t && !d_bary)) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { std::array{ BUILDS_2(k_query_multi, , 4) }, std::array{ BUILDS_2(k_query_multi, , 8) }, std::array{ BUILDS_2(k_query_multi, , 16) } };
    static_assert(SRT_MULTI_HIT_MAX == 16, "the largest bucket holds SRT_MULTI_HIT_MAX slots");
    const int bucket = k <= 4 ? 0 : k <= 8 ? 1 : 2;
    return launch_query(builds[bucket][build_index(count, d_bary)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), query_range(d_t_range), k, d_n_hits,
                        d_hit_id, d_t, d_bary, q.ctr);
}

// mask: a call that is not masked launches k_query_any, with or without the interval; a masked one k_query_any_masked
static int occluded_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const int32_t* d_skip_obj, hipStream_t stream,
                                uint8_t* d_occluded, const RayMask& mask) {
    SRT_TRY(check_query(s, n, d_rays, 0));
    if (!n || !d_occluded) return SRT_OK;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, false, &q));
    static const std::array builds = { BUILDS_1(k_query_any) };
    if (mask.masked)
        return launch_query(&k_query_any_masked, q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_skip_obj, d_occluded, query_range(d_t_range),
                            query_mask(s, mask.words));
    return launch_query(builds[build_index(d_t_range)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_skip_obj, d_occluded, query_range(d_t_range));
}

// srt_closest_points: the nearest triangle within a radius per point, one launch (k_query_points).  A call with a mask array launches the
// MASK build; one without launches the build that reads neither the array nor the scene's table.
// count_hits: the host entry point wants hit_rays also without SRT_FLAG_COUNT_WORK
static inline bool points_wanted(const srt_point_out* o) { return o->tri || o->dist2 || o->point || o->vw || o->region; }
// nearest: srt_nearest_points (include/srt_nearest.h) -- the same call with k_query_nearest, whose bound shrinks
static int closest_points_device_impl(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t flags,
                                      hipStream_t stream, const srt_point_out* out, bool count_hits, bool nearest = false) {
    SRT_TRY(check_query(s, n, d_points, flags));
    if (!out) return SRT_ERR_ARG;
    if (!n || (!count_hits && !points_wanted(out))) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { BUILDS_2(k_query_points) };
    static const std::array shrinking = { BUILDS_2(k_query_nearest) };
    return launch_query((nearest ? shrinking : builds)[build_index(count, d_point_mask)], q.grid, q.stream, s->dev, n, d_points, d_radius, *out, q.ctr, query_mask(s, d_point_mask));
}

// srt_closest_points_multi / srt_nearest_points_multi (include/srt_points_multi.h): the k nearest triangles per point in one walk, one
// launch (k_query_points_multi); the build reserves 4, 8 or 16 slots a point, as trace_rays_multi_device_impl picks them.
// nearest: the walk prunes by the k-th best dist2; n_within is not defined then and is refused.
static inline bool points_multi_wanted(const srt_point_multi_out* o) { return o->n_within || o->n_found || o->tri || o->dist2 || o->point || o->vw || o->region; }
static int check_points_multi(const srt_scene* s, uint32_t n, const float* points, uint32_t k, uint32_t flags, const srt_point_multi_out* out, bool nearest) {
    SRT_TRY(check_query(s, n, points, flags));
    if (!out || k == 0 || k > SRT_POINT_MULTI_MAX || (nearest && out->n_within)) return SRT_ERR_ARG;
    return SRT_OK;
}
static int points_multi_device_impl(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t k, uint32_t flags,
                                    hipStream_t stream, const srt_point_multi_out* out, bool count_hits, bool nearest) {
    SRT_TRY(check_points_multi(s, n, d_points, k, flags, out, nearest));
    if (!n || (!count_hits && !points_multi_wanted(out))) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { std::array{ BUILDS_3(k_query_points_multi, , 4) }, std::array{ BUILDS_3(k_query_points_multi, , 8) },
                                       std::array{ BUILDS_3(k_query_points_multi, , 16) } };
    static_assert(SRT_POINT_MULTI_MAX == 16, "the largest bucket holds SRT_POINT_MULTI_MAX slots");
    const int bucket = k <= 4 ? 0 : k <= 8 ? 1 : 2;
    return launch_query(builds[bucket][build_index(count, d_point_mask, nearest)], q.grid, q.stream, s->dev, n, d_points, d_radius, k, *out, q.ctr,
                        query_mask(s, d_point_mask));
}

// srt_closest_segments (include/srt_segments.h): the nearest triangle within a radius per segment, one launch (k_query_segments).  A call
// with a mask array launches the MASK build; one without launches the build that reads neither the array nor the scene's table.
static inline bool segments_wanted(const srt_segment_out* o) { return o->tri || o->dist2 || o->s || o->point || o->vw || o->feature; }
static int check_segments(const srt_scene* s, uint32_t n, const float* segments, uint32_t flags, const srt_segment_out* out) {
    SRT_TRY(check_query(s, n, segments, flags));
    if (!out) return SRT_ERR_ARG;
    return SRT_OK;
}
static int segments_device_impl(srt_scene* s, uint32_t n, const float* d_segments, const float* d_radius, const uint32_t* d_seg_mask, uint32_t flags,
                                hipStream_t stream, const srt_segment_out* out, bool count_hits) {
    SRT_TRY(check_segments(s, n, d_segments, flags, out));
    if (!n || (!count_hits && !segments_wanted(out))) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { BUILDS_2(k_query_segments) };
    return launch_query(builds[build_index(count, d_seg_mask)], q.grid, q.stream, s->dev, n, d_segments, d_radius, *out, q.ctr, query_mask(s, d_seg_mask));
}

// srt_signed_points (include/srt_signed.h): srt_nearest_points' outputs and a sign by winding along the rays of a direction table, one
// launch (k_query_signed).  No sign output wanted: the call IS srt_nearest_points, with that call's kernels, and `sign` is not read.
// NEAR: whether the nearest phase runs -- a point output or sdist is wanted; without it hit_rays is 0.
static inline bool sign_wanted(const srt_sign_out* o) { return o && (o->sdist || o->inside || o->winding || o->crossings); }
static int check_signed(const srt_scene* s, uint32_t n, const float* points, const srt_sign* sign, uint32_t flags, const srt_point_out* out, const srt_sign_out* sout) {
    SRT_TRY(check_query(s, n, points, flags));
    if (!out && !sout) return SRT_ERR_ARG;
    if (sign_wanted(sout) && sign) {
        if (sign->n_dirs > SRT_SIGN_MAX_DIRS || (sign->n_dirs == 0) != (sign->dirs == nullptr) || (sign->flags & ~(uint32_t)SRT_SIGN_PARITY)) return SRT_ERR_ARG;
    }
    return SRT_OK;
}
static inline uint32_t sign_dirs(const srt_sign* sign) { return sign && sign->dirs ? sign->n_dirs : 3u; }      // (the default table has three)
static int signed_points_device_impl(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, const srt_sign* sign,
                                     uint32_t flags, hipStream_t stream, const srt_point_out* out, const srt_sign_out* sout, bool count_hits) {
    SRT_TRY(check_signed(s, n, d_points, sign, flags, out, sout));
    const srt_point_out none = {};
    if (!sign_wanted(sout)) return closest_points_device_impl(s, n, d_points, d_radius, d_point_mask, flags, stream, out ? out : &none, count_hits, true);
    if (!n) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0, near = (out && points_wanted(out)) || sout->sdist;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { BUILDS_3(k_query_signed) };
    const QuerySign sg = { sign ? sign->dirs : nullptr, sign_dirs(sign), sign && (sign->flags & SRT_SIGN_PARITY) ? 1u : 0u };
    return launch_query(builds[build_index(count, d_point_mask, near)], q.grid, q.stream, s->dev, n, d_points, d_radius, out ? *out : none, *sout, sg, q.ctr,
                        query_mask(s, d_point_mask));
}

// What a shading kernel takes of the params (after query_prologue: the light table is the handle's device copy)
static QueryShade query_shade(const srt_scene* s, const srt_params* p) {
    QueryShade qs;
    qs.lights = s->d_qlights; qs.n_lights = p->n_lights;
    qs.shadow_div = p->shadow_div; qs.reinhard = p->reinhard; qs.gamma = p->gamma;
    qs.bg = (uint32_t)p->background[0] | ((uint32_t)p->background[1] << 8) | ((uint32_t)p->background[2] << 16);
    qs.spread = p->n_lights >= 8 ? 1u : 0u;      // (measured at 1 and 16 samples, DESIGN.md s5: the spread costs phase 1, and pays with the shadow work)
    return qs;
}

// srt_shade_rays: closest hit, shadow rays, Phong, tone map for caller-supplied rays, one launch (k_query_shade)
// d_t_range: the rays' t intervals (srt_shade_rays_range), or null: the builds without the interval, as trace_rays_device_impl chooses its own
static int shade_rays_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, hipStream_t stream, int32_t* d_hit_id,
                                  float* d_t, float* d_rgb_linear, uint8_t* d_rgb8, bool count_hits) {
    SRT_TRY(check_shade(s, n, d_rays, p));
    if (!n) return SRT_OK;
    const bool count = (p->flags & SRT_FLAG_COUNT_WORK) != 0, smooth = (p->flags & SRT_FLAG_SMOOTH_NORMALS) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, p, count || count_hits, &q));
    // the build: counting, smooth normals, and the integer-shininess pow where every object of the scene allows it (as k_shade_tile)
    static const std::array builds = { BUILDS_4(k_query_shade) };
    return launch_query(builds[build_index(count, smooth, s->rec->int_shin, d_t_range)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), query_shade(s, p),
                        d_hit_id, d_t, d_rgb_linear, d_rgb8, q.ctr, query_range(d_t_range));
}

// srt_shade_paths: up to path->depth mirror bounces per ray, shaded and mixed, one launch (k_query_path)
static int check_paths(const srt_scene* s, uint32_t n, const float* rays, const srt_params* p, const srt_path_desc* path) {
    SRT_TRY(check_shade(s, n, rays, p));
    if (!path || path->depth == 0) return SRT_ERR_ARG;
    if (path->depth > SRT_PATH_DEPTH_MAX) return SRT_ERR_LIMIT;
    return SRT_OK;
}
static inline bool paths_wanted(const float* rgb_linear, const uint8_t* rgb8, const srt_path_out* o) {
    return rgb_linear || rgb8 || (o && (o->hit_id || o->t || o->obj || o->rgb_linear || o->rays));
}
static inline bool fresnel_wanted(const srt_fresnel_out* o) { return o && (o->hit_id || o->t || o->rgb_linear || o->fresnel); }

// What a path call may bring beyond its rays, each part NULL where the entry point has none or its caller passes none: the shadow rule
// of srt_*_paths_shadow, the masks per ray kind of srt_*_paths_masked, the refraction table of srt_*_paths_refract, the Fresnel table and
// the side rays' rows of srt_*_paths_fresnel.
struct PathOptions {
    const srt_shadow_rule* shadow = nullptr; const srt_visibility* vis = nullptr; const srt_refraction* refr = nullptr; const srt_fresnel* fres = nullptr;
    // The two tables of a call that splits, both there or both NULL: without an ior nothing can split, and the call is the one without f0
    const float* ior() const { return refr ? refr->ior : nullptr; }
    const float* f0() const { return ior() && fres ? fres->f0 : nullptr; }
    const srt_fresnel_out* side_rows() const { return f0() ? fres->out : nullptr; }
};
// A rule's flags lie within SRT_SHADOW_SELF, a table's are 0
static inline int check_path_options(const PathOptions& o) {
    if (o.refr && o.refr->flags) return SRT_ERR_ARG;
    if (o.fres && o.fres->flags) return SRT_ERR_ARG;
    if (o.shadow && (o.shadow->flags & ~(uint32_t)SRT_SHADOW_SELF)) return SRT_ERR_ARG;
    return SRT_OK;
}
static inline ShadowRule shadow_rule(const srt_shadow_rule* r) { return ShadowRule{ r->t_min, r->t_max, (r->flags & SRT_SHADOW_SELF) ? 1u : 0u }; }
// The rule a masked call without one runs under: the reference's, stated as a rule -- no bound, the hit's object skipped
static inline ShadowRule shadow_rule_or_reference(const srt_shadow_rule* r) { return r ? shadow_rule(r) : ShadowRule{ std::nanf(""), std::nanf(""), 0u }; }
// The masks a refracting call without an srt_visibility runs under: every ray kind sees every object, and the scene's table is not read
static inline QueryMask query_mask_or_all(const srt_scene* s, const srt_visibility* v) { return v ? query_mask(s, v) : QueryMask{ nullptr, nullptr, ~0u, ~0u, ~0u }; }

extern "C++" {
// The five families of a path kernel, each a table over (COUNT, SMOOTH, INT_SHIN), and the one launch of a path call.  The family: with a
// refraction table and a Fresnel table (PathOptions::f0) the FRESNEL one, under what the REFRACT one runs under; else with a
// refraction table (refr and refr->ior both there) the REFRACT one, under the caller's rule or the reference's and the caller's masks or
// all ones; else with masks the MASK one, under the caller's rule or the reference's; else with a rule the SHADOW one; else the family
// that takes none of them -- the kernel srt_shade_paths / srt_render_paths launched before any of them existed.  `lead`: the
// arguments all five take.
template <typename P, typename S, typename M, typename R, typename F>
struct PathBuilds { std::array<P, 8> plain; std::array<S, 8> shadow; std::array<M, 8> masked; std::array<R, 8> refract; std::array<F, 8> fresnel; };
template <typename P, typename S, typename M, typename R, typename F>
static PathBuilds<P, S, M, R, F> path_builds(const std::array<P, 8>& plain, const std::array<S, 8>& shadow, const std::array<M, 8>& masked, const std::array<R, 8>& refract,
                                             const std::array<F, 8>& fresnel) {
    return PathBuilds<P, S, M, R, F>{ plain, shadow, masked, refract, fresnel };
}
template <typename Builds, typename... A>
static int launch_paths(const Builds& builds, const srt_scene* s, const srt_params* p, const PathOptions& o, dim3 grid, hipStream_t stream, const A&... lead) {
    const size_t build = build_index((p->flags & SRT_FLAG_COUNT_WORK) != 0, (p->flags & SRT_FLAG_SMOOTH_NORMALS) != 0, s->rec->int_shin);
    if (const float* d_f0 = o.f0()) {
        const srt_fresnel_out* rows = o.side_rows();
        return launch_query(builds.fresnel[build], grid, stream, lead..., shadow_rule_or_reference(o.shadow), query_mask_or_all(s, o.vis), o.ior(),
                            QueryFresnel{ d_f0, rows ? *rows : srt_fresnel_out{} });
    }
    if (const float* d_ior = o.ior())
        return launch_query(builds.refract[build], grid, stream, lead..., shadow_rule_or_reference(o.shadow), query_mask_or_all(s, o.vis), d_ior);
    if (o.vis) return launch_query(builds.masked[build], grid, stream, lead..., shadow_rule_or_reference(o.shadow), query_mask(s, o.vis));
    if (o.shadow) return launch_query(builds.shadow[build], grid, stream, lead..., shadow_rule(o.shadow));
    return launch_query(builds.plain[build], grid, stream, lead...);
}
}      // extern "C++"

static int shade_paths_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path,
                                   const PathOptions& opt, hipStream_t stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg, bool count_hits) {
    SRT_TRY(check_path_options(opt));
    SRT_TRY(check_paths(s, n, d_rays, p, path));
    if (!n || (!count_hits && !paths_wanted(d_rgb_linear, d_rgb8, seg) && !fresnel_wanted(opt.side_rows()))) return SRT_OK;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, p, (p->flags & SRT_FLAG_COUNT_WORK) != 0 || count_hits, &q));
    static const auto builds = path_builds(std::array{ BUILDS_3(k_query_path) }, std::array{ BUILDS_3(k_query_path_shadow) }, std::array{ BUILDS_3(k_query_path_masked) },
                                           std::array{ BUILDS_3(k_query_path_refract) }, std::array{ BUILDS_3(k_query_path_fresnel) });
    return launch_paths(builds, s, p, opt, q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), query_shade(s, p), query_range(d_t_range), *path, d_rgb_linear, d_rgb8,
                        seg ? *seg : srt_path_out{}, q.ctr);
}

// srt_render_paths: mirror paths for the pixels of a frame, one launch (k_render_path).  A query-family call: the handle's query light table
// and query counter set; the render's counter sets, workspaces, event ring and pipeline string are left alone.
static int check_render_paths(const srt_scene* s, const srt_params* p, const srt_path_desc* path) {
    if (!s || !p) return SRT_ERR_ARG;
    if (p->flags & ~(uint32_t)(SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS | SRT_FLAG_NO_TIMING | SRT_FLAG_FRAMES_IN_FLIGHT)) return SRT_ERR_ARG;      // (variant bits included)
    SRT_TRY(check_frame(scene_facts(s), p));
    if (!path || path->depth == 0) return SRT_ERR_ARG;
    if (path->depth > SRT_PATH_DEPTH_MAX) return SRT_ERR_LIMIT;
    if ((uint64_t)srt_rows_owned(p) * srt_cols_owned(p) * (p->n_lights ? p->n_lights : 1) >= (1ull << 32)) return SRT_ERR_LIMIT;
    return SRT_OK;
}
static int render_paths_device_impl(srt_scene* s, const srt_params* p, const srt_path_desc* path, const PathOptions& opt, hipStream_t stream, float* d_rgb_linear,
                                    uint8_t* d_rgb8, const srt_path_out* seg, bool count_hits) {
    SRT_TRY(check_path_options(opt));
    SRT_TRY(check_render_paths(s, p, path));
    const uint32_t rows = srt_rows_owned(p), wl = srt_cols_owned(p);
    if (!rows || !wl || (!count_hits && !paths_wanted(d_rgb_linear, d_rgb8, seg) && !fresnel_wanted(opt.side_rows()))) return SRT_OK;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, 0, stream, p, (p->flags & SRT_FLAG_COUNT_WORK) != 0 || count_hits, &q));
    const DevParams dp = dev_params(s, p, FramePlan{}).hit;      // the frame's geometry only: the kernel takes lights and literals from QueryShade
    const uint32_t m = (uint32_t)std::lround(std::sqrt((double)p->spp));      // (m x m == spp: check_frame)
    static const auto builds = path_builds(std::array{ BUILDS_3(k_render_path) }, std::array{ BUILDS_3(k_render_path_shadow) }, std::array{ BUILDS_3(k_render_path_masked) },
                                           std::array{ BUILDS_3(k_render_path_refract) }, std::array{ BUILDS_3(k_render_path_fresnel) });
    return launch_paths(builds, s, p, opt, dim3((wl + 15) / 16, (rows + 15) / 16), q.stream, s->dev, dp, p->spp, m, query_shade(s, p), *path, d_rgb_linear, d_rgb8,
                        seg ? *seg : srt_path_out{}, q.ctr);
}

// srt_surface_rays / srt_surface_hits: the surface under each hit and the mirrored ray (k_query_surface, k_query_surface_hits)
static int check_surface(const srt_scene* s, uint32_t n, const float* rays, uint32_t flags, uint32_t allowed) {
    if (!s || (n && !rays) || (flags & ~allowed)) return SRT_ERR_ARG;
    if ((flags & SRT_FLAG_SMOOTH_NORMALS) && !s->dev.tri_normals) return SRT_ERR_ARG;      // needs vertex normals, as check_shade
    return SRT_OK;
}
static inline bool surface_wanted(const srt_surface_out* o) { return o && (o->obj || o->point || o->normal || o->color || o->material || o->bounce); }

static int surface_rays_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t flags, hipStream_t stream, int32_t* d_hit_id,
                                    float* d_t, const srt_surface_out* out, bool count_hits) {
    SRT_TRY(check_surface(s, n, d_rays, flags, SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS));
    // nothing of the surface wanted: the call is srt_trace_rays_range without bary, and launches its kernel
    if (!surface_wanted(out)) return trace_rays_device_impl(s, n, d_rays, d_t_range, flags & SRT_FLAG_COUNT_WORK, stream, d_hit_id, d_t, nullptr, count_hits, RayMask{});
    if (!n) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0, smooth = (flags & SRT_FLAG_SMOOTH_NORMALS) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    static const std::array builds = { BUILDS_3(k_query_surface) };
    return launch_query(builds[build_index(count, smooth, d_t_range)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_hit_id, d_t, *out, q.ctr,
                        query_range(d_t_range));
}

static int check_surface_hits(const srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t, uint32_t flags) {
    SRT_TRY(check_surface(s, n, rays, flags, SRT_FLAG_SMOOTH_NORMALS));
    return (n && (!hit_id || !t)) ? SRT_ERR_ARG : SRT_OK;
}
static int surface_hits_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_hit_id, const float* d_t, uint32_t flags, hipStream_t stream,
                                    const srt_surface_out* out) {
    SRT_TRY(check_surface_hits(s, n, d_rays, d_hit_id, d_t, flags));
    if (!n || !surface_wanted(out)) return SRT_OK;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, false, &q));
    static const std::array builds = { BUILDS_1(k_query_surface_hits) };
    return launch_query(builds[build_index((flags & SRT_FLAG_SMOOTH_NORMALS) != 0)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), d_hit_id, d_t, *out);
}

// srt_ao_rays / srt_ao_hits: the hemisphere visibility at each hit, one launch (k_query_ao).  hits: the hits a caller of srt_ao_hits
// brings (NULL: srt_ao_rays, which walks for its own and returns them in d_hit_id / d_t).
static int check_ao(const srt_scene* s, uint32_t n, const float* rays, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao) {
    SRT_TRY(check_surface(s, n, rays, flags, SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS));
    if (hits && n && (!hits->hit_id || !hits->t)) return SRT_ERR_ARG;
    if (!ao || !ao->dirs || ao->n_dirs == 0 || (ao->flags & ~(uint32_t)SRT_AO_SKIP_SELF)) return SRT_ERR_ARG;
    if (ao->n_dirs > SRT_AO_DIRS_MAX || (uint64_t)n * ao->n_dirs >= (1ull << 32)) return SRT_ERR_LIMIT;
    return SRT_OK;
}
static inline bool ao_wanted(const srt_ao_out* o) { return o && (o->n_occluded || o->ao || o->occ_bits); }
// The deal of rays to waves: the spread deal from this many directions on.  The threshold is borrowed from QueryShade::spread (n_lights >= 8)
// and was not measured itself; the two deals were timed at 16 and 64 directions only ("Ambient occlusion").
#ifndef SRT_AO_SPREAD_FROM
#define SRT_AO_SPREAD_FROM 8u
#endif

static int ao_device_impl(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao,
                          const srt_visibility* vis, hipStream_t stream, int32_t* d_hit_id, float* d_t, const srt_ao_out* out, bool count_hits) {
    SRT_TRY(check_ao(s, n, d_rays, hits, flags, ao));
    const bool wanted = ao_wanted(out);
    // nothing of srt_ao_out wanted, every object visible to the primary rays: srt_ao_rays is srt_trace_rays_masked without bary, and launches its kernel
    if (!hits && !wanted && (!vis || vis->primary == ~0u))
        return trace_rays_device_impl(s, n, d_rays, d_t_range, flags & SRT_FLAG_COUNT_WORK, stream, d_hit_id, d_t, nullptr, count_hits, RayMask{ .masked = true });
    if (!n || (hits && !wanted && !count_hits)) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0, smooth = (flags & SRT_FLAG_SMOOTH_NORMALS) != 0;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, n, stream, nullptr, count || count_hits, &q));
    const QueryAo p = { ao->dirs, wanted ? ao->n_dirs : 0u, ao->t_min, ao->t_max, (ao->flags & SRT_AO_SKIP_SELF) ? 1u : 0u, ao->n_dirs >= SRT_AO_SPREAD_FROM ? 1u : 0u };
    static const std::array builds = { BUILDS_3(k_query_ao) };
    return launch_query(builds[build_index(count, smooth, hits)], q.grid, q.stream, s->dev, n, d_rays, rays_wide(d_rays), query_range(d_t_range),
                        vis ? query_mask(s, vis) : query_mask(s, (const uint32_t*)nullptr),      // (a NULL vis: all ones against the scene's table)
                        p, hits ? *hits : QueryHits{}, d_hit_id, d_t, wanted ? *out : srt_ao_out{}, q.ctr);
}

// srt_render_ao / srt_render_ao_hits: srt_ao_rays' hemisphere visibility for the pixels of a frame, one launch (k_render_ao).  A
// query-family call, as srt_render_paths is: the query counter set; the renders' counter sets, workspaces, event ring and pipeline string
// are left alone.  hits: the hits a caller of srt_render_ao_hits brings, laid out as srt_render_device writes them (NULL: srt_render_ao).
static int check_render_ao(const srt_scene* s, const srt_params* p, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr) {
    if (!s || !p) return SRT_ERR_ARG;
    if (p->flags & ~(uint32_t)(SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS | SRT_FLAG_NO_TIMING | SRT_FLAG_FRAMES_IN_FLIGHT)) return SRT_ERR_ARG;      // (variant bits included)
    SRT_TRY(check_frame(scene_facts(s), p));
    SRT_TRY(check_surface(s, 0, nullptr, flags, SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS));
    if (hits && (!hits->hit_id || !hits->t)) return SRT_ERR_ARG;
    if (!ao || !ao->dirs || ao->n_dirs == 0 || (ao->flags & ~(uint32_t)SRT_AO_SKIP_SELF)) return SRT_ERR_ARG;
    if (fr && (fr->rot ? (!fr->rot_w || !fr->rot_h) : (fr->rot_w || fr->rot_h))) return SRT_ERR_ARG;
    if (ao->n_dirs > SRT_AO_DIRS_MAX || (fr && (fr->rot_w > SRT_AO_ROT_MAX || fr->rot_h > SRT_AO_ROT_MAX))) return SRT_ERR_LIMIT;
    if ((uint64_t)srt_rows_owned(p) * srt_cols_owned(p) * ao->n_dirs * p->spp >= (1ull << 32)) return SRT_ERR_LIMIT;      // (< 2^31 x 2^10 x 2^12: no overflow)
    return SRT_OK;
}
static inline bool ao_frame_wanted(const srt_ao_frame_out* o) { return o && (o->n_occluded || o->ao || o->occ_bits || o->bent || o->ao8); }

static int render_ao_device_impl(srt_scene* s, const srt_params* p, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr,
                                 const srt_visibility* vis, hipStream_t stream, int32_t* d_hit_id, float* d_t, const srt_ao_frame_out* out, bool count_hits) {
    SRT_TRY(check_render_ao(s, p, hits, flags, ao, fr));
    const uint32_t rows = srt_rows_owned(p), wl = srt_cols_owned(p);
    const bool wanted = ao_frame_wanted(out);
    // nothing of srt_ao_frame_out wanted: the _hits form has nothing to do; the ray form writes hit_id / t and walks no AO ray
    if (!rows || !wl || (!wanted && !count_hits && (hits || (!d_hit_id && !d_t)))) return SRT_OK;
    const bool count = (flags & SRT_FLAG_COUNT_WORK) != 0, smooth = (flags & SRT_FLAG_SMOOTH_NORMALS) != 0, rotated = fr && fr->rot;
    QueryLaunch q;
    SRT_TRY(query_prologue(s, 0, stream, nullptr, count || count_hits, &q));
    const DevParams dp = dev_params(s, p, FramePlan{}).hit;      // the frame's geometry only
    const uint32_t m = (uint32_t)std::lround(std::sqrt((double)p->spp));      // (m x m == spp: check_frame)
    const QueryAo qa = { ao->dirs, wanted ? ao->n_dirs : 0u, ao->t_min, ao->t_max, (ao->flags & SRT_AO_SKIP_SELF) ? 1u : 0u, 0u };      // (spread: the deal is the tiles')
    const QueryAoRot rot = rotated ? QueryAoRot{ fr->rot, fr->rot_w, fr->rot_h } : QueryAoRot{ nullptr, 1u, 1u };
    static const std::array builds = { BUILDS_4(k_render_ao) };
    return launch_query(builds[build_index(count, smooth, hits, rotated)], dim3((wl + 15) / 16, (rows + 15) / 16), q.stream, s->dev, dp, p->spp, m,
                        vis ? query_mask(s, vis) : query_mask(s, (const uint32_t*)nullptr), qa, rot, hits ? *hits : QueryHits{}, d_hit_id, d_t,
                        wanted ? *out : srt_ao_frame_out{}, q.ctr);
}

// The host entry points: what the caller brings goes through the pinned staging block (stage_acquire, as every update does) into the
// handle's query block on the scene's stream, the device entry point runs behind it, the call waits and copies the results out.
extern "C++" {      // (templates, down to the entry points)
// One array of a host query, `count` elements of T: a result the caller wants at `out` (null: not wanted), or what the call brings with
// it at `in` (null: not brought) -- the rays (srt_render_paths brings none: a frame's rays are made on the device), their t intervals,
// the skipped objects of srt_occluded, the hits of srt_surface_hits, the per-ray masks of the masked calls, the tables of the path and
// AO calls.  dev: its piece of the query block, which the round trip sets; an absent array takes no space and keeps NULL, which the
// device entry points and the kernels read as "not wanted" or "not brought".
template <typename T>
struct QueryArray {
    const T* in; T* out; size_t count;
    T* dev = nullptr;
    bool present() const { return in || out; }
    size_t bytes() const { return count * sizeof(T); }
    size_t piece() const { return present() ? (bytes() + 255) & ~(size_t)255 : 0; }      // what it takes of the block
    T* on_device() const { return dev; }                                                 // (inside the round trip's launch)
};
template <typename T>
static QueryArray<T> query_out(T* host, size_t count) { return QueryArray<T>{ nullptr, host, count }; }
template <typename T>
static QueryArray<T> query_in(const T* host, size_t count) { return QueryArray<T>{ host, nullptr, count }; }

// The round trip of a host query on the scene's own stream: lay the arrays that are there out in the query block, stage the ones the
// call brings, launch(stream) -- the device entry point --, wait, copy each wanted result out.  The layout: every piece starts on a
// multiple of 256 bytes, as a hipMalloc block does (rays_wide and query_range choose the 8-byte loads by the pointer), and what the call
// brings comes first, so that the same offsets serve the pinned block, which holds those alone.
// preload: the frame is a tile deal, whose padding pixels no kernel writes: the caller's arrays go to the device first, so that the copy
// out returns their padding as it was.  hipMemcpy from pageable memory returns when the data is on the device, so the launch enqueued on
// the stream behind it is ordered behind these copies without an event.  It costs a second transfer of the size of the result (a tile
// deal in the host form is the rare case; a row-wise copy out of the live columns would save it).
template <typename Launch, typename... A>
static int query_round_trip(srt_scene* s, bool preload, Launch launch, A&... arrays) {
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st;
    SRT_TRY(own_stream(s, &st));
    size_t at_in = 0, at_out = ((arrays.in ? arrays.piece() : 0) + ... + 0);
    SRT_TRY(grow(s, at_out + ((arrays.out ? arrays.piece() : 0) + ... + 0), s->query_block));
    char* h = nullptr;
    SRT_TRY(stage_acquire(s, at_out, &h));
    hipError_t e = hipSuccess;
    const auto place = [&](auto& a) {      // its piece; an array the call brings goes into the pinned block and is sent on from it
        if (!a.present()) return;
        size_t& at = a.in ? at_in : at_out;
        a.dev = reinterpret_cast<decltype(a.dev)>(s->query_block.p + at);
        if (a.in && a.bytes() && e == hipSuccess) {
            std::memcpy(h + at, a.in, a.bytes());
            e = hipMemcpyAsync(a.dev, h + at, a.bytes(), hipMemcpyHostToDevice, st);
        }
        at += a.piece();
    };
    (place(arrays), ...);
    HIP_TRY(e);
    HIP_TRY(hipEventRecord(s->staged, st));
    if (preload) ((e = (e == hipSuccess && arrays.out) ? hipMemcpy(arrays.dev, arrays.out, arrays.bytes(), hipMemcpyHostToDevice) : e), ...);
    HIP_TRY(e);
    SRT_TRY(launch(st));
    HIP_TRY(hipStreamSynchronize(st));
    if (s->qlights_stream == st) s->qlights_settled = true;      // a light table sent on this stream has arrived
    ((e = (e == hipSuccess && arrays.out) ? hipMemcpy(arrays.out, arrays.dev, arrays.bytes(), hipMemcpyDeviceToHost) : e), ...);
    HIP_TRY(e);
    return SRT_OK;
}

// The private counter set of the query that just ran (cleared before its launch), as srt_stats; n_lights: shadow rays per hit.
static int query_stats(srt_scene* s, uint32_t n, uint32_t n_lights, srt_stats* stats) {
    std::array<unsigned long long, NCTR> c;
    HIP_TRY(hipMemcpy(c.data(), s->d_qctr, NCTR * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    stats->primary_rays = n;
    for (int k = 0; k < HIT_SHARDS; k++) stats->hit_rays += c[CTR_HIT_BASE + 8 * k];
    stats->shadow_rays = stats->hit_rays * n_lights;
    stats->node_tests_primary = c[1]; stats->tri_tests_primary = c[2];
    stats->node_tests_shadow = c[3]; stats->tri_tests_shadow = c[4];
    return SRT_OK;
}

static int trace_rays_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, int32_t* hit_id, float* t, float* bary,
                           srt_stats* stats, const RayMask& mask) {
    SRT_TRY(check_query(s, n, rays, flags));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    auto o_hit = query_out(hit_id, n); auto o_t = query_out(t, n); auto o_bary = query_out(bary, 3ull * n);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n); auto i_mask = query_in(mask.words, n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        return trace_rays_device_impl(s, n, i_rays.on_device(), i_range.on_device(), flags, st, o_hit.on_device(), o_t.on_device(), o_bary.on_device(), true,
                                      RayMask{ mask.masked, i_mask.on_device() });
    }, o_hit, o_t, o_bary, i_rays, i_range, i_mask));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int closest_points_impl(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t flags,
                               const srt_point_out* out, srt_stats* stats, bool nearest = false) {
    SRT_TRY(check_query(s, n, points, flags));
    if (!out) return SRT_ERR_ARG;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    auto o_tri = query_out(out->tri, n); auto o_d2 = query_out(out->dist2, n); auto o_pt = query_out(out->point, 3ull * n);
    auto o_vw = query_out(out->vw, 2ull * n); auto o_reg = query_out(out->region, n);
    auto i_pts = query_in(points, 3ull * n); auto i_rad = query_in(radius, n); auto i_mask = query_in(point_mask, n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        const srt_point_out dev = { o_tri.on_device(), o_d2.on_device(), o_pt.on_device(), o_vw.on_device(), o_reg.on_device() };
        return closest_points_device_impl(s, n, i_pts.on_device(), i_rad.on_device(), i_mask.on_device(), flags, st, &dev, stats != nullptr, nearest);
    }, o_tri, o_d2, o_pt, o_vw, o_reg, i_pts, i_rad, i_mask));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int points_multi_impl(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t k, uint32_t flags,
                             const srt_point_multi_out* out, srt_stats* stats, bool nearest) {
    SRT_TRY(check_points_multi(s, n, points, k, flags, out, nearest));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    const size_t rows = (size_t)n * k;      // the n x k rows
    auto o_nw = query_out(out->n_within, n); auto o_nf = query_out(out->n_found, n); auto o_tri = query_out(out->tri, rows); auto o_d2 = query_out(out->dist2, rows);
    auto o_pt = query_out(out->point, 3 * rows); auto o_vw = query_out(out->vw, 2 * rows); auto o_reg = query_out(out->region, rows);
    auto i_pts = query_in(points, 3ull * n); auto i_rad = query_in(radius, n); auto i_mask = query_in(point_mask, n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        const srt_point_multi_out dev = { o_nw.on_device(), o_nf.on_device(), o_tri.on_device(), o_d2.on_device(), o_pt.on_device(), o_vw.on_device(), o_reg.on_device() };
        return points_multi_device_impl(s, n, i_pts.on_device(), i_rad.on_device(), i_mask.on_device(), k, flags, st, &dev, stats != nullptr, nearest);
    }, o_nw, o_nf, o_tri, o_d2, o_pt, o_vw, o_reg, i_pts, i_rad, i_mask));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int segments_impl(srt_scene* s, uint32_t n, const float* segments, const float* radius, const uint32_t* seg_mask, uint32_t flags,
                         const srt_segment_out* out, srt_stats* stats) {
    SRT_TRY(check_segments(s, n, segments, flags, out));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    auto o_tri = query_out(out->tri, n); auto o_d2 = query_out(out->dist2, n); auto o_s = query_out(out->s, n); auto o_pt = query_out(out->point, 3ull * n);
    auto o_vw = query_out(out->vw, 2ull * n); auto o_feat = query_out(out->feature, n);
    auto i_seg = query_in(segments, 6ull * n); auto i_rad = query_in(radius, n); auto i_mask = query_in(seg_mask, n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        const srt_segment_out dev = { o_tri.on_device(), o_d2.on_device(), o_s.on_device(), o_pt.on_device(), o_vw.on_device(), o_feat.on_device() };
        return segments_device_impl(s, n, i_seg.on_device(), i_rad.on_device(), i_mask.on_device(), flags, st, &dev, stats != nullptr);
    }, o_tri, o_d2, o_s, o_pt, o_vw, o_feat, i_seg, i_rad, i_mask));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int signed_points_impl(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, const srt_sign* sign, uint32_t flags,
                              const srt_point_out* out, const srt_sign_out* sout, srt_stats* stats) {
    SRT_TRY(check_signed(s, n, points, sign, flags, out, sout));
    const srt_point_out none = {};
    if (!sign_wanted(sout)) return closest_points_impl(s, n, points, radius, point_mask, flags, out ? out : &none, stats, true);
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    if (!out) out = &none;
    const uint32_t nd = sign_dirs(sign);
    const size_t rows = (size_t)n * nd;      // the n x n_dirs rows
    auto o_tri = query_out(out->tri, n); auto o_d2 = query_out(out->dist2, n); auto o_pt = query_out(out->point, 3ull * n);
    auto o_vw = query_out(out->vw, 2ull * n); auto o_reg = query_out(out->region, n);
    auto o_sd = query_out(sout->sdist, n); auto o_in = query_out(sout->inside, n); auto o_wind = query_out(sout->winding, rows); auto o_cross = query_out(sout->crossings, rows);
    auto i_pts = query_in(points, 3ull * n); auto i_rad = query_in(radius, n); auto i_mask = query_in(point_mask, n);
    auto i_dirs = query_in(sign ? sign->dirs : nullptr, 3ull * nd);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        const srt_point_out dev = { o_tri.on_device(), o_d2.on_device(), o_pt.on_device(), o_vw.on_device(), o_reg.on_device() };
        const srt_sign_out sdev = { o_sd.on_device(), o_in.on_device(), o_wind.on_device(), o_cross.on_device() };
        const srt_sign sg = { i_dirs.on_device(), i_dirs.on_device() ? nd : 0u, sign ? sign->flags : 0u };
        return signed_points_device_impl(s, n, i_pts.on_device(), i_rad.on_device(), i_mask.on_device(), &sg, flags, st, &dev, &sdev, stats != nullptr);
    }, o_tri, o_d2, o_pt, o_vw, o_reg, o_sd, o_in, o_wind, o_cross, i_pts, i_rad, i_mask, i_dirs));
    if (!stats) return SRT_OK;
    SRT_TRY(query_stats(s, n, 0, stats));
    stats->shadow_rays = rows;
    return SRT_OK;
}

static int trace_rays_multi_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t k, uint32_t flags, uint32_t* n_hits, int32_t* hit_id,
                                 float* t, float* bary, srt_stats* stats) {
    SRT_TRY(check_multi(s, n, rays, k, flags));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    const size_t rows = (size_t)n * k;      // the n x k rows
    auto o_n = query_out(n_hits, n); auto o_hit = query_out(hit_id, rows); auto o_t = query_out(t, rows); auto o_bary = query_out(bary, 3 * rows);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        return trace_rays_multi_device_impl(s, n, i_rays.on_device(), i_range.on_device(), k, flags, st, o_n.on_device(), o_hit.on_device(), o_t.on_device(),
                                            o_bary.on_device(), true);
    }, o_n, o_hit, o_t, o_bary, i_rays, i_range));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int occluded_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const int32_t* skip_obj, uint8_t* occluded, const RayMask& mask) {
    SRT_TRY(check_query(s, n, rays, 0));
    if (!n || !occluded) return SRT_OK;
    auto o_occ = query_out(occluded, n);
    auto i_rays = query_in(rays, 6ull * n); auto i_skip = query_in(skip_obj, n); auto i_range = query_in(t_range, 2ull * n); auto i_mask = query_in(mask.words, n);
    return query_round_trip(s, false, [&](hipStream_t st) {
        return occluded_device_impl(s, n, i_rays.on_device(), i_range.on_device(), i_skip.on_device(), st, o_occ.on_device(), RayMask{ mask.masked, i_mask.on_device() });
    }, o_occ, i_rays, i_skip, i_range, i_mask);
}

static int shade_rays_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear,
                           uint8_t* rgb8, srt_stats* stats) {
    SRT_TRY(check_shade(s, n, rays, p));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    auto o_hit = query_out(hit_id, n); auto o_t = query_out(t, n); auto o_lin = query_out(rgb_linear, 3ull * n); auto o_rgb8 = query_out(rgb8, 3ull * n);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n);
    SRT_TRY(query_round_trip(s, false, [&](hipStream_t st) {
        return shade_rays_device_impl(s, n, i_rays.on_device(), i_range.on_device(), p, st, o_hit.on_device(), o_t.on_device(), o_lin.on_device(), o_rgb8.on_device(), true);
    }, o_hit, o_t, o_lin, o_rgb8, i_rays, i_range));
    return stats ? query_stats(s, n, p->n_lights, stats) : SRT_OK;
}

// What the host forms of the two path calls share: the seven results of n rays or pixels and the four of the side rays (the per-segment rows
// are depth x n rows each), the reflectance, refraction and Fresnel tables (n_objects floats each, where the call brings them; the side
// rays' rows and f0 only where the call splits, PathOptions::f0), and the round trip of all of them, in which
// launch(stream, path, options, segments) gets the caller's structs with the pieces of the query block in the place of the host arrays.
struct PathArrays {
    QueryArray<float> lin; QueryArray<uint8_t> rgb8;
    QueryArray<int32_t> hit; QueryArray<float> t; QueryArray<int32_t> obj; QueryArray<float> seg_lin, rays;
    QueryArray<float> refl, ior, f0;
    QueryArray<int32_t> side_hit; QueryArray<float> side_t, side_lin, side_F;
    template <typename Launch, typename... In>      // in: what else the call brings; preload: query_round_trip's
    int round_trip(srt_scene* s, bool preload, const srt_path_desc* path, const PathOptions& opt, Launch launch, In&... in) {
        return query_round_trip(s, preload, [&](hipStream_t st) -> int {
            const srt_path_desc dpath = { path->depth, path->bounce_t_min, refl.on_device() };
            const srt_refraction drefr = { ior.on_device(), 0u };
            const srt_path_out dseg = { hit.on_device(), t.on_device(), obj.on_device(), seg_lin.on_device(), rays.on_device() };
            const srt_fresnel_out dside = { side_hit.on_device(), side_t.on_device(), side_lin.on_device(), side_F.on_device() };
            const srt_fresnel dfres = { f0.on_device(), 0u, &dside };
            return launch(st, &dpath, PathOptions{ .shadow = opt.shadow, .vis = opt.vis, .refr = &drefr, .fres = &dfres }, &dseg);
        }, lin, rgb8, hit, t, obj, seg_lin, rays, side_hit, side_t, side_lin, side_F, in..., refl, ior, f0);
    }
};
static PathArrays path_arrays(const srt_scene* s, uint32_t n, const srt_path_desc* path, const PathOptions& opt, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg) {
    const srt_path_out h = seg ? *seg : srt_path_out{};
    const srt_fresnel_out f = opt.side_rows() ? *opt.side_rows() : srt_fresnel_out{};
    const size_t rows = (size_t)path->depth * n, nO = s->dev.n_objects;
    return PathArrays{ query_out(rgb_linear, 3ull * n), query_out(rgb8, 3ull * n), query_out(h.hit_id, rows), query_out(h.t, rows), query_out(h.obj, rows),
                       query_out(h.rgb_linear, 3 * rows), query_out(h.rays, 6 * rows), query_in(path->reflectance, nO), query_in(opt.ior(), nO), query_in(opt.f0(), nO),
                       query_out(f.hit_id, rows), query_out(f.t, rows), query_out(f.rgb_linear, 3 * rows), query_out(f.fresnel, rows) };
}

// srt_shade_paths: hit_rays counts the hits of all segments, hence the shadow rays
static int shade_paths_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, const PathOptions& opt,
                            float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    SRT_TRY(check_path_options(opt));
    SRT_TRY(check_paths(s, n, rays, p, path));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n || (!stats && !paths_wanted(rgb_linear, rgb8, seg) && !fresnel_wanted(opt.side_rows()))) return SRT_OK;
    PathArrays a = path_arrays(s, n, path, opt, rgb_linear, rgb8, seg);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n);
    SRT_TRY(a.round_trip(s, false, path, opt, [&](hipStream_t st, const srt_path_desc* dpath, const PathOptions& dopt, const srt_path_out* dseg) {
        return shade_paths_device_impl(s, n, i_rays.on_device(), i_range.on_device(), p, dpath, dopt, st, a.lin.on_device(), a.rgb8.on_device(), dseg, stats != nullptr);
    }, i_rays, i_range));
    return stats ? query_stats(s, n, p->n_lights, stats) : SRT_OK;
}

// srt_render_paths: as shade_paths_impl, with n the call's local pixels and no rays to stage; primary_rays counts image pixels x spp
static int render_paths_impl(srt_scene* s, const srt_params* p, const srt_path_desc* path, const PathOptions& opt, float* rgb_linear, uint8_t* rgb8,
                             const srt_path_out* seg, srt_stats* stats) {
    SRT_TRY(check_path_options(opt));
    SRT_TRY(check_render_paths(s, p, path));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const uint32_t n = srt_rows_owned(p) * srt_cols_owned(p);      // (< 2^32: check_render_paths)
    if (!n || (!stats && !paths_wanted(rgb_linear, rgb8, seg) && !fresnel_wanted(opt.side_rows()))) return SRT_OK;
    PathArrays a = path_arrays(s, n, path, opt, rgb_linear, rgb8, seg);
    // (a tile deal's padding pixels are not written: what the query block holds there must not reach the caller)
    SRT_TRY(a.round_trip(s, p->block_cols != 0, path, opt, [&](hipStream_t st, const srt_path_desc* dpath, const PathOptions& dopt, const srt_path_out* dseg) {
        return render_paths_device_impl(s, p, dpath, dopt, st, a.lin.on_device(), a.rgb8.on_device(), dseg, stats != nullptr);
    }));
    if (!stats) return SRT_OK;
    SRT_TRY(query_stats(s, n, p->n_lights, stats));
    stats->primary_rays = pixels_owned(p) * p->spp;
    return SRT_OK;
}

// What the host forms of the two surface calls share: the six arrays of the caller's srt_surface_out (host arrays), and the round trip of
// them, in which launch(stream, out) gets the srt_surface_out that names the pieces of the query block for the wanted ones.
struct SurfaceArrays {
    QueryArray<int32_t> obj; QueryArray<float> point, normal, color, material, bounce;
    template <typename Launch, typename... More>      // more: the call's other arrays
    int round_trip(srt_scene* s, Launch launch, More&... more) {
        return query_round_trip(s, false, [&](hipStream_t st) -> int {
            const srt_surface_out dev = { obj.on_device(), point.on_device(), normal.on_device(), color.on_device(), material.on_device(), bounce.on_device() };
            return launch(st, &dev);
        }, more..., obj, point, normal, color, material, bounce);
    }
};
static SurfaceArrays surface_arrays(uint32_t n, const srt_surface_out* out) {
    const srt_surface_out h = out ? *out : srt_surface_out{};
    return SurfaceArrays{ query_out(h.obj, n), query_out(h.point, 3ull * n), query_out(h.normal, 3ull * n), query_out(h.color, 3ull * n), query_out(h.material, 3ull * n),
                          query_out(h.bounce, 6ull * n) };
}

static int surface_rays_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, int32_t* hit_id, float* t, const srt_surface_out* out,
                             srt_stats* stats) {
    SRT_TRY(check_surface(s, n, rays, flags, SRT_FLAG_COUNT_WORK | SRT_FLAG_SMOOTH_NORMALS));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n) return SRT_OK;
    SurfaceArrays a = surface_arrays(n, out);
    auto o_hit = query_out(hit_id, n); auto o_t = query_out(t, n);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n);
    SRT_TRY(a.round_trip(s, [&](hipStream_t st, const srt_surface_out* dev) {
        return surface_rays_device_impl(s, n, i_rays.on_device(), i_range.on_device(), flags, st, o_hit.on_device(), o_t.on_device(), dev, true);
    }, o_hit, o_t, i_rays, i_range));
    return stats ? query_stats(s, n, 0, stats) : SRT_OK;
}

static int surface_hits_impl(srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t, uint32_t flags, const srt_surface_out* out) {
    SRT_TRY(check_surface_hits(s, n, rays, hit_id, t, flags));
    if (!n || !surface_wanted(out)) return SRT_OK;
    SurfaceArrays a = surface_arrays(n, out);
    auto i_rays = query_in(rays, 6ull * n); auto i_hit = query_in(hit_id, n); auto i_t = query_in(t, n);
    return a.round_trip(s, [&](hipStream_t st, const srt_surface_out* dev) {
        return surface_hits_device_impl(s, n, i_rays.on_device(), i_hit.on_device(), i_t.on_device(), flags, st, dev);
    }, i_rays, i_hit, i_t);
}

// What the host forms of the four AO calls share: the direction table the call brings, the rotation table of a frame call, the arrays of
// the caller's srt_ao_out or srt_ao_frame_out (whose first three fields are srt_ao_out's), and the round trip of them, in which
// launch(stream, ao, frame, out) gets the caller's structs with the pieces of the query block in the place of the host arrays.
struct AoArrays {
    QueryArray<float> dirs; QueryArray<uint32_t> cnt; QueryArray<float> val; QueryArray<uint32_t> bits;
    QueryArray<float> rot, bent; QueryArray<uint8_t> ao8;
    uint32_t rot_w, rot_h;
    template <typename Launch, typename... More>      // more: the call's other arrays; preload: query_round_trip's
    int round_trip(srt_scene* s, bool preload, const srt_ao_desc* ao, Launch launch, More&... more) {
        return query_round_trip(s, preload, [&](hipStream_t st) -> int {
            const srt_ao_desc dao = { ao->n_dirs, dirs.on_device(), ao->t_min, ao->t_max, ao->flags };
            const srt_ao_frame dfr = { rot_w, rot_h, rot.on_device() };
            const srt_ao_frame_out dev = { cnt.on_device(), val.on_device(), bits.on_device(), bent.on_device(), ao8.on_device() };
            return launch(st, &dao, &dfr, &dev);
        }, more..., dirs, rot, cnt, val, bits, bent, ao8);
    }
};
// n rays or local pixels; fr: the rotation table of a frame call, or NULL
static AoArrays ao_arrays(size_t n, const srt_ao_desc* ao, const srt_ao_frame* fr, const srt_ao_frame_out& h) {
    const size_t words = n * ((ao->n_dirs + 31u) / 32u);
    const bool rotated = fr && fr->rot;
    return AoArrays{ query_in(ao->dirs, 3ull * ao->n_dirs), query_out(h.n_occluded, n), query_out(h.ao, n), query_out(h.occ_bits, words),
                     query_in(rotated ? fr->rot : nullptr, rotated ? 2ull * fr->rot_w * fr->rot_h : 0), query_out(h.bent, 3 * n), query_out(h.ao8, n),
                     rotated ? fr->rot_w : 0u, rotated ? fr->rot_h : 0u };
}

// hits: the hits a caller of srt_ao_hits brings, or NULL: srt_ao_rays
static int ao_impl(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao,
                   const srt_visibility* vis, int32_t* hit_id, float* t, const srt_ao_out* out, srt_stats* stats) {
    SRT_TRY(check_ao(s, n, rays, hits, flags, ao));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (!n || (hits && !stats && !ao_wanted(out))) return SRT_OK;
    const srt_ao_out h = out ? *out : srt_ao_out{};
    AoArrays a = ao_arrays(n, ao, nullptr, srt_ao_frame_out{ h.n_occluded, h.ao, h.occ_bits, nullptr, nullptr });
    auto o_hit = query_out(hit_id, n); auto o_t = query_out(t, n);
    auto i_rays = query_in(rays, 6ull * n); auto i_range = query_in(t_range, 2ull * n);
    auto i_hit = query_in(hits ? hits->hit_id : nullptr, n); auto i_t = query_in(hits ? hits->t : nullptr, n);
    SRT_TRY(a.round_trip(s, false, ao, [&](hipStream_t st, const srt_ao_desc* dao, const srt_ao_frame*, const srt_ao_frame_out* dev) {
        const QueryHits dh = { i_hit.on_device(), i_t.on_device() };
        const srt_ao_out dout = { dev->n_occluded, dev->ao, dev->occ_bits };
        return ao_device_impl(s, n, i_rays.on_device(), i_range.on_device(), hits ? &dh : nullptr, flags, dao, vis, st, o_hit.on_device(), o_t.on_device(), &dout,
                              stats != nullptr);
    }, o_hit, o_t, i_rays, i_range, i_hit, i_t));
    return stats ? query_stats(s, n, ao_wanted(out) ? ao->n_dirs : 0u, stats) : SRT_OK;      // (nothing wanted: no AO ray was walked)
}

// srt_render_ao / srt_render_ao_hits: as ao_impl, with n the call's local pixels and no rays to stage; primary_rays counts image pixels x
// the sub-samples walked
static int render_ao_impl(srt_scene* s, const srt_params* p, const QueryHits* hits, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr,
                          const srt_visibility* vis, int32_t* hit_id, float* t, const srt_ao_frame_out* out, srt_stats* stats) {
    SRT_TRY(check_render_ao(s, p, hits, flags, ao, fr));
    if (stats) std::memset(stats, 0, sizeof(*stats));
    const uint32_t n = srt_rows_owned(p) * srt_cols_owned(p);      // (< 2^32: check_render_ao)
    const bool wanted = ao_frame_wanted(out);
    if (!n || (!stats && !wanted && (hits || (!hit_id && !t)))) return SRT_OK;
    AoArrays a = ao_arrays(n, ao, fr, out ? *out : srt_ao_frame_out{});
    auto o_hit = query_out(hit_id, n); auto o_t = query_out(t, n);
    auto i_hit = query_in(hits ? hits->hit_id : nullptr, n); auto i_t = query_in(hits ? hits->t : nullptr, n);
    // (a tile deal's padding pixels are not written: what the query block holds there must not reach the caller)
    SRT_TRY(a.round_trip(s, p->block_cols != 0, ao, [&](hipStream_t st, const srt_ao_desc* dao, const srt_ao_frame* dfr, const srt_ao_frame_out* dev) {
        const QueryHits dh = { i_hit.on_device(), i_t.on_device() };
        return render_ao_device_impl(s, p, hits ? &dh : nullptr, flags, dao, fr ? dfr : nullptr, vis, st, o_hit.on_device(), o_t.on_device(), dev, stats != nullptr);
    }, o_hit, o_t, i_hit, i_t));
    if (!stats) return SRT_OK;
    SRT_TRY(query_stats(s, n, wanted ? ao->n_dirs : 0u, stats));      // (nothing wanted: no AO ray was walked)
    stats->primary_rays = pixels_owned(p) * (hits ? 1u : p->spp);
    return SRT_OK;
}
}      // extern "C++"

int srt_trace_rays_device(srt_scene* s, uint32_t n, const float* d_rays, uint32_t flags, void* stream, int32_t* d_hit_id, float* d_t, float* d_bary) {
    return guarded([&] { return trace_rays_device_impl(s, n, d_rays, nullptr, flags, (hipStream_t)stream, d_hit_id, d_t, d_bary, false, RayMask{}); });
}
int srt_trace_rays_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t flags, void* stream, int32_t* d_hit_id, float* d_t,
                                float* d_bary) {
    return guarded([&] { return trace_rays_device_impl(s, n, d_rays, d_t_range, flags, (hipStream_t)stream, d_hit_id, d_t, d_bary, false, RayMask{}); });
}
int srt_trace_rays(srt_scene* s, uint32_t n, const float* rays, uint32_t flags, int32_t* hit_id, float* t, float* bary, srt_stats* stats) {
    return guarded([&] { return trace_rays_impl(s, n, rays, nullptr, flags, hit_id, t, bary, stats, RayMask{}); });
}
int srt_trace_rays_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, int32_t* hit_id, float* t, float* bary, srt_stats* stats) {
    return guarded([&] { return trace_rays_impl(s, n, rays, t_range, flags, hit_id, t, bary, stats, RayMask{}); });
}
int srt_trace_rays_multi_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t k, uint32_t flags, void* stream, uint32_t* d_n_hits,
                                int32_t* d_hit_id, float* d_t, float* d_bary) {
    return guarded([&] { return trace_rays_multi_device_impl(s, n, d_rays, d_t_range, k, flags, (hipStream_t)stream, d_n_hits, d_hit_id, d_t, d_bary, false); });
}
int srt_trace_rays_multi(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t k, uint32_t flags, uint32_t* n_hits, int32_t* hit_id, float* t,
                         float* bary, srt_stats* stats) {
    return guarded([&] { return trace_rays_multi_impl(s, n, rays, t_range, k, flags, n_hits, hit_id, t, bary, stats); });
}
int srt_occluded_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_skip_obj, void* stream, uint8_t* d_occluded) {
    return guarded([&] { return occluded_device_impl(s, n, d_rays, nullptr, d_skip_obj, (hipStream_t)stream, d_occluded, RayMask{}); });
}
int srt_occluded_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const int32_t* d_skip_obj, void* stream, uint8_t* d_occluded) {
    return guarded([&] { return occluded_device_impl(s, n, d_rays, d_t_range, d_skip_obj, (hipStream_t)stream, d_occluded, RayMask{}); });
}
int srt_occluded(srt_scene* s, uint32_t n, const float* rays, const int32_t* skip_obj, uint8_t* occluded) {
    return guarded([&] { return occluded_impl(s, n, rays, nullptr, skip_obj, occluded, RayMask{}); });
}
int srt_occluded_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const int32_t* skip_obj, uint8_t* occluded) {
    return guarded([&] { return occluded_impl(s, n, rays, t_range, skip_obj, occluded, RayMask{}); });
}
int srt_shade_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const srt_params* p, void* stream, int32_t* d_hit_id, float* d_t,
                          float* d_rgb_linear, uint8_t* d_rgb8) {
    return guarded([&] { return shade_rays_device_impl(s, n, d_rays, nullptr, p, (hipStream_t)stream, d_hit_id, d_t, d_rgb_linear, d_rgb8, false); });
}
int srt_shade_rays_range_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, void* stream, int32_t* d_hit_id, float* d_t,
                                float* d_rgb_linear, uint8_t* d_rgb8) {
    return guarded([&] { return shade_rays_device_impl(s, n, d_rays, d_t_range, p, (hipStream_t)stream, d_hit_id, d_t, d_rgb_linear, d_rgb8, false); });
}
int srt_shade_rays(srt_scene* s, uint32_t n, const float* rays, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear, uint8_t* rgb8,
                   srt_stats* stats) {
    return guarded([&] { return shade_rays_impl(s, n, rays, nullptr, p, hit_id, t, rgb_linear, rgb8, stats); });
}
int srt_shade_rays_range(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, int32_t* hit_id, float* t, float* rgb_linear,
                         uint8_t* rgb8, srt_stats* stats) {
    return guarded([&] { return shade_rays_impl(s, n, rays, t_range, p, hit_id, t, rgb_linear, rgb8, stats); });
}
int srt_shade_paths_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path, void* stream,
                           float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return shade_paths_device_impl(s, n, d_rays, d_t_range, p, path, PathOptions{}, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_shade_paths(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, float* rgb_linear, uint8_t* rgb8,
                    const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return shade_paths_impl(s, n, rays, t_range, p, path, PathOptions{}, rgb_linear, rgb8, seg, stats); });
}
int srt_render_paths_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, void* stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return render_paths_device_impl(s, p, path, PathOptions{}, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_render_paths(srt_scene* s, const srt_params* p, const srt_path_desc* path, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return render_paths_impl(s, p, path, PathOptions{}, rgb_linear, rgb8, seg, stats); });
}
// The same four calls under a shadow rule (NULL: the call above, with its kernels)
int srt_shade_paths_shadow_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path,
                                  const srt_shadow_rule* shadow, void* stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return shade_paths_device_impl(s, n, d_rays, d_t_range, p, path, PathOptions{ .shadow = shadow }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_shade_paths_shadow(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                           float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return shade_paths_impl(s, n, rays, t_range, p, path, PathOptions{ .shadow = shadow }, rgb_linear, rgb8, seg, stats); });
}
int srt_render_paths_shadow_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, void* stream, float* d_rgb_linear,
                                   uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return render_paths_device_impl(s, p, path, PathOptions{ .shadow = shadow }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_render_paths_shadow(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, float* rgb_linear, uint8_t* rgb8,
                            const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return render_paths_impl(s, p, path, PathOptions{ .shadow = shadow }, rgb_linear, rgb8, seg, stats); });
}
// Visibility masks: the closest-hit and occlusion calls with a mask per ray, the four path calls with a mask per ray kind (NULL vis: the
// _shadow call above, with its kernels)
int srt_trace_rays_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const uint32_t* d_ray_mask, uint32_t flags, void* stream,
                                 int32_t* d_hit_id, float* d_t, float* d_bary) {
    return guarded([&] { return trace_rays_device_impl(s, n, d_rays, d_t_range, flags, (hipStream_t)stream, d_hit_id, d_t, d_bary, false, RayMask{ .masked = true, .words = d_ray_mask }); });
}
int srt_trace_rays_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const uint32_t* ray_mask, uint32_t flags, int32_t* hit_id, float* t,
                          float* bary, srt_stats* stats) {
    return guarded([&] { return trace_rays_impl(s, n, rays, t_range, flags, hit_id, t, bary, stats, RayMask{ .masked = true, .words = ray_mask }); });
}
int srt_occluded_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const uint32_t* d_ray_mask, const int32_t* d_skip_obj, void* stream,
                               uint8_t* d_occluded) {
    return guarded([&] { return occluded_device_impl(s, n, d_rays, d_t_range, d_skip_obj, (hipStream_t)stream, d_occluded, RayMask{ .masked = true, .words = d_ray_mask }); });
}
int srt_occluded_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const uint32_t* ray_mask, const int32_t* skip_obj, uint8_t* occluded) {
    return guarded([&] { return occluded_impl(s, n, rays, t_range, skip_obj, occluded, RayMask{ .masked = true, .words = ray_mask }); });
}
int srt_shade_paths_masked_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path,
                                  const srt_shadow_rule* shadow, const srt_visibility* vis, void* stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return shade_paths_device_impl(s, n, d_rays, d_t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_shade_paths_masked(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                           const srt_visibility* vis, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return shade_paths_impl(s, n, rays, t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis }, rgb_linear, rgb8, seg, stats); });
}
int srt_render_paths_masked_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis, void* stream,
                                   float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return render_paths_device_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_render_paths_masked(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis, float* rgb_linear,
                            uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return render_paths_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis }, rgb_linear, rgb8, seg, stats); });
}
// Refracting paths: the four path calls with a refraction table after the masks (no table: the _masked call above, with its kernels)
int srt_shade_paths_refract_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path,
                                   const srt_shadow_rule* shadow, const srt_visibility* vis, const srt_refraction* refr, void* stream, float* d_rgb_linear, uint8_t* d_rgb8,
                                   const srt_path_out* seg) {
    return guarded([&] { return shade_paths_device_impl(s, n, d_rays, d_t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_shade_paths_refract(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                            const srt_visibility* vis, const srt_refraction* refr, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return shade_paths_impl(s, n, rays, t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr }, rgb_linear, rgb8, seg, stats); });
}
int srt_render_paths_refract_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis,
                                    const srt_refraction* refr, void* stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return render_paths_device_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_render_paths_refract(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis,
                             const srt_refraction* refr, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return render_paths_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr }, rgb_linear, rgb8, seg, stats); });
}
// Fresnel split: the four path calls with a Fresnel table after the refraction table (no f0, or no ior: the _refract call above, with its kernels)
int srt_shade_paths_fresnel_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, const srt_params* p, const srt_path_desc* path,
                                   const srt_shadow_rule* shadow, const srt_visibility* vis, const srt_refraction* refr, const srt_fresnel* fres, void* stream,
                                   float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return shade_paths_device_impl(s, n, d_rays, d_t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr, .fres = fres }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_shade_paths_fresnel(srt_scene* s, uint32_t n, const float* rays, const float* t_range, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow,
                            const srt_visibility* vis, const srt_refraction* refr, const srt_fresnel* fres, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg,
                            srt_stats* stats) {
    return guarded([&] { return shade_paths_impl(s, n, rays, t_range, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr, .fres = fres }, rgb_linear, rgb8, seg, stats); });
}
int srt_render_paths_fresnel_device(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis,
                                    const srt_refraction* refr, const srt_fresnel* fres, void* stream, float* d_rgb_linear, uint8_t* d_rgb8, const srt_path_out* seg) {
    return guarded([&] { return render_paths_device_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr, .fres = fres }, (hipStream_t)stream, d_rgb_linear, d_rgb8, seg, false); });
}
int srt_render_paths_fresnel(srt_scene* s, const srt_params* p, const srt_path_desc* path, const srt_shadow_rule* shadow, const srt_visibility* vis,
                             const srt_refraction* refr, const srt_fresnel* fres, float* rgb_linear, uint8_t* rgb8, const srt_path_out* seg, srt_stats* stats) {
    return guarded([&] { return render_paths_impl(s, p, path, PathOptions{ .shadow = shadow, .vis = vis, .refr = refr, .fres = fres }, rgb_linear, rgb8, seg, stats); });
}

int srt_surface_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t flags, void* stream, int32_t* d_hit_id, float* d_t,
                            const srt_surface_out* out) {
    return guarded([&] { return surface_rays_device_impl(s, n, d_rays, d_t_range, flags, (hipStream_t)stream, d_hit_id, d_t, out, false); });
}
int srt_surface_rays(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, int32_t* hit_id, float* t, const srt_surface_out* out,
                     srt_stats* stats) {
    return guarded([&] { return surface_rays_impl(s, n, rays, t_range, flags, hit_id, t, out, stats); });
}
int srt_surface_hits_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_hit_id, const float* d_t, uint32_t flags, void* stream,
                            const srt_surface_out* out) {
    return guarded([&] { return surface_hits_device_impl(s, n, d_rays, d_hit_id, d_t, flags, (hipStream_t)stream, out); });
}
int srt_surface_hits(srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t, uint32_t flags, const srt_surface_out* out) {
    return guarded([&] { return surface_hits_impl(s, n, rays, hit_id, t, flags, out); });
}

int srt_ao_rays_device(srt_scene* s, uint32_t n, const float* d_rays, const float* d_t_range, uint32_t flags, const srt_ao_desc* ao, const srt_visibility* vis, void* stream,
                       int32_t* d_hit_id, float* d_t, const srt_ao_out* out) {
    return guarded([&] { return ao_device_impl(s, n, d_rays, d_t_range, nullptr, flags, ao, vis, (hipStream_t)stream, d_hit_id, d_t, out, false); });
}
int srt_ao_rays(srt_scene* s, uint32_t n, const float* rays, const float* t_range, uint32_t flags, const srt_ao_desc* ao, const srt_visibility* vis, int32_t* hit_id, float* t,
                const srt_ao_out* out, srt_stats* stats) {
    return guarded([&] { return ao_impl(s, n, rays, t_range, nullptr, flags, ao, vis, hit_id, t, out, stats); });
}
int srt_ao_hits_device(srt_scene* s, uint32_t n, const float* d_rays, const int32_t* d_hit_id, const float* d_t, uint32_t flags, const srt_ao_desc* ao,
                       const srt_visibility* vis, void* stream, const srt_ao_out* out) {
    const QueryHits hits = { d_hit_id, d_t };
    return guarded([&] { return ao_device_impl(s, n, d_rays, nullptr, &hits, flags, ao, vis, (hipStream_t)stream, nullptr, nullptr, out, false); });
}
int srt_ao_hits(srt_scene* s, uint32_t n, const float* rays, const int32_t* hit_id, const float* t, uint32_t flags, const srt_ao_desc* ao, const srt_visibility* vis,
                const srt_ao_out* out, srt_stats* stats) {
    const QueryHits hits = { hit_id, t };
    return guarded([&] { return ao_impl(s, n, rays, nullptr, &hits, flags, ao, vis, nullptr, nullptr, out, stats); });
}
int srt_render_ao_device(srt_scene* s, const srt_params* p, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr, const srt_visibility* vis, void* stream,
                         int32_t* d_hit_id, float* d_t, const srt_ao_frame_out* out) {
    return guarded([&] { return render_ao_device_impl(s, p, nullptr, flags, ao, fr, vis, (hipStream_t)stream, d_hit_id, d_t, out, false); });
}
int srt_render_ao(srt_scene* s, const srt_params* p, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr, const srt_visibility* vis, int32_t* hit_id, float* t,
                  const srt_ao_frame_out* out, srt_stats* stats) {
    return guarded([&] { return render_ao_impl(s, p, nullptr, flags, ao, fr, vis, hit_id, t, out, stats); });
}
int srt_render_ao_hits_device(srt_scene* s, const srt_params* p, const int32_t* d_hit_id, const float* d_t, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr,
                              const srt_visibility* vis, void* stream, const srt_ao_frame_out* out) {
    const QueryHits hits = { d_hit_id, d_t };
    return guarded([&] { return render_ao_device_impl(s, p, &hits, flags, ao, fr, vis, (hipStream_t)stream, nullptr, nullptr, out, false); });
}
int srt_render_ao_hits(srt_scene* s, const srt_params* p, const int32_t* hit_id, const float* t, uint32_t flags, const srt_ao_desc* ao, const srt_ao_frame* fr,
                       const srt_visibility* vis, const srt_ao_frame_out* out, srt_stats* stats) {
    const QueryHits hits = { hit_id, t };
    return guarded([&] { return render_ao_impl(s, p, &hits, flags, ao, fr, vis, nullptr, nullptr, out, stats); });
}

int srt_closest_points_device(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t flags, void* stream,
                              const srt_point_out* out) {
    return guarded([&] { return closest_points_device_impl(s, n, d_points, d_radius, d_point_mask, flags, (hipStream_t)stream, out, false); });
}
int srt_closest_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t flags, const srt_point_out* out,
                       srt_stats* stats) {
    return guarded([&] { return closest_points_impl(s, n, points, radius, point_mask, flags, out, stats); });
}

int srt_nearest_points_device(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t flags, void* stream,
                              const srt_point_out* out) {
    return guarded([&] { return closest_points_device_impl(s, n, d_points, d_radius, d_point_mask, flags, (hipStream_t)stream, out, false, true); });
}
int srt_nearest_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t flags, const srt_point_out* out,
                       srt_stats* stats) {
    return guarded([&] { return closest_points_impl(s, n, points, radius, point_mask, flags, out, stats, true); });
}

int srt_signed_points_device(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, const srt_sign* sign, uint32_t flags,
                             void* stream, const srt_point_out* out, const srt_sign_out* sout) {
    return guarded([&] { return signed_points_device_impl(s, n, d_points, d_radius, d_point_mask, sign, flags, (hipStream_t)stream, out, sout, false); });
}
int srt_signed_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, const srt_sign* sign, uint32_t flags,
                      const srt_point_out* out, const srt_sign_out* sout, srt_stats* stats) {
    return guarded([&] { return signed_points_impl(s, n, points, radius, point_mask, sign, flags, out, sout, stats); });
}

int srt_closest_points_multi_device(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t k, uint32_t flags,
                                    void* stream, const srt_point_multi_out* out) {
    return guarded([&] { return points_multi_device_impl(s, n, d_points, d_radius, d_point_mask, k, flags, (hipStream_t)stream, out, false, false); });
}
int srt_closest_points_multi(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t k, uint32_t flags,
                             const srt_point_multi_out* out, srt_stats* stats) {
    return guarded([&] { return points_multi_impl(s, n, points, radius, point_mask, k, flags, out, stats, false); });
}
int srt_nearest_points_multi_device(srt_scene* s, uint32_t n, const float* d_points, const float* d_radius, const uint32_t* d_point_mask, uint32_t k, uint32_t flags,
                                    void* stream, const srt_point_multi_out* out) {
    return guarded([&] { return points_multi_device_impl(s, n, d_points, d_radius, d_point_mask, k, flags, (hipStream_t)stream, out, false, true); });
}
int srt_nearest_points_multi(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t k, uint32_t flags,
                             const srt_point_multi_out* out, srt_stats* stats) {
    return guarded([&] { return points_multi_impl(s, n, points, radius, point_mask, k, flags, out, stats, true); });
}
int srt_closest_segments_device(srt_scene* s, uint32_t n, const float* d_segments, const float* d_radius, const uint32_t* d_seg_mask, uint32_t flags,
                                void* stream, const srt_segment_out* out) {
    return guarded([&] { return segments_device_impl(s, n, d_segments, d_radius, d_seg_mask, flags, (hipStream_t)stream, out, false); });
}
int srt_closest_segments(srt_scene* s, uint32_t n, const float* segments, const float* radius, const uint32_t* seg_mask, uint32_t flags,
                         const srt_segment_out* out, srt_stats* stats) {
    return guarded([&] { return segments_impl(s, n, segments, radius, seg_mask, flags, out, stats); });
}

void* srt_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void srt_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- known-answer entry points (device leaf functions on caller vectors; host pointers in and out) ----
namespace {
struct DevBuf : DevArray<char> {
    int alloc(size_t bytes) { HIP_TRY(reserve(bytes ? bytes : 1)); return SRT_OK; }
    int up(const void* h, size_t bytes) { SRT_TRY(alloc(bytes)); HIP_TRY(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice)); return SRT_OK; }
    int down(void* h, size_t bytes) { HIP_TRY(hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost)); return SRT_OK; }
};
}

int srt_kat_ray_aabb(int device, uint32_t n, const float* ray_od, const float* box, uint8_t* exact, uint8_t* branchless,
                     uint8_t* filtered, uint8_t* ambiguous) {
    if (!n || !ray_od || !box || !exact || !branchless || !filtered || !ambiguous) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf r, b, o0, o1, o2, o3;
    SRT_TRY(r.up(ray_od, (size_t)n * 24)); SRT_TRY(b.up(box, (size_t)n * 24));
    SRT_TRY(o0.alloc(n)); SRT_TRY(o1.alloc(n)); SRT_TRY(o2.alloc(n)); SRT_TRY(o3.alloc(n));
    hipLaunchKernelGGL(k_kat_ray_aabb, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)r.p, (const float*)b.p,
                       (uint8_t*)o0.p, (uint8_t*)o1.p, (uint8_t*)o2.p, (uint8_t*)o3.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(o0.down(exact, n)); SRT_TRY(o1.down(branchless, n)); SRT_TRY(o2.down(filtered, n)); SRT_TRY(o3.down(ambiguous, n));
    return SRT_OK;
}

int srt_kat_ray_triangle(int device, uint32_t n, const float* ray_od, const float* tri_points, float* t) {
    if (!n || !ray_od || !tri_points || !t) return SRT_ERR_ARG;
    return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    std::vector<DevTri> tris(n);
    for (uint32_t i = 0; i < n; i++) tris[i] = derive_triangle(tri_points + 12 * (size_t)i);
    DevBuf r, q, o;
    SRT_TRY(r.up(ray_od, (size_t)n * 24)); SRT_TRY(q.up(tris.data(), (size_t)n * sizeof(DevTri))); SRT_TRY(o.alloc((size_t)n * 4));
    hipLaunchKernelGGL(k_kat_ray_triangle, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)r.p, (const DevTri*)q.p, (float*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    return o.down(t, (size_t)n * 4);
    });
}

int srt_kat_ray_triangle_origin(int device, uint32_t n, const float* dir, const float* tri_points, float* t) {
    if (!n || !dir || !tri_points || !t) return SRT_ERR_ARG;
    return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    std::vector<DevTriO> tris_o(n);           // both records as srt_scene_create derives them
    for (uint32_t i = 0; i < n; i++) tris_o[i] = derive_triangle_origin(derive_triangle(tri_points + 12 * (size_t)i));
    DevBuf r, q, o;
    SRT_TRY(r.up(dir, (size_t)n * 12)); SRT_TRY(q.up(tris_o.data(), (size_t)n * sizeof(DevTriO))); SRT_TRY(o.alloc((size_t)n * 4));
    hipLaunchKernelGGL(k_kat_ray_triangle_origin, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)r.p, (const DevTriO*)q.p, (float*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    return o.down(t, (size_t)n * 4);
    });
}

int srt_kat_barycentric(int device, uint32_t n, const float* in15, float* out3) {
    if (!n || !in15 || !out3) return SRT_ERR_ARG;
    return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    std::vector<DevTri> tris(n);
    for (uint32_t i = 0; i < n; i++) tris[i] = derive_triangle(in15 + 15 * (size_t)i);
    DevBuf a, q, o;
    SRT_TRY(a.up(in15, (size_t)n * 60)); SRT_TRY(q.up(tris.data(), (size_t)n * sizeof(DevTri))); SRT_TRY(o.alloc((size_t)n * 12));
    hipLaunchKernelGGL(k_kat_barycentric, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, (const DevTri*)q.p, (float*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    return o.down(out3, (size_t)n * 12);
    });
}

int srt_kat_phong(int device, uint32_t n, const float* in28, float* rgb) {
    if (!n || !in28 || !rgb) return SRT_ERR_ARG;
    return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    std::vector<DevTri> tris(n);
    for (uint32_t i = 0; i < n; i++) tris[i] = derive_triangle(in28 + 28 * (size_t)i + 6);
    DevBuf a, q, o;
    SRT_TRY(a.up(in28, (size_t)n * 28 * 4)); SRT_TRY(q.up(tris.data(), (size_t)n * sizeof(DevTri))); SRT_TRY(o.alloc((size_t)n * 12));
    hipLaunchKernelGGL(k_kat_phong, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, (const DevTri*)q.p, (float*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    return o.down(rgb, (size_t)n * 12);
    });
}

int srt_kat_interp_normal(int device, uint32_t n, const float* in12, float* out3) {
    if (!n || !in12 || !out3) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf a, o;
    SRT_TRY(a.up(in12, (size_t)n * 48)); SRT_TRY(o.alloc((size_t)n * 12));
    hipLaunchKernelGGL(k_kat_interp_normal, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, (float*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    return o.down(out3, (size_t)n * 12);
}

int srt_kat_pow(int device, uint32_t n, const float* x, const float* y, float* fast, float* lib) {
    if (!n || !x || !y || !fast || !lib) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf a, b, o, o2;
    SRT_TRY(a.up(x, (size_t)n * 4)); SRT_TRY(b.up(y, (size_t)n * 4)); SRT_TRY(o.alloc((size_t)n * 4)); SRT_TRY(o2.alloc((size_t)n * 4));
    hipLaunchKernelGGL(k_kat_pow, dim3((n + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, (const float*)b.p, (float*)o.p, (float*)o2.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(o.down(fast, (size_t)n * 4));
    return o2.down(lib, (size_t)n * 4);
}

// out[0] = VALU wave-instructions one SIMD issues per cycle: per SIMD (XCC / SE / SH / CU / SIMD of HW_ID), the instructions of the
// waves that ran on it over the cycles from its first wave's start to its last wave's end (s_memtime), median over the SIMDs;
// out[1] = shader clock in GHz during the run (s_memtime against the 100 MHz s_memrealtime); out[2] = the same rate from the
// chip-wide span (all waves' instructions / (SIMDs x clock x (last end - first start))), which includes launch ramp and tail;
// out[3] = waves per SIMD (median) that shared a SIMD during the run.
int srt_debug_valu_rate(int device, uint32_t iters, double* out) {
    if (!iters || !out) return SRT_ERR_ARG;
    return guarded([&]() -> int {
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    const uint32_t n_cu = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    const uint32_t wgs = n_cu * 8u;                            // 8 workgroups of 4 waves per CU = 8 waves per SIMD, all resident
    DevBuf sink, st;
    SRT_TRY(sink.alloc((size_t)wgs * 256 * 4)); SRT_TRY(st.alloc((size_t)wgs * 4 * 8 * 8));
    for (int rep = 0; rep < 2; rep++) {                        // the first launch warms the clock
        static const bool packed = std::getenv("SRT_VALU_PACKED") != nullptr;        // measure v_pk_fma_f32 instead (same instruction count)
        if (packed) hipLaunchKernelGGL(k_valu_rate<true>, dim3(wgs), dim3(256), 0, 0, iters, (float*)sink.p, (unsigned long long*)st.p);
        else        hipLaunchKernelGGL(k_valu_rate<false>, dim3(wgs), dim3(256), 0, 0, iters, (float*)sink.p, (unsigned long long*)st.p);
        HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    }
    std::vector<unsigned long long> h((size_t)wgs * 32);
    SRT_TRY(st.down(h.data(), h.size() * 8));
    const size_t nw = (size_t)wgs * 4;
    std::vector<double> clk(nw);
    unsigned long long rmin = ~0ull, rmax = 0;
    struct Simd { unsigned long long t0 = ~0ull, t1 = 0; uint32_t waves = 0; };
    std::map<unsigned long long, Simd> simds;
    for (size_t w = 0; w < nw; w++) {
        const unsigned long long t0 = h[8 * w], t1 = h[8 * w + 1], r0 = h[8 * w + 2], r1 = h[8 * w + 3], where = h[8 * w + 4];
        clk[w] = (double)(t1 - t0) / (double)(r1 - r0) * 0.1;      // GHz: ticks per 10 ns
        if (r0 < rmin) rmin = r0;
        if (r1 > rmax) rmax = r1;
        Simd& sd = simds[((where >> 32) & 0xfull) << 16 | (where & 0x7f30ull)];      // XCC | SE, SH, CU, SIMD bits of HW_ID
        if (t0 < sd.t0) sd.t0 = t0;
        if (t1 > sd.t1) sd.t1 = t1;
        sd.waves++;
    }
    std::vector<double> rate, share;
    for (const auto& kv : simds) { rate.push_back(64.0 * iters * kv.second.waves / (double)(kv.second.t1 - kv.second.t0)); share.push_back((double)kv.second.waves); }
    std::nth_element(rate.begin(), rate.begin() + rate.size() / 2, rate.end());
    std::nth_element(share.begin(), share.begin() + share.size() / 2, share.end());
    std::nth_element(clk.begin(), clk.begin() + nw / 2, clk.end());
    out[0] = rate[rate.size() / 2];
    out[1] = clk[nw / 2];
    out[2] = (64.0 * iters * (double)nw) / ((double)simds.size() * out[1] * 1e9 * ((double)(rmax - rmin) * 1e-8));
    out[3] = share[share.size() / 2];
    return SRT_OK;
    });
}

int srt_kat_tonemap(int device, uint32_t n, const float* lin, float reinhard, float gamma, float* tone, int32_t* q) {
    if (!n || !lin || !tone || !q) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf a, o, o2;
    SRT_TRY(a.up(lin, (size_t)n * 12)); SRT_TRY(o.alloc((size_t)n * 12)); SRT_TRY(o2.alloc((size_t)n * 12));
    hipLaunchKernelGGL(k_kat_tonemap, dim3((3 * n + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, reinhard, gamma, (float*)o.p, (int32_t*)o2.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(o.down(tone, (size_t)n * 12));
    return o2.down(q, (size_t)n * 12);
}

int srt_kat_tone_filter(int device, uint32_t n, const float* lin, float reinhard, float gamma, int32_t* q, int32_t* q_filter, uint8_t* decided) {
    if (!n || !lin || !q || !q_filter || !decided) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    DevBuf a, o, o2, o3;
    SRT_TRY(a.up(lin, (size_t)n * 4)); SRT_TRY(o.alloc((size_t)n * 4)); SRT_TRY(o2.alloc((size_t)n * 4)); SRT_TRY(o3.alloc((size_t)n));
    const uint32_t triples = (uint32_t)(((uint64_t)n + 2) / 3);
    hipLaunchKernelGGL(k_kat_tone_filter, dim3((triples + 255) / 256), dim3(256), 0, 0, n, (const float*)a.p, reinhard, gamma, (int32_t*)o.p, (int32_t*)o2.p, (uint8_t*)o3.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(o.down(q, (size_t)n * 4)); SRT_TRY(o2.down(q_filter, (size_t)n * 4));
    return o3.down(decided, (size_t)n);
}

int srt_kat_tone_filter_sweep(int device, uint32_t first_bits, uint32_t last_bits, float reinhard, float gamma, double* out) {
    if (!out || last_bits < first_bits) return SRT_ERR_ARG;
    HIP_TRY(hipSetDevice(device));
    const unsigned long long count = (unsigned long long)last_bits - first_bits + 1ull, zero[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    unsigned long long h[6];
    DevBuf o;
    SRT_TRY(o.up(zero, sizeof(zero)));
    const unsigned long long wgs = (count + 255ull) / 256ull;
    hipLaunchKernelGGL(k_kat_tone_sweep, dim3((uint32_t)(wgs < 2048ull ? wgs : 2048ull)), dim3(256), 0, 0, first_bits, count, reinhard, gamma, (unsigned long long*)o.p);
    HIP_TRY(hipGetLastError()); HIP_TRY(hipDeviceSynchronize());
    SRT_TRY(o.down(h, sizeof(h)));
    for (int k = 0; k < 4; k++) out[k] = (double)h[k];
    for (int k = 4; k < 6; k++) std::memcpy(out + k, h + k, 8);
    return SRT_OK;
}

} // extern "C"
