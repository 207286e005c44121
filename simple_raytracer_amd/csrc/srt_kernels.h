// srt_kernels.h -- the HIP kernels of the ray-trace path (gfx950).  Included by srt_hip.hip only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "srt_device.h"
#include "srt_tile_spans.h"

using namespace srt;

// =================================================================================================
// Device-side scene / params views (passed by value in kernarg SGPRs)
// =================================================================================================
struct DevScene {
    const DevNode* nodes;
    const DevWide* wide;          // inner nodes with both children's boxes (node-queue kernels), pre-order over inner nodes
    const int32_t* obj_root_info; // n_objects: what an object's ROOT is -- ~(its DevWide index) < 0, or a leaf's (first << 5 | count)
    const DevNode* root_nodes;    // n_objects: a copy of every object's root record, contiguous -- the root tests of a tile read them with
                                  // INDEPENDENT loads (index = object) instead of obj_range[ob] -> nodes[root], one dependent pair per object
    const float* scene_box;       // 8 floats (min.xyz max.x | max.yz - -): the union of the objects' root boxes, laid out like a node's box
    const DevTri* tris;
    const DevTriO* tris_o;        // the same triangles as rays from the origin test them (closest-hit phase)
    const int32_t* tri_obj;
    const int32_t* tri_tex;       // may be null (no textures)
    const float* tri_tc;          // n_tris x 6, may be null
    const float* tri_normals;     // n_tris x 9 vertex normals, may be null (SRT_FLAG_SMOOTH_NORMALS only)
    const float* obj_color;       // n_objects x 3
    const float* obj_mat;         // n_objects x 3
    const int2* obj_range;        // n_objects: [first node, end node) in pre-order
    const int32_t* obj_tri_first; // n_objects + 1: first triangle id of each object (triangles are numbered object by object)
    const uint8_t* tex;
    const unsigned long long* tex_off;
    const uint32_t* tex_w;
    const uint32_t* tex_h;
    const unsigned long long* tex_size;
    uint32_t n_nodes, n_tris, n_objects;
    uint32_t pad_;                // explicit: the struct travels by value inside FrameTab, whose size is asserted: no implicit padding anywhere
};
static_assert(sizeof(DevScene) == 20 * 8 + 16, "DevScene has no implicit padding");

struct DevParams {
    uint32_t W, H, rows;          // W = width of the rows this call writes (local width); rows of them
    uint32_t Wimg;                // image width (== W unless the frame is dealt in tiles: col_block > 0)
    uint32_t col_block;           // srt_params.block_cols: 0 = full-width scanline blocks
    uint32_t block_rows, block_first, block_stride;
    int32_t i0, j0;
    float sub_x, sub_y;           // sub-pixel offset added to dir.xy (0 for the reference's one ray per pixel)
    float focal;
    uint32_t n_lights;
    const float* lights;          // device, n_lights x 3
    float shadow_div, reinhard, gamma;
    uint32_t bg;                  // r | g << 8 | b << 16
    uint32_t smooth;              // interpolateNormal mode (simple_raytracer.cpp:132-140,162)
    uint32_t xcd_rows;            // host-side choice of the k_trace_nq build that deals whole tile rows to XCDs
    uint32_t shadow_px_major;     // shadow bits as the packet shadow kernel writes them: per pixel one u64 per 64 light samples
    uint32_t cam;                 // camera mode (srt_params.ray_matrix, an extension): rays are taken into the scene's space
    float cm[12];                 // columns 0..2 (direction) and 3 (origin) of that matrix, xyz each
    uint32_t exp, heavy_steps;    // heavy_steps: packet shadow walks of that many steps make their quadrant a HEAVY one in the next frame's list (0 = off).  exp: experiment switches (A/B variants, wave-uniform branches): bit 0 = queue pushes in LANE order (the round-2 form) instead of node-major
    uint32_t pk_units, pk_take;   // packet shadow kernel: units a wave should have to walk -- surplus waves of the fixed-size grid leave at once (0 = all stay) --, and how many unit numbers one atomic takes
};
static_assert(sizeof(DevParams) == 160, "DevParams has no implicit padding");
constexpr uint32_t EXP_EXACT_TONE = 16u;      // DevParams.exp: store_pixel skips the tone map's filter and runs the exact functions on every channel (variant 63, A/B)

// counters[0] hit pixels, [1]/[2] node/triangle tests of the closest-hit kernel, [3]/[4] of the shade kernel
__device__ __forceinline__ void wave_add(unsigned long long* ctr, unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(ctr, v);
}

// bits of a ballot below this lane: its rank among the lanes that voted
__device__ __forceinline__ uint32_t lane_prefix(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// The lane id once more, opaque to the compiler.  What a lane derives from it -- the LDS addresses of its own slots (lane << 2, lane * 16
// + base), lane >> 4 -- is one or two VALU operations away; derived from the plain lane id it is hoisted out of every loop and, at seven
// waves per SIMD, kept in scratch across the walks in between (a reload = an L2 round trip on the wave's dependent chain).  Derived from
// this copy inside a loop it is formed where it is used.
__device__ __forceinline__ uint32_t lane_again(uint32_t lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// Hit-pixel statistic without a hot atomic: one word takes ~12 ns per atomic, so 32 k waves adding to one
// address would serialise for ~0.4 ms.  64 shards, 64 B apart, summed on the host.
constexpr int HIT_SHARDS = 64;
constexpr int CTR_HIT_BASE = 8;                  // counters[8 + 8*shard]
__device__ __forceinline__ void count_hits(unsigned long long* counters, bool is_hit, uint32_t tile_index) {
    const unsigned long long m = __ballot(is_hit);
    if ((threadIdx.x & 63) == 0 && m) {
        const uint32_t shard = tile_index & (HIT_SHARDS - 1);
        atomicAdd(counters + CTR_HIT_BASE + 8 * shard, (unsigned long long)__popcll(m));
    }
}

constexpr int NCTR = 8 + 8 * HIT_SHARDS;        // [1..4] node / triangle tests, [8 + 8*shard] hit counts
// The last kernel of a render clears the counter set of the next render (two sets alternate).
__device__ __forceinline__ void zero_next_counters(unsigned long long* next) {
    if (blockIdx.x == 0 && blockIdx.y == 0)
        for (int i = threadIdx.x; i < NCTR; i += 256) next[i] = 0ull;
}

// local output row -> image row under block-cyclic scanline ownership (include/srt.h srt_params)
__device__ __forceinline__ uint32_t image_row(const DevParams& p, uint32_t r) {
    if (p.col_block) return r;                                             // tiles dealt in two dimensions: every call owns tiles in every row
    if (p.block_stride == 1) return p.block_first * p.block_rows + r;      // consecutive blocks (whole frame on one device): no division
    if ((p.block_rows & (p.block_rows - 1u)) == 0u) {                      // 8, 16, 32 ... rows a block (the usual deal): a shift instead of the
        const uint32_t sh = 31u - (uint32_t)__builtin_clz(p.block_rows);   // ~35-instruction integer division every lane would run
        return (((r >> sh) * p.block_stride + p.block_first) << sh) + (r & (p.block_rows - 1u));
    }
    return ((r / p.block_rows) * p.block_stride + p.block_first) * p.block_rows + (r % p.block_rows);
}
// local output column -> image column (include/srt.h srt_params.block_cols); y = image row
__device__ __forceinline__ uint32_t image_col(const DevParams& p, uint32_t px, uint32_t y) {
    if (!p.col_block) return px;
    const uint32_t off = (p.block_first + p.block_stride - (y / p.block_rows) % p.block_stride) % p.block_stride;     // owned bx = first - by (mod stride)
    return ((px / p.col_block) * p.block_stride + off) * p.col_block + px % p.col_block;
}
// is local pixel (px, r) a pixel of the image (not beyond the buffer, not padding of a tile deal)?
__device__ __forceinline__ bool pixel_live(const DevParams& p, uint32_t px, uint32_t r) {
    return px < p.W && r < p.rows && (!p.col_block || image_col(p, px, r) < p.Wimg);
}
// sendRaysAndIntersectPointsColors:511-517: dir = (i, j, focal), i = x + int(-W/2); px = LOCAL column, y = image row.
// Camera mode (extension): the same ray in the scene's space, (M[0] * dx + M[1] * dy) + M[2] * dz, leaving M[3].xyz.
__device__ __forceinline__ V3 primary_dir(const DevParams& p, uint32_t px, uint32_t y) {
    const V3 d = mk((float)(p.i0 + (int)image_col(p, px, y)) + p.sub_x, (float)(p.j0 + (int)y) + p.sub_y, p.focal);
    if (!p.cam) return d;
    return mk((p.cm[0] * d.x + p.cm[3] * d.y) + p.cm[6] * d.z, (p.cm[1] * d.x + p.cm[4] * d.y) + p.cm[7] * d.z,
              (p.cm[2] * d.x + p.cm[5] * d.y) + p.cm[8] * d.z);
}
__device__ __forceinline__ V3 ray_origin(const DevParams& p) {
    return p.cam ? mk(p.cm[9], p.cm[10], p.cm[11]) : mk(0.0f, 0.0f, 0.0f);
}
// The parameters of a WHOLE frame in the reference's ray form, as constants (the WHOLE kernels: k_trace_nq_whole8_spans,
// k_shade_tile_whole_spans): no column tiles, consecutive scanline blocks from row 0, one ray per pixel, no camera matrix, no experiment
// switch -- what plan_frame asserts before it names such a kernel.  Every function above is inlined, so with these fields constant
// image_row(p, r) is r, image_col is px, pixel_live is px < p.W && r < p.rows, primary_dir is ((float)(p.i0 + px), (float)(p.j0 + r),
// p.focal) -- (float)n + 0.0f has the bits of (float)n for every integer n, 0 included: a conversion never gives -0.0 --, ray_origin is the
// zero vector and every p.exp arm is gone, and the kernel neither loads these words nor keeps them in registers.
__device__ __forceinline__ DevParams whole_frame_params(const DevParams& p) {
    DevParams q = p;
    q.Wimg = p.W; q.col_block = 0u; q.block_first = 0u; q.block_stride = 1u;
    q.sub_x = 0.0f; q.sub_y = 0.0f;
    q.cam = 0u;
    for (int i = 0; i < 12; i++) q.cm[i] = 0.0f;
    q.exp = 0u;
    return q;
}
// a body's parameters and scene: the caller's, or (WHOLE) a copy -- the parameters in their whole-frame form --, whose words the body
// may then ask for where it wants them
template <bool WHOLE>
__device__ __forceinline__ decltype(auto) frame_params(const DevParams& p) {
    if constexpr (WHOLE) return whole_frame_params(p); else return (p);
}
template <bool WHOLE>
__device__ __forceinline__ decltype(auto) frame_scene(const DevScene& s) {
    if constexpr (WHOLE) return DevScene(s); else return (s);
}

// 16x16 pixel tile per 256-thread workgroup, one 8x8 sub-tile per wavefront: the 64 primary rays of
// a wave are neighbours, so they walk the same top-of-tree nodes (loads of one node by many lanes
// coalesce into one 32 B fetch) and diverge only deep in the tree.
__device__ __forceinline__ bool tile_pixel(const DevParams& p, uint32_t& px, uint32_t& r) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    px = blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    r  = blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    return pixel_live(p, px, r);
}

// A finished pixel, wherever it comes from: the light sum as it is into rgb_linear, and into rgb8 Reinhard + gamma (:391-398), the
// quantiser (:447-449) and the black -> background rule (:518, drawImage:476-487).  lit = false (a miss, a ray without a hit): no tone
// map, the background bytes.  Either output may be absent.  The three channels' quantised tone map is quant_tone's (srt_device.h): decided
// by the f32 filter where its margin allows, by quant1(tone1()) where not -- or everywhere under exp & EXP_EXACT_TONE; the same bytes.
__device__ __forceinline__ void store_pixel(float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, const size_t pix, const V3 sum, const bool lit,
                                            const float reinhard, const float gamma, const uint32_t bg, const uint32_t exp) {
    if (rgb_linear) { rgb_linear[pix * 3] = sum.x; rgb_linear[pix * 3 + 1] = sum.y; rgb_linear[pix * 3 + 2] = sum.z; }
    if (rgb8) {
        int q[3] = {0, 0, 0};
        if (lit) { const float c[3] = {sum.x, sum.y, sum.z}; quant_tone<3>(c, reinhard, gamma, (exp & EXP_EXACT_TONE) != 0u, q); }
        if ((q[0] | q[1] | q[2]) == 0) { q[0] = bg & 255; q[1] = (bg >> 8) & 255; q[2] = (bg >> 16) & 255; }
        rgb8[pix * 3] = (uint8_t)q[0]; rgb8[pix * 3 + 1] = (uint8_t)q[1]; rgb8[pix * 3 + 2] = (uint8_t)q[2];
    }
}
// A miss is final where it is found: zero light sum, background pixel.
__device__ __forceinline__ void store_miss(float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, const size_t pix, const uint32_t bg) {
    store_pixel(rgb_linear, rgb8, pix, mk(0.0f, 0.0f, 0.0f), false, 0.0f, 0.0f, bg, 0u);
}

// =================================================================================================
// Kernel 1: closest hit.  rayIntersection:405-431 with boundingBoxIntersection:296-317 fused in:
// walk ALL slab-passing nodes of ALL objects in pre-order (== reference visit order), test leaf
// triangles in stored order, strict '<' keeps the first (lowest id) of equal t.  No t-pruning: the
// reference has none and its slab test may cull what Moller-Trumbore would hit, so the candidate
// set must be reproduced exactly.
// =================================================================================================
template <bool COUNT>
__global__ __launch_bounds__(256) void k_closest_hit(DevScene s, DevParams p, int32_t* __restrict__ hit_id,
                                                     float* __restrict__ t_out, unsigned long long* __restrict__ counters) {
    uint32_t px, r;
    const bool live = tile_pixel(p, px, r);
    unsigned long long n_node = 0, n_tri = 0;
    float best = __builtin_inff();
    int32_t best_id = -1;
    if (live) {
        const V3 o = mk(0.0f, 0.0f, 0.0f);
        const V3 d = primary_dir(p, px, image_row(p, r));
        const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
        const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
        int32_t i = 0;
        const int32_t n = (int32_t)s.n_nodes;
        while (i < n) {
            const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
            const int32_t skip = __float_as_int(b.z), leaf = __float_as_int(b.w);
            if (COUNT) n_node++;
            if (ray_aabb(o, d, a.x, a.y, a.z, a.w, b.x, b.y)) {
                if (leaf >= 0) {
                    const int32_t first = leaf >> LEAF_SHIFT, cnt = leaf & LEAF_MAX;
                    for (int32_t k = 0; k < cnt; k++) {
                        V3 p1, e1, e2;
                        load_tri_edges(tris4, (size_t)(first + k), p1, e1, e2);
                        if (COUNT) n_tri++;
                        const float t = ray_triangle(o, d, p1, e1, e2);
                        if (t != SRT_NEG_INF && t < best) { best = t; best_id = first + k; }
                    }
                }
                i = i + 1;
            } else {
                i = skip;
            }
        }
        const size_t pix = (size_t)r * p.W + px;
        hit_id[pix] = best_id;
        t_out[pix] = best;
    }
    if (COUNT) { wave_add(counters + 1, n_node); wave_add(counters + 2, n_tri); }
}

// =================================================================================================
// Kernel 1, wave-queue form.  Same traversal, but the Moller-Trumbore tests are taken out of the
// divergent per-lane loop: a lane that passes a leaf's box pushes (triangle, lane) pairs into a
// per-wavefront LDS queue; whenever 64 pairs are queued the whole wave tests them at once (one pair per
// lane, 100 % SIMD utilisation) and merges with a 64-bit LDS atomicMin on (t bits << 32 | triangle id).
// t >= 0 orders as its bit pattern, so the minimum key is the reference's closest hit and, on equal t,
// the lowest id, i.e. the first in visit order (strict '<', simple_raytracer.cpp:429).
// =================================================================================================
constexpr int QCAP = 64 + 64 * 8 + 64;      // leftover (< 64) + one push round (64 lanes x <= 8) + slack
constexpr int PUSH_MAX = 8;                 // per lane per round; larger leaves are pushed in slices

template <bool COUNT>
__global__ __launch_bounds__(256) void k_closest_hit_q(DevScene s, DevParams p, int32_t* __restrict__ hit_id,
                                                       float* __restrict__ t_out, float* __restrict__ rgb_linear,
                                                       uint8_t* __restrict__ rgb8, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* q = q_all[wave];
    unsigned long long* best = best_all + wave * 64;
    uint32_t px, r;
    const bool live = tile_pixel(p, px, r);
    const uint32_t tile_x = blockIdx.x * 16 + (wave & 1) * 8, tile_r = blockIdx.y * 16 + (wave >> 1) * 8;
    unsigned long long n_node = 0, n_tri = 0;
    best[lane] = ~0ull;
    const V3 o = mk(0.0f, 0.0f, 0.0f);
    const V3 d = primary_dir(p, px, image_row(p, live ? r : 0));
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    const int32_t n = (int32_t)s.n_nodes;
    int32_t i = live ? 0 : n;
    int32_t leaf_off = 0;
    uint32_t qn = 0;                                    // wave-uniform queue length
    float4 na = nodes4[0], nb = nodes4[1];              // node i (valid while i < n)
    for (;;) {
        const bool active = i < n;
        const unsigned long long act = __ballot(active);
        if (act) {
            uint32_t cnt = 0, first = 0;
            if (active) {
                const float4 a = na, b = nb;
                const int32_t skip = __float_as_int(b.z), leaf = __float_as_int(b.w);
                if (COUNT && leaf_off == 0) n_node++;
                int32_t next;
                bool stay = false;
                if (ray_aabb_nb(o, d, a.x, a.y, a.z, a.w, b.x, b.y)) {
                    next = i + 1;
                    if (leaf >= 0) {
                        const int32_t c = (leaf & LEAF_MAX) - leaf_off;
                        first = (uint32_t)((leaf >> LEAF_SHIFT) + leaf_off);
                        cnt = (uint32_t)(c < PUSH_MAX ? c : PUSH_MAX);
                        if (c > PUSH_MAX) { leaf_off += PUSH_MAX; stay = true; } else leaf_off = 0;
                    }
                } else {
                    next = skip;
                }
                if (!stay) {
                    if (next < n) { na = nodes4[2 * (size_t)next]; nb = nodes4[2 * (size_t)next + 1]; }
                    i = next;
                }
            }
            // wave-wide exclusive prefix sum of cnt (0..8) by bit planes
            uint32_t pre = 0, tot = 0;
            #pragma unroll
            for (int bit = 0; bit < 4; bit++) {
                const unsigned long long m = __ballot((cnt >> bit) & 1u);
                pre += lane_prefix(m) << bit;
                tot += (uint32_t)__popcll(m) << bit;
            }
            for (uint32_t k = 0; k < cnt; k++) q[qn + pre + k] = ((first + k) << 6) | lane;
            qn += tot;
        } else if (qn == 0) {
            break;
        }
        __builtin_amdgcn_wave_barrier();
        while (qn >= 64 || (!act && qn)) {
            const uint32_t m = qn < 64 ? qn : 64;
            qn -= m;
            if (lane < m) {
                const uint32_t e = q[qn + lane];
                const uint32_t src = e & 63u, tri = e >> 6;
                const V3 ds = primary_dir(p, tile_x + (src & 7), image_row(p, tile_r + (src >> 3)));
                V3 p1, e1, e2;
                load_tri_edges(tris4, tri, p1, e1, e2);
                if (COUNT) n_tri++;
                const float t = ray_triangle(o, ds, p1, e1, e2);
                // candidate iff t != -inf && t < +inf (the initial distanceComparison, :408); NaN fails '<'
                if (t != SRT_NEG_INF && t < __builtin_inff()) {
                    const uint32_t tb = (t == 0.0f) ? 0u : __float_as_uint(t);     // -0.0 ties with +0.0
                    atomicMin(&best[src], ((unsigned long long)tb << 32) | tri);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __builtin_amdgcn_wave_barrier();
    bool is_hit = false;
    if (live) {
        const unsigned long long key = best[lane];
        int32_t id = -1;
        float t = __builtin_inff();
        if (key != ~0ull) {
            id = (int32_t)(uint32_t)key;
            // the winner's t with its own bits (incl. the sign of a zero): same function, same inputs
            V3 p1, e1, e2;
            load_tri_edges(tris4, (size_t)id, p1, e1, e2);
            t = ray_triangle(o, d, p1, e1, e2);
        }
        const size_t pix = (size_t)r * p.W + px;
        hit_id[pix] = id;
        t_out[pix] = t;
        if (id < 0) store_miss(rgb_linear, rgb8, pix, p.bg);
        is_hit = id >= 0;
    }
    count_hits(counters, is_hit, blockIdx.y * gridDim.x + blockIdx.x);
    if (COUNT) { wave_add(counters + 1, n_node); wave_add(counters + 2, n_tri); }
}

// =================================================================================================
// Kernel 1, node-queue form (shipped).  Lanes are decoupled from pixels: a wavefront owns a 4x4 pixel
// tile and keeps TWO LDS queues -- (node, pixel) pairs still to be slab-tested and (triangle, pixel)
// pairs still to be Moller-Trumbore-tested.  Every step pops 64 node pairs (LIFO, so the frontier stays
// depth-first small), tests them one per lane, pushes both children of a passing inner node and the
// triangles of a passing leaf.  All 64 lanes work as long as the tile has work, whatever the spread
// between its rays, and a heavy tile's work is cut into 4x more (and 4x shorter) waves than with one
// ray per lane.  The set of tested pairs is exactly "every node whose ancestors all pass"
// (boundingBoxIntersection:296-317) and the merge is the order-independent (t, id) minimum, so hits,
// t bits and work counts are those of the reference walk.
// If the node queue cannot take a step's children the wave finishes those subtrees with the stackless
// pre-order walk (skip links) instead -- any tree shape is handled with bounded LDS.
// =================================================================================================
// ---- list of quadrants (4x4 pixels) with hits: what the packet shadow kernel (srt_packet.h) works through ----------------
constexpr int QL_SHARDS = 64;            // shard lists; a quadrant goes to shard (tile index & 63)
constexpr int QL_STRIDE = 16;            // counters 64 B apart
// entry = two words: tile index << 2 | quadrant, and the quadrant's 16-bit hit mask (bit = y * 4 + x).  Called by one lane of a
// wave whose quadrant has a hit.
//
// HEAVY quadrants first (round 3).  The packet shadow kernel's launch ends when its longest walk does: a walk through a tree crown
// is 300-500 dependent steps (~0.3 ms), most walks are a dozen, and the quadrants arrive in the order the closest-hit waves happen to
// finish -- so some long walks start when the launch is nearly over (SQ_WAVE_CYCLES: the kernel's 8,192 wave slots are 70 % busy on the
// K4 frame, 45 % on an eighth of it).  A quadrant's walks are as long in the next frame as in this one (an orbit moves the picture by
// a few pixels, a benchmark not at all), so the shadow kernel leaves the step count of a quadrant's longest walk in a cost map
// (one word per quadrant, behind the list: qlist + 2 * QL_SHARDS * qcap words), and the NEXT frame's append reads it (and clears it):
// quadrants at or above heavy_steps grow from the END of their shard's array (own counters, [QL_SHARDS, 2 * QL_SHARDS)), and the
// shadow kernel deals all units of the heavy entries before any other.  Order only: every unit still owns its bytes of the result.
constexpr int QL_FETCH = 64;                     // counters the shadow kernel's waves take their unit numbers from: unit u belongs to counter u % 64.
                                                 // 256 of them (32 waves per counter instead of 128) were measured at the end of round 3 and are much WORSE
                                                 // (K4 9.37 -> 10.2 ms per 8 frames, K3 with 64 samples 7.37 -> 10.3; one number per atomic 14.3 / 14.8): the
                                                 // cost of these atomics is not the waves per address -- fewer atomics (pk_take) is what helps
constexpr int QL_COUNTERS = 2 * QL_SHARDS + QL_FETCH;      // list lengths | heavy-list lengths | units handed out
__device__ __forceinline__ uint32_t* quadrant_cost_map(uint32_t* qlist, uint32_t qcap) { return qlist + 2u * (size_t)QL_SHARDS * qcap; }
__device__ __forceinline__ void quadrant_list_append(uint32_t* __restrict__ qcount, uint32_t* __restrict__ qlist, uint32_t qcap,
                                                     uint32_t tile_index, uint32_t quadrant, uint32_t hit_mask, uint32_t heavy_steps) {
    const uint32_t shard = tile_index & (QL_SHARDS - 1), key = (tile_index << 2) | quadrant;
    bool heavy = false;
    if (heavy_steps) {
        uint32_t* const cost = quadrant_cost_map(qlist, qcap) + key;       // key < 4 * tiles <= QL_SHARDS * qcap
        const uint32_t c = *cost;
        heavy = c >= heavy_steps;
        if (c) *cost = 0u;
    }
    if (heavy) {
        const uint32_t slot = atomicAdd(qcount + (QL_SHARDS + shard) * QL_STRIDE, 1u);
        if (slot < qcap) reinterpret_cast<uint2*>(qlist)[(size_t)shard * qcap + (qcap - 1u - slot)] = make_uint2(key, hit_mask);
    } else {
        const uint32_t slot = atomicAdd(qcount + shard * QL_STRIDE, 1u);
        if (slot < qcap) reinterpret_cast<uint2*>(qlist)[(size_t)shard * qcap + slot] = make_uint2(key, hit_mask);
    }
}

constexpr int NQ_P = 16;                    // rays per wavefront of the shadow kernel (4x4 pixel quadrant)
constexpr int LQ_WORDS = 2 * (64 + 128);    // (leaf, ray) pair queue of the node-queue kernels: < 64 left over + <= 128 per push (two children per lane), 2 words each

// ---- the queues of closest_hit_phase and shadow_phase ------------------------------------------------------------------------
// A wave serves up to 64 rays, each known by its SLOT (the pixel lane of the closest-hit phase, the ray slot of the shadow phase),
// and keeps two LIFO queues in LDS with wave-uniform lengths:
//   nq: one word per entry, node << 6 | slot.  Narrow form: a 32 B DevNode still to be tested.  Wide form: a 64 B DevWide record of
//       an inner node that is known to pass; a pop tests BOTH its children.
//   tq: two words per entry, a passing leaf's (first << 5 | count) and the slot.  Whenever 64 entries are queued the phase's own
//       `drain` (its tri_batch) takes 64 of them, one per lane, so at most 63 wait when a push begins.
// A step pops <= 64 nq entries, one per lane, and pushes the children of the passing inner nodes and the passing leaves.
// `lane_order` (p.exp & 1) says where: false = node-major, all entries of one child side before those of the other, so that rays that
// visit one node stay neighbours; true = each lane's entries side by side.  If nq cannot take a step's children the wave finishes
// those subtrees with the stackless pre-order walk over the DevNode records (i = pass ? i + 1 : skip[i]): any tree shape is handled
// with bounded LDS.  Such a walk takes the exact test only (it is rare), and a shadow ray that has its hit leaves it at once.
// The leaf-queue pushes are shared below.  The node pops, the child pushes and the overflow walks are still written out per phase
// and form: stated as shared functions they compile to different code (more spills in the shipped kernels).
// queue each lane's passing leaf (is_leaf = false: nothing)
template <typename DRAIN>
__device__ __forceinline__ void leaf_queue_push(uint32_t* tq, uint32_t& tqn, uint32_t info, bool is_leaf, uint32_t slot, DRAIN drain) {
    const unsigned long long lm = __ballot(is_leaf);
    if (lm) {
        if (is_leaf) {
            const uint32_t pos = tqn + lane_prefix(lm);
            tq[2 * pos] = info; tq[2 * pos + 1] = slot;
        }
        tqn += (uint32_t)__popcll(lm);
        __builtin_amdgcn_wave_barrier();
        while (tqn >= 64) drain();
    }
}
// the same for up to two passing leaves per lane (the two children of a DevWide record)
template <typename DRAIN>
__device__ __forceinline__ void leaf_queue_push2(uint32_t* tq, uint32_t& tqn, bool lane_order, uint32_t info_a, bool leaf_a, uint32_t info_b, bool leaf_b,
                                                 uint32_t slot, DRAIN drain) {
    const unsigned long long ma = __ballot(leaf_a), mb = __ballot(leaf_b);
    if (ma | mb) {
        uint32_t pos = tqn + lane_prefix(ma) + lane_prefix(mb), q = pos + (leaf_a ? 1u : 0u);
        if (!lane_order) { pos = tqn + lane_prefix(ma); q = tqn + (uint32_t)__popcll(ma) + lane_prefix(mb); }      // node-major
        if (leaf_a) { tq[2 * pos] = info_a; tq[2 * pos + 1] = slot; }
        if (leaf_b) { tq[2 * q] = info_b; tq[2 * q + 1] = slot; }
        tqn += (uint32_t)__popcll(ma) + (uint32_t)__popcll(mb);
        __builtin_amdgcn_wave_barrier();
        while (tqn >= 64) drain();
    }
}


// TWL / THL: log2 of the tile width / height a wavefront owns (shipped: 4x4); FILTER: filtered slab predicate.
#ifdef SRT_DIAG
// Diagnostic build only (python -m simple_raytracer_amd.build --diag -> libsrt_hip_diag.so, never shipped): per-wave
// cycle stamps of the closest-hit phase, written where rgb_linear would go (8 x u64 per wave).
#define SRT_STAMP(v) do { v = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_s_waitcnt(0xC07F); } while (0)
// whole-tile record of the fused kernels: slot 5 = HW_ID | XCC_ID << 32, slots 6 / 7 = absolute start / end stamps
__device__ __forceinline__ void diag_tile_record(float* rgb_linear, uint32_t bx, uint32_t by, uint32_t gx, unsigned long long k0, unsigned long long k1,
                                                 unsigned long long ka = 0, unsigned long long kb = 0) {      // ka / kb: after the launch-time barrier / after the closest-hit phase
    if ((threadIdx.x & 63) == 0 && rgb_linear) {
        unsigned long long* dgp = reinterpret_cast<unsigned long long*>(rgb_linear) + (((size_t)by * gx + bx) * 4 + (threadIdx.x >> 6)) * 8;
        const unsigned long long hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);
        dgp[5] = hw | (xcc << 32); dgp[6] = k0; dgp[7] = k1;
        if (ka) { dgp[3] = ka - k0; dgp[4] = kb - ka; }
    }
}
#else
#define SRT_STAMP(v) do { } while (0)
#endif

// The phase runs per wavefront on LDS the caller provides: nq[NQCAP], tq[QCAP], best[P], dir[P].  On return the
// lanes < P hold their pixel's hit id and t (also written to hit_id / t_out, with the final pixel for misses).
// CAM: camera mode (srt_params.ray_matrix): the rays start at the camera's position in the scene's space and their directions have
// three varying components, so the phase keeps (dx, dy, dz) per ray, takes the reciprocals per test and tests triangles in the general
// form (P1, e1, e2 and the ray's origin) instead of the origin form -- the arithmetic of the oracle's camera mode.
// WIDE: the queue holds inner nodes that are known to pass, as indices of their DevWide records (srt_device.h): a pop tests BOTH
// children.  !WIDE is the round-1/2 form (a queue entry is a node still to be tested, 32 B records), kept for A/B (variant 40).
// HALF (with TWL = 3, THL = 2): the wave owns the upper or lower half of the workgroup's 8x8 tile -- `wave` = 0 / 1, rows 4 * wave ..
// 4 * wave + 3, all eight columns -- and ray pl < 32 is the pixel x = (pl >> 4 & 1) * 4 + (pl & 3), y = pl >> 2 & 3 of the half: pl >> 4
// is the 4x4 quadrant inside the half and pl & 15 the pixel of that quadrant as the four-wave form numbers it, so ray pl of half h is
// entry 32 * h + pl of the tile's root masks and bit 32 * h + pl of the tile's shadow words.
// OWN_ROOTS (with HALF and !WIDE, and only where `own_roots` is set): nobody has tested the roots for this wave -- it has no partner and
// no launch-time barrier (k_trace_nq_wave8_spans) -- so it puts its own 32 rays through the root table, one (ray, object) pair per lane,
// and queues for a passing root what the root_pass branch queues: the same pairs in the same order.
// PAIRS: the triangle loop of a batch holds two named records and runs over pairs of tests (below); the same tests in the same order.
template <bool COUNT, int NQCAP, int TWL, int THL, bool FILTER, bool CAM = false, bool WIDE = false, bool HALF = false, bool OWN_ROOTS = false, bool PAIRS = false>
__device__ __forceinline__ void closest_hit_phase(const DevScene& s, const DevParams& p, uint32_t* nq, uint32_t* tq,
                                                  unsigned long long* best, float4* dir,
                                                  int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                  float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                  unsigned long long* __restrict__ counters, int32_t& out_id, float& out_t, V3& out_d,
                                                  const uint32_t bx, const uint32_t by, const uint32_t gx,      // workgroup tile coordinates, tiles per row
                                                  const uint32_t wave,                                          // quadrant of the tile this wave owns
                                                  uint32_t* __restrict__ qcount = nullptr, uint32_t* __restrict__ qlist = nullptr, uint32_t qcap = 0,   // list of quadrants with hits (4x4 waves only)
                                                  const uint32_t* root_pass = nullptr,        // per ray of this quadrant: which objects' ROOT boxes it passes (bit = object), from
                                                                                              // finish_background_tile, which has put all 64 rays of the tile through every root already
                                                  const bool own_roots = false) {             // OWN_ROOTS: the wave tests the roots itself and queues their children (at most 32 objects)
    constexpr int P = 1 << (TWL + THL);           // rays per wavefront
    static_assert(!OWN_ROOTS || (HALF && !WIDE && !COUNT), "the wave's own root pass is the half-tile form's, over the 32 B records");
    static_assert(!PAIRS || !COUNT, "the pair loop has no counting build");
    const uint32_t lane = threadIdx.x & 63;
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    static_assert(!HALF || (TWL == 3 && THL == 2), "a half tile is 8x4 pixels");
    const uint32_t tile_x = HALF ? bx * 8 + ((lane >> 4) & 1u) * 4 : (bx * 2 + (wave & 1)) << TWL, tile_r = HALF ? by * 8 + wave * 4 : (by * 2 + (wave >> 1)) << THL;
    const uint32_t px = tile_x + (lane & (HALF ? 3u : (1u << TWL) - 1)), r = tile_r + ((lane >> (HALF ? 2 : TWL)) & ((1u << THL) - 1));
    const bool live = lane < P && pixel_live(p, px, r);
    const V3 o = CAM ? ray_origin(p) : mk(0.0f, 0.0f, 0.0f);
    if (lane < P) {
        V3 dmine = mk(0.f, 0.f, p.focal);
        best[lane] = ~0ull;
        if (live) dmine = primary_dir(p, px, image_row(p, r));
        if (CAM) dir[lane] = make_float4(dmine.x, dmine.y, dmine.z, 0.f);
        else { const RayRcp rq = ray_rcp(dmine); dir[lane] = make_float4(dmine.x, dmine.y, rq.x, rq.y); }   // + reciprocals for the filtered slab test (all NaN for a ray the filter must not decide; dmine.z is p.focal)
    }
    const float rcp_focal = __builtin_amdgcn_rcpf(p.focal);
    const unsigned long long livem = __ballot(live);
    unsigned long long n_node = 0, n_tri = 0;
    uint32_t nqn = 0, tqn = 0;                       // wave-uniform queue lengths
    __builtin_amdgcn_wave_barrier();
    unsigned long long dg_pop = 0, dg_load = 0; (void)dg_pop; (void)dg_load;
    unsigned long long dg_t0 = 0, dg_a = 0, dg_b = 0, dg_test = 0, dg_commit = 0, dg_tri = 0, dg_steps = 0, dg_batches = 0, dg_items = 0, dg_titems = 0;
    (void)dg_t0; (void)dg_a; (void)dg_b; (void)dg_test; (void)dg_commit; (void)dg_tri; (void)dg_steps; (void)dg_batches; (void)dg_items; (void)dg_titems;
    SRT_STAMP(dg_t0);

    // One batch of <= 64 queued (leaf, pixel) pairs, one per lane: the lane runs Moller-Trumbore over the leaf's
    // triangles in stored order (next triangle's loads issued before the current test), keeps the first minimum
    // (strict '<', :429) and merges once with the LDS atomicMin.  A queue entry is two words: the leaf's
    // (first << 5 | count) and the pixel lane.
    auto tri_batch = [&]() {
        const uint32_t m = tqn < 64 ? tqn : 64;
        tqn -= m;
#ifdef SRT_DIAG
        unsigned long long c0, c1; SRT_STAMP(c0); dg_batches++; dg_titems += m;
#endif
        // a batch that does not fill the wave (the flush at the end of a tile: 16 rays x a leaf or two) is spread over
        // sub-lanes: S lanes share one (leaf, ray) pair and take every S-th triangle; the merge below does not care who
        // found the minimum.  A full batch has S = 1: one pair per lane.
        const uint32_t sh = m <= 8 ? 3u : (m <= 16 ? 2u : (m <= 32 ? 1u : 0u));
        const uint32_t S = 1u << sh, pi = lane >> sh, sub = lane & (S - 1u);
        if (pi < m) {
            const uint32_t info = tq[2 * (tqn + pi)], pl = tq[2 * (tqn + pi) + 1];
            const uint32_t first = info >> LEAF_SHIFT, cnt = info & LEAF_MAX;
            const float4 dxy = dir[pl];
            const V3 d = mk(dxy.x, dxy.y, CAM ? dxy.z : p.focal);
            float bt = __builtin_inff();
            uint32_t bi = 0;
            // one triangle per iteration, the next one's three dwordx4 loads issued before the current test: a wave spends
            // most of its life behind s_waitcnt, and the all-lanes-rejected exits of a single test skip more code than two
            // interleaved tests could (measured: 5 % of the launch); ids rise inside a lane, so strict '<' keeps the first minimum
            // The GENERAL record (P1, e1, e2) also for rays from the origin: 12 operations more a test than the origin record (tvec, qvec
            // precomputed; still what the packet kernel reads, whose operands are scalar), but ONE record array in the caches instead of two
            // -- this phase and the shadow phase then read the same 48 bytes of a triangle.  o = 0 gives tvec = 0 - P1 and qvec =
            // cross(tvec, e1) with the host's operations: same bits.  Same box: K3 4.30 -> 4.25 ms per 36 frames, cube over ground
            // 3.12 -> 3.06, K4's closest-hit launch 0.239 -> 0.232 ms.
            const float4* tp = reinterpret_cast<const float4*>(s.tris) + ((size_t)first + sub) * 3;
            if constexpr (PAIRS) {
                // The same loop without its rotation (n -> a: eight moves at the head of every test and nine at its end, 17 of about 91
                // VALU instructions): two named records, A and B.  A is tested while B's loads are in flight, B while the next A's are; an odd
                // count, and a count of one, end in A.  Ascending ids, the strict '<' and `bi` as below.
                auto test = [&](const float4 c0, const float4 c1, const float c2, const uint32_t k) {
                    const float ta = ray_triangle(o, d, mk(c0.x, c0.y, c0.z), mk(c0.w, c1.x, c1.y), mk(c1.z, c1.w, c2));
                    if (ta != SRT_NEG_INF && ta < bt) { bt = ta; bi = first + k; }
                };
                float4 a0, a1, b0, b1; float a2, b2;
                // (every path that goes on has loaded the set it goes on with: no set is carried round the loop beside its successor,
                // which is what the compiler turned into copies)
                if (sub < cnt) {
                    a0 = tp[0]; a1 = tp[1]; a2 = tp[2].x;
                    for (uint32_t k = sub;; k += 2u * S) {
                        if (k + S >= cnt) { test(a0, a1, a2, k); break; }                    // ends in A
                        tp += 3 * S; b0 = tp[0]; b1 = tp[1]; b2 = tp[2].x;
                        test(a0, a1, a2, k);
                        if (k + 2u * S >= cnt) { test(b0, b1, b2, k + S); break; }            // ends in B
                        tp += 3 * S; a0 = tp[0]; a1 = tp[1]; a2 = tp[2].x;
                        test(b0, b1, b2, k + S);
                    }
                }
            } else {
            float4 n0, n1; float n2;                     // (the record's last three words are the face normal: not read here)
            if (sub < cnt) { n0 = tp[0]; n1 = tp[1]; n2 = tp[2].x; }
            for (uint32_t k = sub; k < cnt; k += S) {
                const float4 a0 = n0, a1 = n1; const float a2 = n2;
                if (k + S < cnt) { tp += 3 * S; n0 = tp[0]; n1 = tp[1]; n2 = tp[2].x; }      // the next triangle's record is in flight during this test
                if (COUNT) n_tri++;
                const float ta = ray_triangle(o, d, mk(a0.x, a0.y, a0.z), mk(a0.w, a1.x, a1.y), mk(a1.z, a1.w, a2));
                // candidate iff t != -inf && t < best (initially +inf, :408); NaN fails '<'; -0.0 == +0.0 keeps the first
                if (ta != SRT_NEG_INF && ta < bt) { bt = ta; bi = first + k; }
            }
            }
            if (bt < __builtin_inff()) {
                const uint32_t tb = (bt == 0.0f) ? 0u : __float_as_uint(bt);     // -0.0 ties with +0.0
                atomicMin(&best[pl], ((unsigned long long)tb << 32) | bi);
            }
        }
        __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
        SRT_STAMP(c1); dg_tri += c1 - c0;
#endif
    };
    const uint32_t n_obj = s.n_objects;
    const uint32_t nlive = (uint32_t)__popcll(livem);
    constexpr uint32_t OBJ_G = (NQCAP / (2 * P)) < 16 ? (NQCAP / (2 * P)) : 16;      // roots pushed at once: P * OBJ_G <= NQCAP / 2
    if constexpr (WIDE) {
    const float4* wide4 = reinterpret_cast<const float4*>(s.wide);
    for (uint32_t obj0 = 0; obj0 < n_obj && nlive; obj0 += OBJ_G) {
        const uint32_t g = (n_obj - obj0) < OBJ_G ? (n_obj - obj0) : OBJ_G;
        // the roots: either tested already (root_pass: wave 0 ran them for the whole tile with full lanes) or tested here, one (ray,
        // object) pair per lane; a passing root that is an inner node is queued, a passing leaf's triangles are
        for (uint32_t base = 0; base < P * g; base += 64) {
            const uint32_t k = base + lane_again(lane);
            const uint32_t pl = k & (P - 1), ob = k >> (TWL + THL);
            bool ok = k < P * g && ((livem >> pl) & 1ull);
            if (!COUNT && root_pass) ok = ok && ((root_pass[pl] >> (obj0 + ob)) & 1u);
            else if (ok) {
                const int32_t root = s.obj_range[obj0 + ob].x;
                const float4 a = nodes4[2 * (size_t)root], b = nodes4[2 * (size_t)root + 1];
                const float4 dxy = dir[pl];
                const V3 d = mk(dxy.x, dxy.y, CAM ? dxy.z : p.focal);
                RayRcp rc;
                if (CAM) rc = ray_rcp(d);
                else { rc.x = dxy.z; rc.y = dxy.w; rc.z = __builtin_fmaf(dxy.z, 0.0f, rcp_focal); }      // rcp_focal, or NaN with the other two (ray_rcp's rule)
                if (COUNT) n_node++;
                ok = slab_pass<FILTER>(o, d, rc, a.x, a.y, a.z, a.w, b.x, b.y);
            }
            int32_t info = 0;
            if (ok) info = s.obj_root_info[obj0 + ob];
            const bool inner = ok && info < 0, leafp = ok && info >= 0 && (info & LEAF_MAX) != 0;
            const unsigned long long im = __ballot(inner);
            if (inner) nq[nqn + lane_prefix(im)] = ((uint32_t)(~info) << 6) | pl;
            nqn += (uint32_t)__popcll(im);
            leaf_queue_push2(tq, tqn, p.exp & 1u, (uint32_t)info, leafp, 0u, false, pl, tri_batch);
        }
        __builtin_amdgcn_wave_barrier();
        while (nqn) {
            const uint32_t m = nqn < 64 ? nqn : 64;
            nqn -= m;
#ifdef SRT_DIAG
            SRT_STAMP(dg_a); dg_steps++; dg_items += m;
            const unsigned long long tri_before = dg_tri;
#endif
            const bool have = lane < m;
            uint32_t pl = 0;
            int32_t linfo = 0, rinfo = 0, node = 0, rnode = 0;
            bool in_l = false, in_r = false, lf_l = false, lf_r = false;
            V3 d = mk(0.f, 0.f, p.focal);
            if (have) {
                const uint32_t e = nq[nqn + lane];
                pl = e & 63u;
#ifdef SRT_DIAG
                { unsigned long long c_; asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); SRT_STAMP(c_); dg_pop += c_ - dg_a; dg_a = c_; }
#endif
                const float4* wp = wide4 + 4 * (size_t)(e >> 6);
                const float4 r0 = wp[0], r1 = wp[1], r2 = wp[2];
                const int4 r3 = reinterpret_cast<const int4*>(wp)[3];
                const float4 dxy = dir[pl];
#ifdef SRT_DIAG
                { unsigned long long c_; asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); SRT_STAMP(c_); dg_load += c_ - dg_a; dg_a = c_; }
#endif
                d = mk(dxy.x, dxy.y, CAM ? dxy.z : p.focal);
                RayRcp rc;
                if (CAM) rc = ray_rcp(d);
                else { rc.x = dxy.z; rc.y = dxy.w; rc.z = __builtin_fmaf(dxy.z, 0.0f, rcp_focal); }      // rcp_focal, or NaN with the other two (ray_rcp's rule)
                linfo = r3.x; rinfo = r3.y; node = r3.z; rnode = r3.w;
                if (COUNT) n_node += 2;
                bool pass_l, pass_r;
                slab_pass2<FILTER>(o, d, rc, r0, r1, r2, pass_l, pass_r);
                in_l = pass_l && linfo < 0; lf_l = pass_l && linfo >= 0 && (linfo & LEAF_MAX) != 0;
                in_r = pass_r && rinfo < 0; lf_r = pass_r && rinfo >= 0 && (rinfo & LEAF_MAX) != 0;
            }
            __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
            SRT_STAMP(dg_b); dg_test += dg_b - dg_a;
#endif
            const unsigned long long ml = __ballot(in_l), mr = __ballot(in_r);
            const uint32_t n_in = (uint32_t)__popcll(ml) + (uint32_t)__popcll(mr);
            if (nqn + n_in <= (uint32_t)NQCAP) {
                if (!(p.exp & 1u)) {      // node-major: all right children, then all left children -- rays that visit one node stay neighbours
                    if (in_r) nq[nqn + lane_prefix(mr)] = ((uint32_t)(~rinfo) << 6) | pl;
                    if (in_l) nq[nqn + (uint32_t)__popcll(mr) + lane_prefix(ml)] = ((uint32_t)(~linfo) << 6) | pl;
                } else {
                const uint32_t pos = nqn + lane_prefix(ml) + lane_prefix(mr);
                if (in_r) nq[pos] = ((uint32_t)(~rinfo) << 6) | pl;
                if (in_l) nq[pos + (in_r ? 1u : 0u)] = ((uint32_t)(~linfo) << 6) | pl;      // left child on top: popped first
                }
                nqn += n_in;
                leaf_queue_push2(tq, tqn, p.exp & 1u, (uint32_t)linfo, lf_l, (uint32_t)rinfo, lf_r, pl, tri_batch);
            } else {
                // queue full: finish the passing children's subtrees with the stackless pre-order walk over the 32 B records
                // (i = pass ? i + 1 : skip[i]).  Left subtree = nodes (node + 2 .. rnode), right = (rnode + 1 .. skip[rnode]); with both
                // the walk runs through and hops over the right child itself, which has been tested above.
                leaf_queue_push2(tq, tqn, p.exp & 1u, (uint32_t)linfo, lf_l, (uint32_t)rinfo, lf_r, pl, tri_batch);
                int32_t i = 0, end = 0, hop = -1;
                if (in_l | in_r) {
                    i = in_l ? node + 2 : rnode + 1;
                    end = in_r ? s.nodes[rnode].skip : rnode;
                    hop = (in_l && in_r) ? rnode : -1;
                }
                while (__ballot(i < end)) {
                    int32_t inf2 = -1;
                    bool lp2 = false;
                    if (i < end) {
                        if (i == hop) i = hop + 1;
                        else {
                            const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
                            const int32_t sk = __float_as_int(b.z);
                            inf2 = __float_as_int(b.w);
                            if (COUNT) n_node++;
                            if (ray_aabb_nb(o, d, a.x, a.y, a.z, a.w, b.x, b.y)) {
                                lp2 = inf2 >= 0 && (inf2 & LEAF_MAX) != 0;
                                i = i + 1;
                            } else {
                                i = sk;
                            }
                        }
                    }
                    leaf_queue_push2(tq, tqn, p.exp & 1u, (uint32_t)inf2, lp2, 0u, false, pl, tri_batch);
                }
            }
            __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
            { unsigned long long c2_; SRT_STAMP(c2_); dg_commit += (c2_ - dg_b) - (dg_tri - tri_before); }
#endif
        }
    }
    } else
    for (uint32_t obj0 = 0; obj0 < n_obj && nlive; obj0 += OBJ_G) {
        // roots of up to OBJ_G objects for every live pixel, in chunks of 64 (node, pixel) pairs
        const uint32_t g = (n_obj - obj0) < OBJ_G ? (n_obj - obj0) : OBJ_G;
        if (OWN_ROOTS && own_roots) {      // (a constant false where OWN_ROOTS is: those builds get the statement below as they always did)
            // the wave's own root pass: the record from the contiguous root table (index = object: nothing waits for obj_range), the
            // filtered test with the exact fallback, and a passing root queues its two children, or its triangles, as below
            for (uint32_t base = 0; base < P * g; base += 64) {
                const uint32_t k = base + lane_again(lane);
                const uint32_t pl = k & (P - 1), ob = k >> (TWL + THL);
                bool ok = k < P * g && ((livem >> pl) & 1ull);
                int32_t root = 0, info = -1;
                if (ok) {
                    const float4* rn = reinterpret_cast<const float4*>(s.root_nodes) + 2 * (size_t)(obj0 + ob);
                    const float4 a = rn[0], b = rn[1];
                    root = s.obj_range[obj0 + ob].x;
                    const float4 dxy = dir[pl];
                    const V3 d = mk(dxy.x, dxy.y, CAM ? dxy.z : p.focal);
                    RayRcp rc;
                    if (CAM) rc = ray_rcp(d);
                    else { rc.x = dxy.z; rc.y = dxy.w; rc.z = __builtin_fmaf(dxy.z, 0.0f, rcp_focal); }      // rcp_focal, or NaN with the other two (ray_rcp's rule)
                    info = __float_as_int(b.w);
                    ok = slab_pass<FILTER>(o, d, rc, a.x, a.y, a.z, a.w, b.x, b.y);
                }
                const bool inner = ok && info < 0, leafp = ok && info >= 0 && (info & LEAF_MAX) != 0;
                const unsigned long long im = __ballot(inner);
                if (inner) {
                    uint32_t pos = nqn + 2 * lane_prefix(im), pos1 = pos + 1;
                    if (!(p.exp & 1u)) { pos = nqn + lane_prefix(im); pos1 = pos + (uint32_t)__popcll(im); }      // node-major
                    nq[pos] = ((uint32_t)(~info) << 6) | pl;          // right child
                    nq[pos1] = ((uint32_t)(root + 1) << 6) | pl;      // left child on top: popped first
                }
                nqn += 2 * (uint32_t)__popcll(im);
                leaf_queue_push(tq, tqn, (uint32_t)info, leafp, pl, tri_batch);
            }
        } else if (!COUNT && root_pass) {
            // the root tests are done (wave 0 ran them for the whole tile with full lanes): queue what a passing root queues -- its two
            // children, or its triangles -- and skip the first node step, which would run at 16 rays x 2 roots = 32 of 64 lanes
            for (uint32_t base = 0; base < P * g; base += 64) {
                const uint32_t k = base + lane_again(lane);
                const uint32_t pl = k & (P - 1), ob = k >> (TWL + THL);
                const bool ok = k < P * g && ((livem >> pl) & 1ull) && ((root_pass[pl] >> (obj0 + ob)) & 1u);
                int32_t root = 0, info = -1;
                if (ok) { root = s.obj_range[obj0 + ob].x; info = s.root_nodes[obj0 + ob].leaf; }      // two independent loads
                const bool inner = ok && info < 0, leafp = ok && info >= 0 && (info & LEAF_MAX) != 0;
                const unsigned long long im = __ballot(inner);
                if (inner) {
                    uint32_t pos = nqn + 2 * lane_prefix(im), pos1 = pos + 1;
                    if (!(p.exp & 1u)) { pos = nqn + lane_prefix(im); pos1 = pos + (uint32_t)__popcll(im); }      // node-major
                    nq[pos] = ((uint32_t)(~info) << 6) | pl;          // right child
                    nq[pos1] = ((uint32_t)(root + 1) << 6) | pl;      // left child on top: popped first
                }
                nqn += 2 * (uint32_t)__popcll(im);
                leaf_queue_push(tq, tqn, (uint32_t)info, leafp, pl, tri_batch);
            }
        } else
        for (uint32_t base = 0; base < P * g; base += 64) {
            const uint32_t k = base + lane_again(lane);
            const uint32_t pl = k & (P - 1), ob = k >> (TWL + THL);
            const bool ok = k < P * g && ((livem >> pl) & 1ull);
            const unsigned long long m = __ballot(ok);
            if (ok) nq[nqn + lane_prefix(m)] = ((uint32_t)s.obj_range[obj0 + ob].x << 6) | pl;
            nqn += (uint32_t)__popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        while (nqn) {
            const uint32_t m = nqn < 64 ? nqn : 64;
            nqn -= m;
#ifdef SRT_DIAG
            SRT_STAMP(dg_a); dg_steps++; dg_items += m;
            const unsigned long long tri_before = dg_tri;
#endif
            const bool have = lane < m;
            uint32_t pl = 0;
            int32_t node = 0, info = -1, skip = 0;
            bool inner = false, leafp = false;
            V3 d = mk(0.f, 0.f, p.focal);
            if (have) {
                const uint32_t e = nq[nqn + lane];
                pl = e & 63u; node = (int32_t)(e >> 6);
#ifdef SRT_DIAG
                { unsigned long long c_; asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); SRT_STAMP(c_); dg_pop += c_ - dg_a; dg_a = c_; }
#endif
                const float4 a = nodes4[2 * (size_t)node], b = nodes4[2 * (size_t)node + 1];
                const float4 dxy = dir[pl];
#ifdef SRT_DIAG
                { unsigned long long c_; asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); SRT_STAMP(c_); dg_load += c_ - dg_a; dg_a = c_; }
#endif
                d = mk(dxy.x, dxy.y, CAM ? dxy.z : p.focal);
                skip = __float_as_int(b.z); info = __float_as_int(b.w);
                if (COUNT) n_node++;
                bool pass;
                if (FILTER) {
                    bool amb;
                    RayRcp rc;
                    if (CAM) rc = ray_rcp(d);
                    else { rc.x = dxy.z; rc.y = dxy.w; rc.z = __builtin_fmaf(dxy.z, 0.0f, rcp_focal); }      // rcp_focal, or NaN with the other two (ray_rcp's rule)
                    pass = ray_aabb_filtered(o, rc, a.x, a.y, a.z, a.w, b.x, b.y, amb);
                    if (amb) pass = ray_aabb_nb(o, d, a.x, a.y, a.z, a.w, b.x, b.y);      // rare: exact divides decide
                } else {
                    pass = ray_aabb_nb(o, d, a.x, a.y, a.z, a.w, b.x, b.y);
                }
                if (pass) {
                    if (info < 0) inner = true;
                    else leafp = (info & LEAF_MAX) != 0;
                }
            }
            __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
            SRT_STAMP(dg_b); dg_test += dg_b - dg_a;
#endif
            const unsigned long long im = __ballot(inner);
            const uint32_t n_in = (uint32_t)__popcll(im);
            if (nqn + 2 * n_in <= (uint32_t)NQCAP) {
                if (inner) {
                    uint32_t pos = nqn + 2 * lane_prefix(im), pos1 = pos + 1;
                    if (!(p.exp & 1u)) { pos = nqn + lane_prefix(im); pos1 = pos + n_in; }      // node-major
                    nq[pos] = ((uint32_t)(~info) << 6) | pl;          // right child
                    nq[pos1] = ((uint32_t)(node + 1) << 6) | pl;      // left child on top: popped first
                }
                nqn += 2 * n_in;
                leaf_queue_push(tq, tqn, (uint32_t)info, leafp, pl, tri_batch);
            } else {
                // queue full: finish these subtrees with the stackless pre-order walk (i = pass ? i+1 : skip[i])
                leaf_queue_push(tq, tqn, (uint32_t)info, leafp, pl, tri_batch);
                int32_t i = inner ? node + 1 : 0, end = inner ? skip : 0;
                while (__ballot(i < end)) {
                    int32_t inf2 = -1;
                    bool lp2 = false;
                    if (i < end) {
                        const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
                        const int32_t sk = __float_as_int(b.z);
                        inf2 = __float_as_int(b.w);
                        if (COUNT) n_node++;
                        if (ray_aabb_nb(o, d, a.x, a.y, a.z, a.w, b.x, b.y)) {
                            lp2 = inf2 >= 0 && (inf2 & LEAF_MAX) != 0;
                            i = i + 1;
                        } else {
                            i = sk;
                        }
                    }
                    leaf_queue_push(tq, tqn, (uint32_t)inf2, lp2, pl, tri_batch);
                }
            }
            __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
            { unsigned long long c2_; SRT_STAMP(c2_); dg_commit += (c2_ - dg_b) - (dg_tri - tri_before); }
#endif
        }
    }
    while (tqn) tri_batch();
    __builtin_amdgcn_wave_barrier();
#ifdef SRT_DIAG
    {
        unsigned long long c3; SRT_STAMP(c3);
        if (lane == 0 && rgb_linear) {
            unsigned long long* dgp = reinterpret_cast<unsigned long long*>(rgb_linear) +
                                      (((size_t)by * gx + bx) * 4 + wave) * 8;
            dgp[0] = c3 - dg_t0; dgp[1] = dg_steps; dgp[2] = dg_batches; dgp[3] = dg_test; dgp[4] = dg_commit; dgp[5] = dg_tri;
            dgp[6] = dg_pop; dgp[7] = dg_load;
        }
        rgb_linear = nullptr;
    }
#endif

    bool is_hit = false;
    out_id = -1; out_t = __builtin_inff(); out_d = mk(0.f, 0.f, p.focal);
    if (live) {
        // the lane's own ray, as it has stood in dir[] since the set-up (same bits): not kept in registers through the walk
        const float4 dl = dir[lane];
        const V3 dmine = mk(dl.x, dl.y, CAM ? dl.z : p.focal);
        out_d = dmine;
        const unsigned long long key = best[lane];
        int32_t id = -1;
        float t = __builtin_inff();
        if (key != ~0ull) {
            id = (int32_t)(uint32_t)key;
            // the key carries the winner's t bit for bit, except that -0.0 was merged as +0.0 (they tie, :429): only a
            // zero is evaluated again, to get its sign (same function, same inputs)
            t = __uint_as_float((uint32_t)(key >> 32));
            if (t == 0.0f) {
                V3 p1, e1, e2;
                load_tri_edges(tris4, (size_t)id, p1, e1, e2);
                t = ray_triangle(o, dmine, p1, e1, e2);
            }
        }
        const size_t pix = (size_t)r * p.W + px;
        hit_id[pix] = id;
        t_out[pix] = t;
        if (id < 0) store_miss(rgb_linear, rgb8, pix, p.bg);
        is_hit = id >= 0;
        out_id = id; out_t = t;
    }
    // The hit statistic is taken by the SHADING kernel since the end of round 3 (one atomic per 8x8 tile with hits there instead of one per
    // quadrant wave here: these fire-and-forget atomics cost the K3 trace launch 4 % -- 0.1157 -> 0.111 ms without them); exp bit 5: the
    // pipeline has no shading launch behind this phase (k_trace_shade_nq), count here.
    if (p.exp & 32u) count_hits(counters, is_hit, by * gx + bx);
    if (TWL == 2 && THL == 2 && qlist) {
        const unsigned long long hm = __ballot(is_hit);          // all lanes vote: not inside the lane-0 branch
        if (lane == 0 && hm) quadrant_list_append(qcount, qlist, qcap, by * gx + bx, wave, (uint32_t)hm, p.heavy_steps);
    }
    if (COUNT) { wave_add(counters + 1, n_node); wave_add(counters + 2, n_tri); }
}

// Background tiles: most of a typical frame, and a wave that only learns that its 16 rays miss every object costs ~150 VALU
// instructions of set-up, queueing and write-out.  So wave 0 of a workgroup first puts the tile's 64 rays (one per lane)
// through the slab test of every object's root box -- the very test the first node step of each ray would run -- while the
// other three waves wait at a launch-time barrier (nobody has work to wait behind yet); if no ray passes any root it writes
// the 64 background pixels (and, when shadow_bits is given, the tile's all-clear shadow words) with full lanes.  Returns true
// to every thread of the workgroup when the tile is finished.
// One WAVE puts the 64 rays of tile (bx, by) through every object's root box; if none passes any it writes the tile's background
// pixels (and all-clear shadow words).  Returns (wave-uniform) whether the tile is live; root_pass (LDS, 64 words, quadrant * 16 +
// pixel) receives, per ray, the objects whose root box it passes.
template <bool FILTER, bool CAM = false>
__device__ __forceinline__ bool background_test_wave(const DevScene& s, const DevParams& p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                     float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                     unsigned long long* __restrict__ shadow_bits,
                                                     const uint32_t bx, const uint32_t by, const uint32_t gx, uint32_t* root_pass,
                                                     const uint32_t root_half_stride = 0) {      // != 0: the masks of rays 32 .. 63 start this many words after those of rays 0 .. 31
    const uint32_t lane = threadIdx.x & 63, quad = lane >> 4, ql = lane & 15u;
    const uint32_t px = bx * 8 + (quad & 1) * 4 + (ql & 3), r = by * 8 + (quad >> 1) * 4 + (ql >> 2);
    const bool live = pixel_live(p, px, r);
    const V3 o = CAM ? ray_origin(p) : mk(0.f, 0.f, 0.f);
    const V3 dd = live ? primary_dir(p, px, image_row(p, r)) : mk(0.f, 0.f, p.focal);
    const RayRcp rc = ray_rcp(dd);
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    bool any = false;
    uint32_t pmask = 0;
    // four objects at a time: their root records come from the contiguous table by wave-uniform (scalar) loads that depend on nothing
    // but the object's number, so all eight requests of a group are in flight together (a scene of seven objects used to be a chain of
    // fourteen dependent round trips before the workgroup's other three waves could start)
    const float4* rn4 = reinterpret_cast<const float4*>(s.root_nodes);
    const uint32_t n_obj = s.n_objects;
    // Scenes of several objects: the union of their root boxes first.  A ray that CERTAINLY fails it -- filtered test decided, not
    // ambiguous: tfar_U < tnear_U by more than the margin -- fails every root box inside it under the reference's own comparisons: per
    // axis an inner box's t-interval nests in the union's, so tnear_A >= tnear_U and tfar_A <= tfar_U, and tnear_A - tfar_A exceeds both
    // the union's margin (2e-6 of |tnear_U| + |tfar_U|) and, when A's values are much larger than the union's, half of |tnear_A| +
    // |tfar_A| itself -- either way far more than the half-ulp the correctly rounded quotients of A can move.  Most tiles of a 4K frame
    // of the reference's scenes are sky: one test instead of one per object on the path every tile waits behind.
    bool skip_roots = false;
    if (FILTER && n_obj >= 3u && !(p.exp & 10u)) {      // (variants 45 / 46 switch it off, A/B)
        const float4 ua = reinterpret_cast<const float4*>(s.scene_box)[0], ub = reinterpret_cast<const float4*>(s.scene_box)[1];
        bool amb_u;
        const bool pass_u = ray_aabb_filtered(o, rc, ua.x, ua.y, ua.z, ua.w, ub.x, ub.y, amb_u);
        skip_roots = !__ballot(live && (pass_u || amb_u));
    }
    if (skip_roots) { /* no ray can pass any root: pmask stays 0 */ } else
    if (p.exp & 2u) {        // A/B: the round-2 loop (obj_range[ob] -> nodes[root], one object after the other)
        for (uint32_t ob = 0; ob < n_obj; ob++) {
            const int32_t root = s.obj_range[ob].x;
            const float4 a = nodes4[2 * (size_t)root], b = nodes4[2 * (size_t)root + 1];
            const bool pass = slab_pass<FILTER>(o, dd, rc, a.x, a.y, a.z, a.w, b.x, b.y);
            any |= pass;
            if (pass && ob < 32u) pmask |= 1u << ob;
        }
    } else {
        // G objects at a time (2 for scenes of one or two objects, else 4)
        auto group = [&](const uint32_t ob0, auto G_) {
            constexpr uint32_t G = decltype(G_)::value;
            float4 a[G], b[G];
#pragma unroll
            for (uint32_t k = 0; k < G; k++) {
                const uint32_t ob = ob0 + k < n_obj ? ob0 + k : n_obj - 1u;
                a[k] = rn4[2 * (size_t)ob]; b[k] = rn4[2 * (size_t)ob + 1];
            }
            // (a slot beyond the last object repeats the last object: same bit.)  The filtered tests are one straight line of code, so
            // the loads above stay together at its head; what the filter could not decide is settled afterwards by the exact form
            bool pass[G], amb[G];
            bool any_amb = false;
#pragma unroll
            for (uint32_t k = 0; k < G; k++) {
                if (FILTER) pass[k] = ray_aabb_filtered(o, rc, a[k].x, a[k].y, a[k].z, a[k].w, b[k].x, b[k].y, amb[k]);
                else { pass[k] = ray_aabb_nb(o, dd, a[k].x, a[k].y, a[k].z, a[k].w, b[k].x, b[k].y); amb[k] = false; }
                any_amb |= amb[k];
            }
            if (FILTER && any_amb) {
#pragma unroll
                for (uint32_t k = 0; k < G; k++) if (amb[k]) pass[k] = ray_aabb_nb(o, dd, a[k].x, a[k].y, a[k].z, a[k].w, b[k].x, b[k].y);
            }
#pragma unroll
            for (uint32_t k = 0; k < G; k++) {
                const uint32_t ob = ob0 + k < n_obj ? ob0 + k : n_obj - 1u;
                any |= pass[k];
                if (pass[k] && ob < 32u) pmask |= 1u << ob;
            }
        };
        if (n_obj <= 2u) group(0u, std::integral_constant<uint32_t, 2>());
        else for (uint32_t ob0 = 0; ob0 < n_obj; ob0 += 4u) group(ob0, std::integral_constant<uint32_t, 4>());
    }
    if (root_pass) root_pass[root_half_stride ? (lane >> 5) * root_half_stride + (lane & 31u) : lane] = live ? pmask : 0u;
    const unsigned long long m = __ballot(live && any);
    if (m == 0ull) {
        if (live) {      // what closest_hit_phase writes for a miss
            const size_t pix = (size_t)r * p.W + px;
            hit_id[pix] = -1;
            t_out[pix] = __builtin_inff();
            store_miss(rgb_linear, rgb8, pix, p.bg);
        }
        if (shadow_bits) {
            const size_t tile_index = (size_t)by * gx + bx;
            for (uint32_t l = lane; l < p.n_lights; l += 64) shadow_bits[tile_index * p.n_lights + l] = 0ull;
        }
    }
    return m != 0ull;
}

template <bool FILTER, bool CAM = false>
__device__ __forceinline__ bool finish_background_tile(const DevScene& s, const DevParams& p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                       float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                       unsigned long long* __restrict__ shadow_bits,
                                                       const uint32_t bx, const uint32_t by, const uint32_t gx,
                                                       uint32_t* root_pass = nullptr,        // LDS, 64 words (quadrant * 16 + pixel): out, per ray the objects whose root box it passes
                                                       const uint32_t root_half_stride = 0) {
    __shared__ uint32_t tile_live;
    if ((threadIdx.x >> 6) == 0) {
        const bool live = background_test_wave<FILTER, CAM>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, bx, by, gx, root_pass, root_half_stride);
        if ((threadIdx.x & 63) == 0) tile_live = live ? 1u : 0u;
    }
    __syncthreads();
    return tile_live == 0u;
}

// COARSE: a workgroup owns 2 x 2 tiles (16 x 16 pixels): its four waves put one tile's 64 rays each through the root boxes at once,
// then work through the live tiles one after the other (four waves per tile, as ever).  For frames that are mostly background
// (3840x2160 of the reference's scenes: 94 % of 129,600 tiles) the launch is bound by workgroup dispatch, and this is a quarter
// of the workgroups; the host picks it for big frames only (a frame full of geometry keeps the finer grid's balance).
template <bool COUNT, int NQCAP, int TWL, int THL, bool FILTER, bool COARSE = false, bool WIDE = false, int MINW = 1>
__global__ __launch_bounds__(256, MINW) void k_closest_hit_nq(DevScene s, DevParams p, int32_t* __restrict__ hit_id,
                                                        float* __restrict__ t_out, float* __restrict__ rgb_linear,
                                                        uint8_t* __restrict__ rgb8, unsigned long long* __restrict__ counters,
                                                        uint32_t* __restrict__ qcount, uint32_t* __restrict__ qlist, uint32_t qcap) {
    constexpr int P = 1 << (TWL + THL);
    __shared__ uint32_t nq_all[4][NQCAP];
    __shared__ uint32_t tq_all[4][LQ_WORDS];
    __shared__ unsigned long long best_all[4][P];
    __shared__ float4 dir_all[4][P];
    const uint32_t wave = threadIdx.x >> 6;
    int32_t id; float t; V3 d;
    if (COARSE && !COUNT && TWL == 2 && THL == 2) {
        __shared__ uint32_t root_pass4[4][64];
        __shared__ uint32_t live4[4];
        const uint32_t gx = (p.W + 7u) / 8u, gy = (p.rows + 7u) / 8u;
        {
            const uint32_t bx = blockIdx.x * 2u + (wave & 1u), by = blockIdx.y * 2u + (wave >> 1);
            bool live = false;
            if (bx < gx && by < gy) live = background_test_wave<FILTER>(s, p, hit_id, t_out, rgb_linear, rgb8, nullptr, bx, by, gx, root_pass4[wave]);
            if ((threadIdx.x & 63) == 0) live4[wave] = live ? 1u : 0u;
        }
        __syncthreads();
        const bool roots_done = s.n_objects <= 32u;
        for (uint32_t k = 0; k < 4u; k++) {
            if (!live4[k]) continue;                                  // workgroup-uniform
            closest_hit_phase<COUNT, NQCAP, TWL, THL, FILTER, false, WIDE>(s, p, nq_all[wave], tq_all[wave], best_all[wave], dir_all[wave],
                                                              hit_id, t_out, rgb_linear, rgb8, counters, id, t, d,
                                                              blockIdx.x * 2u + (k & 1u), blockIdx.y * 2u + (k >> 1), gx, wave, qcount, qlist, qcap,
                                                              roots_done ? root_pass4[k] + wave * 16 : nullptr);
        }
        return;
    }
    __shared__ uint32_t root_pass[64];
    const bool roots_done = !COUNT && TWL == 2 && THL == 2 && s.n_objects <= 32u;      // wave 0 tests every root for the tile's 64 rays first
    if (!COUNT && TWL == 2 && THL == 2 && finish_background_tile<FILTER>(s, p, hit_id, t_out, rgb_linear, rgb8, nullptr, blockIdx.x, blockIdx.y, gridDim.x, root_pass)) return;
    closest_hit_phase<COUNT, NQCAP, TWL, THL, FILTER, false, WIDE>(s, p, nq_all[wave], tq_all[wave], best_all[wave], dir_all[wave],
                                                      hit_id, t_out, rgb_linear, rgb8, counters, id, t, d, blockIdx.x, blockIdx.y, gridDim.x, wave, qcount, qlist, qcap,
                                                      roots_done ? root_pass + wave * 16 : nullptr);
}

// =================================================================================================
// Kernel 2: shadow rays + shading + tone map.  softShadow:348-401 -> shadowIntersection:321-342 +
// phongIllumination:144-200, then the pixel (store_pixel).  Shading runs once, for the closest hit (the
// reference re-shades every improving hit and keeps the last: same value).  The hit object's own tree is
// skipped (the reference walks it and discards the result, :328/:331) and the any-hit walk exits at the
// first hit.
// =================================================================================================
// One shadow ray on its own lane: shadowIntersection:321-342 over every node outside [self.x, self.y), t unbounded, any
// Moller-Trumbore result other than -inf counts (NaN included); the lane leaves at its first hit.
// FILTER: the slab test through slab_pass (reciprocal filter, exact fallback) instead of the exact divides alone -- the same answers.
// COUNT: the oracle's algorithmic counts -- objects in order, one slab test per node met, one triangle test up to and including the
// first hit.
// RANGE (the occlusion query with a t interval, srt_query.h): a result counts only if it is in range, !(t < t_min) && !(t > t_max) --
// closed, a NaN bound bounds nothing, a NaN t is in range; the walk visits the same nodes, and the lane leaves at its first hit in range.
// MASK (visibility masks, include/srt.h): object k takes part iff (obj_mask[k] & ray_m) != 0, a NULL obj_mask reading as all ones.  The
// objects' ranges are contiguous and i only moves forward, so the lane keeps a cursor -- obj_cur, the object whose root comes next, and
// obj_root, that root's index.  Whenever i arrives there the cursor moves on, and a hidden object is stepped over like `self`: no record of
// it is read, nothing is tested or counted.  Each jump goes back to the loop's head, so a self range or a hidden object (or an object
// without nodes) that follows is met in turn.
template <bool COUNT, bool FILTER, bool RANGE = false, bool MASK = false>
__device__ __forceinline__ bool any_hit_range(const DevScene& s, int2 self, V3 so, V3 sd,
                                              unsigned long long& n_node, unsigned long long& n_tri, const float t_min = 0.0f, const float t_max = 0.0f,
                                              const uint32_t* __restrict__ obj_mask = nullptr, const uint32_t ray_m = 0u) {
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    RayRcp rc;
    if (FILTER) rc = ray_rcp(so, sd);      // (FILTER: the ray queries, whose origins a caller supplies)
    const int32_t n = (int32_t)s.n_nodes;
    int32_t i = 0;
    int32_t obj_root = 0;
    uint32_t obj_cur = 0;
    bool hit = false;
    while (i < n && !hit) {
        if (MASK && i == obj_root && obj_cur < s.n_objects) {
            const int2 r = s.obj_range[obj_cur];
            const uint32_t om = obj_mask ? obj_mask[obj_cur] : 0xFFFFFFFFu;
            obj_cur++;
            obj_root = r.y;
            if (!(om & ray_m)) i = r.y;
            continue;
        }
        if (i == self.x) { i = self.y; continue; }
        const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
        const int32_t skip = __float_as_int(b.z), leaf = __float_as_int(b.w);
        if (COUNT) n_node++;
        if (FILTER ? slab_pass<true>(so, sd, rc, a.x, a.y, a.z, a.w, b.x, b.y) : ray_aabb(so, sd, a.x, a.y, a.z, a.w, b.x, b.y)) {
            if (leaf >= 0) {
                const int32_t first = leaf >> LEAF_SHIFT, cnt = leaf & LEAF_MAX;
                for (int32_t k = 0; k < cnt && !hit; k++) {
                    V3 p1, e1, e2;
                    load_tri_edges(tris4, (size_t)(first + k), p1, e1, e2);
                    if (COUNT) n_tri++;
                    const float t = ray_triangle(so, sd, p1, e1, e2);
                    hit = t != SRT_NEG_INF && (!RANGE || (!(t < t_min) && !(t > t_max)));      // any t >= 0, NaN included (:335)
                }
            }
            i = i + 1;
        } else {
            i = skip;
        }
    }
    return hit;
}

// What shading needs to know of the surface at a hit.
struct Surface {
    V3 color;              // the object's colour (:437-440), or the texel under the hit point (:350-361)
    V3 nrm;                // the face normal, or interpolateNormal's (phongIllumination:159,162, opt-in mode)
    float ka, ks, sh;
};
// The surface of triangle `id` where the ray o + d * t meets it.  The barycentric coordinates are taken once, for a textured triangle
// and for smooth normals.
__device__ __forceinline__ Surface surface_at(const DevScene& s, const int32_t id, const V3 o, const V3 d, const float t, const bool smooth) {
    Surface f;
    const int32_t obj = s.tri_obj[id];
    const float4* tp = reinterpret_cast<const float4*>(s.tris) + (size_t)id * 3;
    const float4 t2 = tp[2];
    f.nrm = mk(t2.y, t2.z, t2.w);
    f.color = mk(s.obj_color[obj * 3], s.obj_color[obj * 3 + 1], s.obj_color[obj * 3 + 2]);
    const int32_t tex = s.tri_tex ? s.tri_tex[id] : -1;
    V3 bc = mk(0.0f, 0.0f, 0.0f);
    if (tex >= 0 || smooth) {
        const float4 t0 = tp[0], t1 = tp[1];
        bc = barycentric(mk(t0.x, t0.y, t0.z), mk(t0.w, t1.x, t1.y), mk(t1.z, t1.w, t2.x), o + d * t);
    }
    if (tex >= 0) {
        const float* tc = s.tri_tc + (size_t)id * 6;
        const float tx = (bc.x * tc[0] + bc.y * tc[2]) + bc.z * tc[4];                          // :123-125
        const float ty = (bc.x * tc[1] + bc.y * tc[3]) + bc.z * tc[5];
        long long idx = ((long long)((int)ty * (int)s.tex_w[tex] + (int)tx)) * 3;               // :357
        // the reference reads out of bounds if the texel index leaves the image (UB); this project clamps into the texture instead
        const long long last = (long long)s.tex_size[tex] - 3;
        idx = idx < 0 ? 0 : (idx > last ? last : idx);
        const uint8_t* td = s.tex + s.tex_off[tex] + idx;
        f.color = mk(td[0] / 255.0f, td[1] / 255.0f, td[2] / 255.0f);
    }
    f.ka = s.obj_mat[obj * 3]; f.ks = s.obj_mat[obj * 3 + 1]; f.sh = s.obj_mat[obj * 3 + 2];
    if (smooth) {
        const float* n9 = s.tri_normals + (size_t)id * 9;
        f.nrm = normalize3(mk((bc.x * n9[0] + bc.y * n9[3]) + bc.z * n9[6], (bc.x * n9[1] + bc.y * n9[4]) + bc.z * n9[7],
                              (bc.x * n9[2] + bc.y * n9[5]) + bc.z * n9[8]));
    }
    return f;
}

// The light-sample sum of softShadow:366-383 over samples [l0, l0 + m), in light order: Phong per sample, a shadowed sample divided
// (:369), one f32 add per component and sample into `sum` (:370).  `shadowed(l)` says whether sample l's shadow ray was blocked.
template <bool INT_SHIN, typename SH>
__device__ __forceinline__ void add_light_samples(V3& sum, const Surface& f, const V3 o, const V3 d, const float t, const float* __restrict__ lights,
                                                  const uint32_t l0, const uint32_t m, const float shadow_div, SH shadowed) {
    for (uint32_t l = l0; l < l0 + m; l++) {
        const float* lp = lights + (size_t)l * 3;
        const V3 L = mk(lp[0], lp[1], lp[2]);
        const bool sd = shadowed(l);
        V3 c = phong<INT_SHIN>(f.nrm, o, d, L, f.color, f.ka, f.ks, f.sh, t);
        if (sd) c = mk(c.x / shadow_div, c.y / shadow_div, c.z / shadow_div);
        sum = sum + c;
    }
}

// One thread per pixel: the shadow rays walk on their own lanes (exact slab test: variant 1 and its counts are defined by it).
template <bool COUNT>
__global__ __launch_bounds__(256) void k_shade(DevScene s, DevParams p, const int32_t* __restrict__ hit_id,
                                               const float* __restrict__ t_in, float* __restrict__ rgb_linear,
                                               uint8_t* __restrict__ rgb8, unsigned long long* __restrict__ counters,
                                               unsigned long long* __restrict__ counters_next) {
    if (counters_next) zero_next_counters(counters_next);
    uint32_t px, r;
    const bool live = tile_pixel(p, px, r);
    unsigned long long n_node = 0, n_tri = 0;
    bool is_hit = false;
    if (live) {
        const size_t pix = (size_t)r * p.W + px;
        const int32_t id = hit_id[pix];
        V3 sum = mk(0.0f, 0.0f, 0.0f);
        if (id >= 0) {
            is_hit = true;
            const float t = t_in[pix];
            const V3 o = mk(0.0f, 0.0f, 0.0f);
            const V3 d = primary_dir(p, px, image_row(p, r));
            const Surface f = surface_at(s, id, o, d, t, false);
            const int2 self = s.obj_range[s.tri_obj[id]];
            const V3 dt = d * t;                      // shadowIntersection:325-326: origin d*t, dir L - d*t
            add_light_samples<false>(sum, f, o, d, t, p.lights, 0u, p.n_lights, p.shadow_div, [&](uint32_t l) -> bool {
                const V3 L = mk(p.lights[l * 3], p.lights[l * 3 + 1], p.lights[l * 3 + 2]);
                return any_hit_range<COUNT, false>(s, self, dt, L - dt, n_node, n_tri);
            });
        }
        store_pixel(rgb_linear, rgb8, pix, sum, is_hit, p.reinhard, p.gamma, p.bg, p.exp);
    }
    count_hits(counters, is_hit, blockIdx.y * gridDim.x + blockIdx.x);
    if (COUNT) { wave_add(counters + 3, n_node); wave_add(counters + 4, n_tri); }
}


// =================================================================================================
// Kernel 2a: shadow rays, node-queue form.  A 256-thread workgroup owns an 8x8 pixel tile, each of its
// four wavefronts a 4x4 quadrant.  A wave compacts its hit pixels (ballot + rank) and walks work items
// (hit pixel, light sample) 16 rays at a time with the same two LDS queues as the closest-hit kernel:
// 64 lanes serve 16 rays, so lanes stay full whatever the hit pattern, and with many light samples the
// rays of a step share their origin.  shadowIntersection:321-342: origin d*t, direction L - d*t
// (unnormalised, no epsilon); any candidate of ANOTHER object with Moller-Trumbore != -inf (NaN included)
// shadows.  A hit raises the ray's flag; queued pairs of a flagged ray are dropped when popped.
// Result: per 8x8 tile and light sample one 64-bit word of four 16-bit fields, field = quadrant (wave), bit = y*4 + x inside it.
// SEQ = true is the counting build: per-ray sequential pre-order walk with exit at the first hit, whose
// slab / triangle test counts are the algorithmic counts the CPU oracle mirrors.
// =================================================================================================
// Per-wave LDS of the shadow phase (beside the two queues)
template <int RS, int P = NQ_P>    // RS = shadow rays in flight per round: 16, or 64 when there are many light samples; P = pixels of the wave
struct ShadowLds {
    float4 ray[2 * RS];            // per ray slot: origin, direction
    float4 pixd[P];                // per hit rank: t, pixel lane, own object's node range
    float4 pso[P];                 // per hit rank: the shadow rays' origin d * t (:326)
    int2 selfr[RS];                // per ray slot: node range of the hit object
    uint32_t flag[RS];
    uint32_t mask[64];             // per light sample of the current group: shadowed pixels of this wave's 4x4 quadrant (P = 32: of its 8x4 half)
};

// Per-wave LDS of the half-tile trace kernel (trace_nq_body's HALF) beside the two queues: the closest-hit phase's dir[] and best[] lie
// over the front of the shadow phase's ShadowLds, 768 B a wave less, which with 512-entry queues is 11,144 B a workgroup -- nine
// 1,280-byte granules, fourteen workgroups per 160 KiB CU where the separate arrays (ten granules) admitted twelve.  Per wave:
//
//   data                                  written                                      read                                      dead after
//   dir[P]                                set-up of closest_hit_phase                  every node step and triangle batch; last  the write-out
//                                                                                      read dir[lane] at the phase's write-out
//   best[P]                               set-up of closest_hit_phase                  last read best[lane] at the write-out     the write-out
//   shadow.mask[0 .. 31] of wave h (the   by wave 0, before the launch-time barrier    only while closest_hit_phase queues the   rewritten by wave h in
//   tile's root masks, rays 32h ..)       (finish_background_tile)                     roots                                     its own shadow phase
//   shadow.ray, pixd, pso, selfr, flag    first in shadow_phase, from id, t and d      in shadow_phase                           end of the shadow phase
//                                         held in registers
//
// So `closest` may share bytes with ray / pixd / pso / selfr / flag and never with mask, which is live through the closest-hit phase: it
// ends at or before mask's offset.  One object with two views, so that the compiler knows the views alias; trace_nq_body keeps the
// phases' accesses apart (a wavefront fence and the wave barrier between them).  ShadowLds itself is what every other kernel declares.
template <int RS, int P>
union HalfTileLds {
    struct { float4 dir[P]; unsigned long long best[P]; } closest;
    ShadowLds<RS, P> shadow;
};

// Runs per wavefront, with no workgroup-level synchronisation: `id` / `t_hit` are the hit id and t of this lane's pixel
// (lanes < 16; -1 = miss).  The wave writes its own 16-bit field of the tile's word (field = quadrant, bit = pixel lane
// y * 4 + x inside the quadrant), so a wave that is done leaves the CU without waiting for its three neighbours.
// P = 32: the wave owns half `wave` of the tile (closest_hit_phase's HALF: lanes < 32, pixel lane = quadrant of the half * 16 + y * 4 + x)
// and writes the 32-bit half `wave` of the tile's word -- fields 2 * wave and 2 * wave + 1 -- in one store.
// PAIRS: the triangle loop over pairs of tests with two named records, as closest_hit_phase's.
template <bool SEQ, int NQCAP, bool FILTER, int RS, bool EARLY = true, bool WIDE = false, int P = NQ_P, bool PAIRS = false>
__device__ __forceinline__ void shadow_phase(const DevScene& s, const DevParams& p, uint32_t* nq, uint32_t* tq, ShadowLds<RS, P>& L,
                                             int32_t id, float t_hit, V3 d_hit,
                                             unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                                             const uint32_t bx, const uint32_t by, const uint32_t gx, const uint32_t wave,
                                             const uint32_t l_begin = 0u, const uint32_t l_end_ = 0xffffffffu) {   // light samples [l_begin, l_end) of p.n_lights
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t l_end = l_end_ < p.n_lights ? l_end_ : p.n_lights;
    float4* ray = L.ray;
    int2* selfr = L.selfr;
    uint32_t* flag = L.flag;
    float4* pixd = L.pixd;
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    static_assert(P == 16 || P == 32, "a wave owns a 4x4 quadrant or an 8x4 half of the tile");
    const uint32_t qx = P == 32 ? (lane >> 4) & 1u : wave & 1, qy = P == 32 ? 0u : wave >> 1;
    const uint32_t tile_x = bx * 8 + qx * 4, tile_r = by * 8 + (P == 32 ? wave * 4 : qy * 4);
    const uint32_t px = tile_x + (lane & 3), r = tile_r + ((lane >> 2) & 3);
    const bool live = lane < P && pixel_live(p, px, r);
    const size_t tile_index = (size_t)by * gx + bx;
    const uint32_t wave_s = __builtin_amdgcn_readfirstlane(wave);      // wave-uniform: waits for the stores at the end in a scalar register
    unsigned long long n_node = 0, n_tri = 0;
    if (!live) id = -1;
    const uint32_t hm = (uint32_t)__ballot(id >= 0);
    const uint32_t nh = (uint32_t)__popc(hm);
    int32_t self_root = -2;
    V3 so_mine = mk(0.f, 0.f, 0.f);
    if (id >= 0) {
        const int2 self = s.obj_range[s.tri_obj[id]];
        const uint32_t rank = __popc(hm & ((1u << lane) - 1u));
        pixd[rank] = make_float4(t_hit, __uint_as_float(lane), __int_as_float(self.x), __int_as_float(self.y));
        V3 so_px = d_hit * t_hit;                                      // :326
        if (p.cam) so_px = ray_origin(p) + so_px;                      // camera mode: the primary ray did not start at 0
        L.pso[rank] = make_float4(so_px.x, so_px.y, so_px.z, 0.f);
        self_root = self.x; so_mine = so_px;
    }
    // Quick reject (EARLY): on most quadrants of the ground no shadow ray passes the ROOT box of any other object, and the queue
    // machinery below is a chain of dependent steps to find that out (profiles/diag_timeline_parts.py: the waves of slab tiles hold 22
    // of a CU's 24 wave slots, so a wave's lifetime IS the throughput).  So the wave first puts every (ray, light sample, other
    // object) through that root's slab test -- the test the first node step would run -- at 16 rays x 4 combinations per pass; if
    // nothing passes, the quadrant's shadow words are zero.  K3 with 4 light samples: 0.210 -> 0.187 ms per frame.  (P = 32: 32 rays x 2.)
    const uint32_t n_combo = (l_end - l_begin) * s.n_objects;
    if (!SEQ && EARLY && l_end > l_begin && (nh == 0u || n_combo <= 64u)) {
        const uint32_t rl = lane & (uint32_t)(P - 1), slot = lane / (uint32_t)P;
        const float sx = __shfl(so_mine.x, (int)rl, 64), sy = __shfl(so_mine.y, (int)rl, 64), sz = __shfl(so_mine.z, (int)rl, 64);
        const int32_t sroot = __shfl(self_root, (int)rl, 64);
        const V3 so = mk(sx, sy, sz);
        bool pass_any = false;
        if (sroot != -2 && nh) {
            for (uint32_t c = slot; c < n_combo; c += 64u / (uint32_t)P) {
                const uint32_t lq = c / s.n_objects, ob = c - lq * s.n_objects, l = l_begin + lq;
                const int32_t root = s.obj_range[ob].x;
                const float4 a = reinterpret_cast<const float4*>(s.root_nodes)[2 * (size_t)ob], b = reinterpret_cast<const float4*>(s.root_nodes)[2 * (size_t)ob + 1];      // (independent of `root`)
                if (root == sroot) continue;                          // never the hit object's own tree (:331)
                const V3 sd = mk(p.lights[l * 3], p.lights[l * 3 + 1], p.lights[l * 3 + 2]) - so;      // :325
                bool pass;
                if (FILTER) {
                    bool amb;
                    pass = ray_aabb_filtered(so, ray_rcp(sd), a.x, a.y, a.z, a.w, b.x, b.y, amb);
                    if (amb) pass = ray_aabb_nb(so, sd, a.x, a.y, a.z, a.w, b.x, b.y);
                } else pass = ray_aabb_nb(so, sd, a.x, a.y, a.z, a.w, b.x, b.y);
                pass_any |= pass;
            }
        }
        if (!__ballot(pass_any)) {
            L.mask[lane] = 0u;                                        // (read by the wave that shades the tile in the one-launch build)
            if (shadow_bits) for (uint32_t l = l_begin + lane; l < l_end; l += 64u) {
                if (P == 32) reinterpret_cast<uint32_t*>(shadow_bits)[(tile_index * p.n_lights + l) * 2 + wave_s] = 0u;
                else reinterpret_cast<uint16_t*>(shadow_bits)[(tile_index * p.n_lights + l) * 4 + wave_s] = 0;
            }
            return;
        }
    }
    uint32_t nqn = 0, tqn = 0;
    unsigned long long dg_k = 0, dg_m = 0, dg_steps = 0;      // (diagnostic, variant 47)

    // one batch of <= 64 queued (leaf, ray) pairs: the lane walks the leaf's triangles until one hits
    auto tri_batch = [&]() {
        const uint32_t m = tqn < 64 ? tqn : 64;
        tqn -= m;
        const uint32_t lt = lane_again(lane);
        if (lt < m) {
            const uint32_t info = tq[2 * (tqn + lt)], rs = tq[2 * (tqn + lt) + 1];
            if (!flag[rs]) {
                const uint32_t first = info >> LEAF_SHIFT, cnt = info & LEAF_MAX;
                const float4 ro4 = ray[rs], rd4 = ray[RS + rs];
                const V3 ro = mk(ro4.x, ro4.y, ro4.z), rd = mk(rd4.x, rd4.y, rd4.z);
                const float4* tp = tris4 + (size_t)first * 3;
                float4 t0 = tp[0], t1 = tp[1];
                float e2z = reinterpret_cast<const float*>(tp + 2)[0];
                bool hit = false;
                if constexpr (PAIRS) {
                    // two named records instead of the rotation (closest_hit_phase's pair loop): the same tests in the same order, the stop at
                    // the first hit -- a record already requested is simply not used
                    auto test = [&](const float4 c0, const float4 c1, const float c2) -> bool {
                        return ray_triangle(ro, rd, mk(c0.x, c0.y, c0.z), mk(c0.w, c1.x, c1.y), mk(c1.z, c1.w, c2)) != SRT_NEG_INF;      // any t >= 0, NaN included (:335)
                    };
                    float4 u0, u1; float u2;
                    uint32_t k = 0;
                    bool have_a = cnt != 0u;
                    while (have_a && k + 1 < cnt) {
                        tp += 3; u0 = tp[0]; u1 = tp[1]; u2 = reinterpret_cast<const float*>(tp + 2)[0];
                        hit = test(t0, t1, e2z);
                        have_a = k + 2 < cnt;
                        if (!hit) {
                            if (have_a) { tp += 3; t0 = tp[0]; t1 = tp[1]; e2z = reinterpret_cast<const float*>(tp + 2)[0]; }
                            hit = test(u0, u1, u2);
                        }
                        k += 2;
                        if (hit) have_a = false;
                    }
                    if (have_a) hit = test(t0, t1, e2z);
                } else
                for (uint32_t k = 0; k < cnt && !hit; k++) {
                    const float4 c0_ = t0, c1_ = t1; const float cz = e2z;
                    if (k + 1 < cnt) { tp += 3; t0 = tp[0]; t1 = tp[1]; e2z = reinterpret_cast<const float*>(tp + 2)[0]; }
                    const float t = ray_triangle(ro, rd, mk(c0_.x, c0_.y, c0_.z), mk(c0_.w, c1_.x, c1_.y), mk(c1_.z, c1_.w, cz));
                    hit = t != SRT_NEG_INF;                          // any t >= 0, NaN included (:335)
                }
                if (hit) flag[rs] = 1u;
            }
        }
        __builtin_amdgcn_wave_barrier();
    };
    // (the two-leaf push stays a copy of leaf_queue_push2 here: sharing it changes the code of the wide filtered shadow kernels)
    auto push_tris2 = [&](uint32_t info_a, bool leaf_a, uint32_t info_b, bool leaf_b, uint32_t rs) {
        const unsigned long long ma = __ballot(leaf_a), mb = __ballot(leaf_b);
        if (ma | mb) {
            uint32_t pos = tqn + lane_prefix(ma) + lane_prefix(mb), q = pos + (leaf_a ? 1u : 0u);
            if (!(p.exp & 1u)) { pos = tqn + lane_prefix(ma); q = tqn + (uint32_t)__popcll(ma) + lane_prefix(mb); }      // node-major
            if (leaf_a) { tq[2 * pos] = info_a; tq[2 * pos + 1] = rs; }
            if (leaf_b) { tq[2 * q] = info_b; tq[2 * q + 1] = rs; }
            tqn += (uint32_t)__popcll(ma) + (uint32_t)__popcll(mb);
            __builtin_amdgcn_wave_barrier();
            while (tqn >= 64) tri_batch();
        }
    };
    const float4* wide4 = reinterpret_cast<const float4*>(s.wide);

    constexpr uint32_t OBJ_G = (NQCAP / (2 * RS)) < 16 ? (NQCAP / (2 * RS)) : 16;     // RS * OBJ_G <= NQCAP / 2
    const uint32_t n_obj = s.n_objects;
    for (uint32_t l0 = l_begin; l0 < l_end; l0 += 64) {              // light samples in groups of 64
        const uint32_t Lg = (l_end - l0) < 64u ? (l_end - l0) : 64u;
        L.mask[lane_again(lane)] = 0u;
        __builtin_amdgcn_wave_barrier();
        const uint32_t n_items = nh * Lg;
        // item / Lg below as a multiplication: exact for item < 16 * Lg, Lg <= 64 ((65536 / Lg + 1) * Lg - 65536 <= Lg, and item < 65536 / Lg).
        // Wave-uniform, so it waits in a scalar register; the reciprocal of a per-lane division waited in a vector register, or in scratch.
        // (32 pixels: item < 32 * Lg reaches 2 * 65536 / Lg, so the scale is 2^20 there -- (2^20 / Lg + 1) * Lg - 2^20 <= Lg, item < 2^20 / Lg,
        // and item * (2^20 + 1) < 2^32.)
        constexpr uint32_t LG_SHIFT = P == 32 ? 20u : 16u;
        const uint32_t lg_magic = __builtin_amdgcn_readfirstlane((1u << LG_SHIFT) / Lg + 1u);
        for (uint32_t base = 0; base < n_items; base += RS) {        // RS rays per round
            const uint32_t ln = lane_again(lane);                 // (the slots' addresses are formed here, not kept across the rounds)
            const uint32_t item = base + ln;
            const bool valid = ln < RS && item < n_items;
            uint32_t pl = 0, lg = 0;
            V3 so = mk(0.f, 0.f, 0.f), sd = mk(0.f, 0.f, 1.f);
            int2 self = make_int2(-1, -1);
            if (valid) {
                const uint32_t hr = (Lg == 1u) ? item : (item * lg_magic) >> LG_SHIFT;
                lg = item - hr * Lg;
                const float4 pd = pixd[hr];
                pl = __float_as_uint(pd.y);
                self = make_int2(__float_as_int(pd.z), __float_as_int(pd.w));
                const float4 so4 = L.pso[hr];
                const uint32_t l = l0 + lg;
                const V3 L = mk(p.lights[l * 3], p.lights[l * 3 + 1], p.lights[l * 3 + 2]);
                so = mk(so4.x, so4.y, so4.z);
                sd = L - so;                                      // :325
            }
            bool shadowed = false;
            if (SEQ) {
                if (valid) shadowed = any_hit_range<true, false>(s, self, so, sd, n_node, n_tri);
            } else {
                if (ln < RS) {      // (.w, which no test reads: the ray's pixel lane and light sample wait here during the walk, not in registers)
                    ray[ln] = make_float4(so.x, so.y, so.z, __uint_as_float(pl));
                    ray[RS + ln] = make_float4(sd.x, sd.y, sd.z, __uint_as_float(lg));
                    selfr[ln] = self;
                    flag[ln] = valid ? 0u : 1u;
                }
                const unsigned long long validm = __ballot(valid);
                __builtin_amdgcn_wave_barrier();
                if constexpr (WIDE) {
                for (uint32_t obj0 = 0; obj0 < n_obj; obj0 += OBJ_G) {
                    const uint32_t g = (n_obj - obj0) < OBJ_G ? (n_obj - obj0) : OBJ_G;
                    // the other objects' roots, one (ray, object) pair per lane: a passing inner root is queued, a passing leaf's triangles are
                    for (uint32_t kb = 0; kb < RS * g; kb += 64) {
                        const uint32_t k = kb + lane_again(lane);
                        const uint32_t rs = k & (RS - 1), ob = k / RS;
                        bool ok = k < RS * g && ((validm >> rs) & 1ull);
                        int32_t info = 0;
                        if (ok) {
                            const int32_t root = s.obj_range[obj0 + ob].x;
                            ok = root != selfr[rs].x && !flag[rs];                 // never the hit object's own tree (:331)
                            if (ok) {
                                const float4* rn = reinterpret_cast<const float4*>(s.root_nodes) + 2 * (size_t)(obj0 + ob);
                                const float4 a = rn[0], b = rn[1];
                                const float4 o4 = ray[rs], d4 = ray[RS + rs];
                                const V3 ro = mk(o4.x, o4.y, o4.z), rd = mk(d4.x, d4.y, d4.z);
                                ok = slab_pass<FILTER>(ro, rd, ray_rcp(rd), a.x, a.y, a.z, a.w, b.x, b.y);
                                if (ok) info = s.obj_root_info[obj0 + ob];
                            }
                        }
                        const bool inner = ok && info < 0, leafp = ok && info >= 0 && (info & LEAF_MAX) != 0;
                        const unsigned long long im = __ballot(inner);
                        if (inner) nq[nqn + lane_prefix(im)] = ((uint32_t)(~info) << 6) | rs;
                        nqn += (uint32_t)__popcll(im);
                        push_tris2((uint32_t)info, leafp, 0u, false, rs);
                    }
                    __builtin_amdgcn_wave_barrier();
                    while (nqn) {
                        const uint32_t m = nqn < 64 ? nqn : 64;
                        nqn -= m;
                        uint32_t rs = 0;
                        int32_t linfo = 0, rinfo = 0, node = 0, rnode = 0;
                        bool in_l = false, in_r = false, lf_l = false, lf_r = false;
                        V3 ro = mk(0.f, 0.f, 0.f), rd = mk(0.f, 0.f, 1.f);
                        if (p.exp & 4u) {        // diagnostic (variant 47): how many DISTINCT records does a step read?
                            const uint32_t e_ = lane < m ? nq[nqn + lane] : 0xffffffffu;
                            const uint32_t w_ = e_ >> 6, prev_ = (uint32_t)__shfl_up((int)w_, 1, 64);
                            const bool live_ = lane < m && !flag[e_ & 63u];
                            dg_k += (unsigned long long)__popcll(__ballot(live_ && (lane == 0 || w_ != prev_)));
                            dg_m += (unsigned long long)__popcll(__ballot(live_));
                            dg_steps++;
                        }
                        if (lane < m) {
                            const uint32_t e = nq[nqn + lane];
                            rs = e & 63u;
                            if (!flag[rs]) {                          // already shadowed rays drop their queued pairs
                                const float4* wp = wide4 + 4 * (size_t)(e >> 6);
                                const float4 r0 = wp[0], r1 = wp[1], r2 = wp[2];
                                const int4 r3 = reinterpret_cast<const int4*>(wp)[3];
                                const float4 o4 = ray[rs], d4 = ray[RS + rs];
                                ro = mk(o4.x, o4.y, o4.z); rd = mk(d4.x, d4.y, d4.z);
                                linfo = r3.x; rinfo = r3.y; node = r3.z; rnode = r3.w;
                                bool pass_l, pass_r;
                                slab_pass2<FILTER>(ro, rd, ray_rcp(rd), r0, r1, r2, pass_l, pass_r);
                                in_l = pass_l && linfo < 0; lf_l = pass_l && linfo >= 0 && (linfo & LEAF_MAX) != 0;
                                in_r = pass_r && rinfo < 0; lf_r = pass_r && rinfo >= 0 && (rinfo & LEAF_MAX) != 0;
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        const unsigned long long ml = __ballot(in_l), mr = __ballot(in_r);
                        const uint32_t n_in = (uint32_t)__popcll(ml) + (uint32_t)__popcll(mr);
                        if (nqn + n_in <= (uint32_t)NQCAP) {
                            if (!(p.exp & 1u)) {
                                if (in_r) nq[nqn + lane_prefix(mr)] = ((uint32_t)(~rinfo) << 6) | rs;
                                if (in_l) nq[nqn + (uint32_t)__popcll(mr) + lane_prefix(ml)] = ((uint32_t)(~linfo) << 6) | rs;
                            } else {
                            const uint32_t pos = nqn + lane_prefix(ml) + lane_prefix(mr);
                            if (in_r) nq[pos] = ((uint32_t)(~rinfo) << 6) | rs;
                            if (in_l) nq[pos + (in_r ? 1u : 0u)] = ((uint32_t)(~linfo) << 6) | rs;
                            }
                            nqn += n_in;
                            push_tris2((uint32_t)linfo, lf_l, (uint32_t)rinfo, lf_r, rs);
                        } else {
                            // queue full: the passing children's subtrees by the stackless walk
                            push_tris2((uint32_t)linfo, lf_l, (uint32_t)rinfo, lf_r, rs);
                            int32_t i = 0, end = 0, hop = -1;
                            if (in_l | in_r) {
                                i = in_l ? node + 2 : rnode + 1;
                                end = in_r ? s.nodes[rnode].skip : rnode;
                                hop = (in_l && in_r) ? rnode : -1;
                            }
                            while (__ballot(i < end)) {
                                int32_t inf2 = -1;
                                bool lp2 = false;
                                if (i < end) {
                                    if (flag[rs]) i = end;
                                    else if (i == hop) i = hop + 1;
                                    else {
                                        const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
                                        const int32_t sk = __float_as_int(b.z);
                                        inf2 = __float_as_int(b.w);
                                        if (ray_aabb_nb(ro, rd, a.x, a.y, a.z, a.w, b.x, b.y)) {
                                            lp2 = inf2 >= 0 && (inf2 & LEAF_MAX) != 0;
                                            i = i + 1;
                                        } else {
                                            i = sk;
                                        }
                                    }
                                }
                                push_tris2((uint32_t)inf2, lp2, 0u, false, rs);
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                } else
                for (uint32_t obj0 = 0; obj0 < n_obj; obj0 += OBJ_G) {
                    const uint32_t g = (n_obj - obj0) < OBJ_G ? (n_obj - obj0) : OBJ_G;
                    for (uint32_t kb = 0; kb < RS * g; kb += 64) {
                        const uint32_t k = kb + lane_again(lane);
                        const uint32_t rs = k & (RS - 1), ob = k / RS;
                        bool ok = k < RS * g && ((validm >> rs) & 1ull);
                        int32_t root = 0;
                        if (ok) { root = s.obj_range[obj0 + ob].x; ok = root != selfr[rs].x; }   // never the hit object's own tree (:331)
                        const unsigned long long m = __ballot(ok);
                        if (ok) nq[nqn + lane_prefix(m)] = ((uint32_t)root << 6) | rs;
                        nqn += (uint32_t)__popcll(m);
                    }
                    __builtin_amdgcn_wave_barrier();
                    while (nqn) {
                        const uint32_t m = nqn < 64 ? nqn : 64;
                        nqn -= m;
                        uint32_t rs = 0;
                        int32_t node = 0, info = -1, skip = 0;
                        bool inner = false, leafp = false;
                        V3 ro = mk(0.f, 0.f, 0.f), rd = mk(0.f, 0.f, 1.f);
                        if (lane < m) {
                            const uint32_t e = nq[nqn + lane];
                            rs = e & 63u; node = (int32_t)(e >> 6);
                            if (!flag[rs]) {                          // already shadowed rays drop their queued pairs
                                const float4 a = nodes4[2 * (size_t)node], b = nodes4[2 * (size_t)node + 1];
                                const float4 o4 = ray[rs], d4 = ray[RS + rs];
                                ro = mk(o4.x, o4.y, o4.z); rd = mk(d4.x, d4.y, d4.z);
                                skip = __float_as_int(b.z); info = __float_as_int(b.w);
                                bool pass;
                                if (FILTER) {
                                    bool amb;
                                    pass = ray_aabb_filtered(ro, ray_rcp(rd), a.x, a.y, a.z, a.w, b.x, b.y, amb);
                                    if (amb) pass = ray_aabb_nb(ro, rd, a.x, a.y, a.z, a.w, b.x, b.y);
                                } else {
                                    pass = ray_aabb_nb(ro, rd, a.x, a.y, a.z, a.w, b.x, b.y);
                                }
                                if (pass) {
                                    if (info < 0) inner = true;
                                    else leafp = (info & LEAF_MAX) != 0;
                                }
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                        const unsigned long long im = __ballot(inner);
                        const uint32_t n_in = (uint32_t)__popcll(im);
                        if (nqn + 2 * n_in <= (uint32_t)NQCAP) {
                            if (inner) {
                                uint32_t pos = nqn + 2 * lane_prefix(im), pos1 = pos + 1;
                                if (!(p.exp & 1u)) { pos = nqn + lane_prefix(im); pos1 = pos + n_in; }
                                nq[pos] = ((uint32_t)(~info) << 6) | rs;
                                nq[pos1] = ((uint32_t)(node + 1) << 6) | rs;
                            }
                            nqn += 2 * n_in;
                            leaf_queue_push(tq, tqn, (uint32_t)info, leafp, rs, tri_batch);
                        } else {
                            leaf_queue_push(tq, tqn, (uint32_t)info, leafp, rs, tri_batch);
                            int32_t i = inner ? node + 1 : 0, end = inner ? skip : 0;
                            while (__ballot(i < end)) {
                                int32_t inf2 = -1;
                                bool lp2 = false;
                                if (i < end) {
                                    if (flag[rs]) { i = end; }
                                    else {
                                        const float4 a = nodes4[2 * (size_t)i], b = nodes4[2 * (size_t)i + 1];
                                        const int32_t sk = __float_as_int(b.z);
                                        inf2 = __float_as_int(b.w);
                                        if (ray_aabb_nb(ro, rd, a.x, a.y, a.z, a.w, b.x, b.y)) {
                                            lp2 = inf2 >= 0 && (inf2 & LEAF_MAX) != 0;
                                            i = i + 1;
                                        } else {
                                            i = sk;
                                        }
                                    }
                                }
                                leaf_queue_push(tq, tqn, (uint32_t)inf2, lp2, rs, tri_batch);
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                while (tqn) tri_batch();
                __builtin_amdgcn_wave_barrier();
                if (valid) {
                    const uint32_t lz = lane_again(lane);
                    shadowed = flag[lz] != 0u;
                    pl = __float_as_uint(ray[lz].w); lg = __float_as_uint(ray[RS + lz].w);
                }
                __builtin_amdgcn_wave_barrier();
            }
            if (shadowed && valid) atomicOr(&L.mask[lg], 1u << pl);
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t lw = lane_again(lane);      // (the word's address is formed here, not kept across the walk)
        if (shadow_bits && lw < Lg) {
            if (P == 32) reinterpret_cast<uint32_t*>(shadow_bits)[(tile_index * p.n_lights + l0 + lw) * 2 + wave_s] = L.mask[lw];
            else reinterpret_cast<uint16_t*>(shadow_bits)[(tile_index * p.n_lights + l0 + lw) * 4 + wave_s] = (uint16_t)L.mask[lw];
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (SEQ) { wave_add(counters + 3, n_node); wave_add(counters + 4, n_tri); }
    if (!SEQ && (p.exp & 4u) && lane == 0) { atomicAdd(counters + 5, dg_k); atomicAdd(counters + 6, dg_m); atomicAdd(counters + 7, dg_steps); }
}

// blockIdx.z = chunk of `l_chunk` light samples: with many samples a tile's shadow rays are cut over several workgroups (a
// wave that walks 16 pixels x 64 samples through dense geometry alone can outlast the rest of the launch)
template <bool SEQ, int NQCAP, bool FILTER, int RS = 16, int MINW = 1, bool WIDE = true>
__global__ __launch_bounds__(256, MINW) void k_shadow_nq(DevScene s, DevParams p, const int32_t* __restrict__ hit_id,
                                                   const float* __restrict__ t_in, unsigned long long* __restrict__ shadow_bits,
                                                   unsigned long long* __restrict__ counters, uint32_t l_chunk = 0xffffffffu) {
    __shared__ uint32_t nq_all[4][NQCAP];
    __shared__ uint32_t tq_all[4][LQ_WORDS];
    __shared__ ShadowLds<RS> lds_all[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // p.xcd_rows (scenes far bigger than an L2; the host pads gridDim.y to a multiple of 8): XCD j walks tile rows j, j + 8, ... left to
    // right, as the closest-hit kernels of such scenes do -- neighbouring tiles' shadow rays read the same records in the same L2
    const uint32_t gx = gridDim.x;
    uint32_t bx = blockIdx.x, by = blockIdx.y;
    if (p.xcd_rows) {
        const uint32_t w = blockIdx.y * gx + blockIdx.x, idx = w >> 3;
        by = (idx / gx) * 8u + (w & 7u); bx = idx % gx;
        if (by >= (p.rows + 7u) / 8u) return;
    }
    const uint32_t px = bx * 8 + (wave & 1) * 4 + (lane & 3), r = by * 8 + (wave >> 1) * 4 + ((lane >> 2) & 3);
    int32_t id = -1; float t = 0.f;
    V3 d = mk(0.f, 0.f, p.focal);
    if (lane < NQ_P && pixel_live(p, px, r)) { id = hit_id[(size_t)r * p.W + px]; t = t_in[(size_t)r * p.W + px]; d = primary_dir(p, px, image_row(p, r)); }
    const uint32_t l_begin = l_chunk == 0xffffffffu ? 0u : blockIdx.z * l_chunk;
    shadow_phase<SEQ, NQCAP, FILTER, RS, true, WIDE>(s, p, nq_all[wave], tq_all[wave], lds_all[wave], id, t, d, shadow_bits, counters, bx, by, gx, wave,
                                         l_begin, l_chunk == 0xffffffffu ? 0xffffffffu : l_begin + l_chunk);
}

// One hit pixel: `shadowed(l)` says whether light sample l's shadow ray was blocked.
template <bool INT_SHIN = false, typename SH>
__device__ __forceinline__ void shade_hit_pixel(const DevScene& s, const DevParams& p, const int32_t id, const float t, const uint32_t px, const uint32_t r,
                                                SH shadowed, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8) {
    const V3 o = ray_origin(p);
    const V3 d = primary_dir(p, px, image_row(p, r));
    const Surface f = surface_at(s, id, o, d, t, p.smooth != 0u);
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    add_light_samples<INT_SHIN>(sum, f, o, d, t, p.lights, 0u, p.n_lights, p.shadow_div, shadowed);
    store_pixel(rgb_linear, rgb8, (size_t)r * p.W + px, sum, true, p.reinhard, p.gamma, p.bg, p.exp);
}

// =================================================================================================
// Kernel 1+2a fused (shipped): the wavefront that found its 4x4 tile's closest hits goes straight on to the
// tile's shadow rays -- hit ids, t and the hit object are still in registers, the queues are reused, and
// a frame is two launches (this + shading).  Workgroup = 8x8 pixel tile, 4 waves.
// =================================================================================================
// ROOTS_AGAIN: the round-1 form (every wave re-tests the roots), for A/B
// SHADE: the frame in ONE launch.  The tile's four waves finish at different times and none waits: each leaves its 16 hit ids / t
// in LDS (its shadow masks are there already) and bumps an LDS counter, and the wave that finds the other three done shades the
// tile's 64 pixels, one per lane -- what k_shade_tile does in a second launch from hit ids, t and shadow words re-read from
// memory.  Up to 63 light samples (one group of masks); `shadow_bits` may be null then (nobody reads the words).
// WIDE (the 64 B inner-node records): measured per kernel -- the stand-alone shadow kernel, whose rays cross a
// soup's overlapping boxes hundreds of nodes deep, gains 10 % from it; the fused kernel and the closest-hit kernel, whose frames are
// mostly short waves, lose 5 % (16 VGPRs of record per lane instead of 8: spills at six waves per SIMD), so they keep the 32 B records.
// HALF: the workgroup is TWO waves (128 threads) and wave h owns rows 4h .. 4h + 3 of the tile, 32 rays (closest_hit_phase's HALF,
// shadow_phase's P = 32): the same (node, ray) and (triangle, ray) pairs, merged the same way, on half the waves -- a ground-slab wave's
// one node step and one triangle batch fill 64 lanes instead of 32, and a background tile parks one wave at the barrier, not three.
// The tile's root masks wait in the two waves' own shadow masks (rays 32h .. 32h + 31 in half_all[h].shadow.mask[0 .. 31]): wave h alone writes
// that array again, in its shadow phase, after it has read them -- 256 B less -- and a wave's dir[] and best[] lie over the front of its
// ShadowLds (HalfTileLds, with the lifetimes): nine LDS granules a workgroup, fourteen workgroups per CU with the 72 VGPRs of a 7-wave build.
// ONE (with HALF, over tile spans only): the workgroup is ONE wave, a half tile.  Blocks 2b and 2b + 1 of a grid row are the upper and
// lower half of the tile that block b of the two-wave form owns, so the grid is twice as wide and the span table still counts tiles.  No
// tile-wide root pass, no barrier and no root masks: the wave tests the roots of its own 32 rays (closest_hit_phase's OWN_ROOTS) and
// leaves the CU -- with its LDS -- when it is done, whatever the tile's other half is doing.  ONE == 2, the dispatch order that ships (ONE ==
// 1 is kept under variant 32): a tile's halves EIGHT workgroups apart -- blocks 16g .. 16g + 7 are the upper halves of tiles 8g .. 8g + 7,
// the next eight their lower halves -- on a grid row padded to a multiple of sixteen, so that both halves of a tile run on one XCD
// (workgroups are dealt round-robin over the eight) and read their records through the same L2: 39 % of the L2 requests miss instead of
// 44 %, and the headline step is another 1.3 % shorter.
template <bool COUNT, int NQCAP, bool FILTER, int RS, bool XCD_ROWS, bool ROOTS_AGAIN, bool SHADE = false, bool CAM = false, bool WIDE = false, bool ROW_Z = false,
          bool HALF = false, int ONE = 0, bool WHOLE = false>
__device__ __forceinline__ void trace_nq_body(const DevScene& s_given, const DevParams& p_given, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                              float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                              unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                                              unsigned long long* __restrict__ counters_next = nullptr, uint32_t* __restrict__ qcount = nullptr,
                                              const TileSpans* spans = nullptr,      // the frame's tile spans (k_trace_nq_spans, k_trace_nq_half_spans); null: the kernel has none
                                              const uint32_t* __restrict__ box_epoch = nullptr) {      // with spans, a launch captured into a graph: the records' box epoch word (below)
    // Tile spans (the _spans kernels, launched only with a table that is on): the grid is (widest span, live tile rows), and a workgroup
    // beyond its row's span leaves before it touches LDS or a barrier.  The two words this takes -- row0 and the row's span, which is
    // indexed by blockIdx.y itself -- are requested together and waited for once (the empty asm keeps both loads in front of the branch).
    // A launch that is being CAPTURED into a graph (box_epoch non-null) may be replayed after the boxes have changed, with the table of
    // the boxes it was captured with in its arguments.  It keeps the full grid; a workgroup outside the spans leaves only if the records'
    // epoch word -- rewritten in stream order by every upload, pose and refit -- still is the table's, and otherwise does a tile's whole
    // work, as k_shade_tile_spans then shades every tile.  A workgroup inside the spans never reads the word.
    static_assert(!ONE || HALF, "one wave per workgroup is a half tile");
    // WHOLE (with ONE): the frame is whole and in the reference's ray form, at compile time -- the parameters a split frame, a camera matrix
    // and the A/B switches need are constants from here on (whole_frame_params), and the triangle loops of both phases run over pairs
    static_assert(!WHOLE || ONE, "the whole-frame form is the one-wave kernel's");
    decltype(auto) p_own = frame_params<WHOLE>(p_given);      // (WHOLE: a copy, the general frame: the caller's)
    decltype(auto) s_own = frame_scene<WHOLE>(s_given);
    const DevParams& p = p_own; const DevScene& s = s_own;
    uint32_t span_bx = blockIdx.x, span_by = blockIdx.y; bool span_on = false;
    if constexpr (WHOLE) {
        // The general prologue below reads its arguments where it uses them: the frame's width, the epoch pointer, the span words, the row
        // count, the set-up's words, one scalar round trip each in front of the wave's first LDS write.  Here everything between entry and
        // the end of the root pass -- the span words, the frame's extent, the ray's three words, the root table -- is ONE batch: no address
        // depends on a loaded word (the span is indexed by blockIdx.y), and the empty asm keeps all of it in front of the first branch.
        static_assert(ONE == 2, "the whole-frame form has the shipped dispatch order only");
        const uint32_t blk_x = ((blockIdx.x >> 4) << 3) | (blockIdx.x & 7u);
        uint32_t sp = reinterpret_cast<const uint32_t*>(spans->row)[blockIdx.y < TILE_SPAN_ROWS ? blockIdx.y : TILE_SPAN_ROWS - 1u];      // x0 | n << 16
        uint32_t row0 = spans->row0, n_rows = spans->n_rows;
        unsigned long long epoch_at = reinterpret_cast<unsigned long long>(box_epoch);
        asm volatile("" : "+s"(sp), "+s"(row0), "+s"(n_rows), "+s"(epoch_at), "+s"(p_own.W), "+s"(p_own.rows), "+s"(p_own.i0), "+s"(p_own.j0), "+s"(p_own.focal),
                          "+s"(s_own.n_objects), "+s"(s_own.root_nodes), "+s"(s_own.obj_range));
        if (blk_x >= (p.W + 7u) / 8u) return;      // (the padding of a captured launch's whole grid; a span's is beyond the span)
        span_bx = blk_x;
        // (the pointer comes back from the asm without its address space: named again, so that the word stays a scalar load)
        typedef const uint32_t __attribute__((address_space(4))) * EpochWord;
        const EpochWord epoch_word = (EpochWord)epoch_at;
        if (!epoch_word) {
            if (blk_x >= (sp >> 16)) return;
            span_on = true;
            span_by = row0 + blockIdx.y;
            span_bx = (sp & 0xffffu) + blk_x;
        } else {      // a captured launch: the table counts from tile row 0, and is only as good as its epoch
            const bool outside = blockIdx.y >= n_rows || blk_x - (sp & 0xffffu) >= (sp >> 16);
            if (outside && *epoch_word == spans->epoch) return;
        }
    } else
    if constexpr (ONE != 0) {      // the same prologue for two workgroups a tile (stated apart: the other builds keep their code to the byte)
        const uint32_t blk_x = ONE == 2 ? ((blockIdx.x >> 4) << 3) | (blockIdx.x & 7u) : blockIdx.x >> 1;      // the workgroup's tile in its grid row
        if (ONE == 2 && blk_x >= (p.W + 7u) / 8u) return;      // (the padding of a captured launch's whole grid; a span's is beyond the span)
        span_bx = blk_x;
        if (!box_epoch) {
            uint32_t row0 = spans->row0;
            uint32_t sp = reinterpret_cast<const uint32_t*>(spans->row)[blockIdx.y < TILE_SPAN_ROWS ? blockIdx.y : TILE_SPAN_ROWS - 1u];      // x0 | n << 16
            asm volatile("" : "+s"(sp), "+s"(row0));
            if (blk_x >= (sp >> 16)) return;
            span_on = true;
            span_by = row0 + blockIdx.y;
            span_bx = (sp & 0xffffu) + blk_x;
        } else {
            uint32_t sp = reinterpret_cast<const uint32_t*>(spans->row)[blockIdx.y < TILE_SPAN_ROWS ? blockIdx.y : TILE_SPAN_ROWS - 1u];
            uint32_t n_rows = spans->n_rows;
            asm volatile("" : "+s"(sp), "+s"(n_rows));
            const bool outside = blockIdx.y >= n_rows || blk_x - (sp & 0xffffu) >= (sp >> 16);
            if (outside && *box_epoch == spans->epoch) return;
        }
    } else
    if (spans) {
        if (!box_epoch) {
            uint32_t row0 = spans->row0;
            uint32_t sp = reinterpret_cast<const uint32_t*>(spans->row)[blockIdx.y < TILE_SPAN_ROWS ? blockIdx.y : TILE_SPAN_ROWS - 1u];      // x0 | n << 16
            asm volatile("" : "+s"(sp), "+s"(row0));
            if (blockIdx.x >= (sp >> 16)) return;
            span_on = true;
            span_by = row0 + blockIdx.y;
            span_bx = (sp & 0xffffu) + blockIdx.x;
        } else {      // (the host hands a captured launch a table whose rows count from tile row 0: row0 == 0, again no load waits for another)
            uint32_t sp = reinterpret_cast<const uint32_t*>(spans->row)[blockIdx.y < TILE_SPAN_ROWS ? blockIdx.y : TILE_SPAN_ROWS - 1u];
            uint32_t n_rows = spans->n_rows;
            asm volatile("" : "+s"(sp), "+s"(n_rows));
            const bool outside = blockIdx.y >= n_rows || blockIdx.x - (sp & 0xffffu) >= (sp >> 16);
            if (outside && *box_epoch == spans->epoch) return;
        }
    }
    __shared__ uint32_t fin_count;
    __shared__ int32_t fin_id[64];
    __shared__ float fin_t[64];
    if (SHADE) {
        if (threadIdx.x == 0) fin_count = 0u;              // (the barrier in finish_background_tile orders this before the first bump)
        if (counters_next) zero_next_counters(counters_next);
        if (qcount && blockIdx.x == 0 && blockIdx.y == 0) for (uint32_t i = threadIdx.x; i < (uint32_t)QL_COUNTERS; i += 256u) qcount[i * QL_STRIDE] = 0u;
    }
    static_assert(!HALF || (!SHADE && !COUNT), "the half-tile form has no one-launch and no counting build");
    static_assert(!ONE || (!XCD_ROWS && !ROW_Z && !CAM && !ROOTS_AGAIN), "one wave per workgroup: the plain tile order of a frame with spans only");
    constexpr int NW = ONE ? 1 : HALF ? 2 : 4, P = HALF ? 32 : NQ_P;      // waves per workgroup, rays per wave
    __shared__ uint32_t nq_all[NW][NQCAP];
    __shared__ uint32_t tq_all[NW][LQ_WORDS];
    const uint32_t wave = ONE == 2 ? (blockIdx.x >> 3) & 1u : ONE ? blockIdx.x & 1u : threadIdx.x >> 6;      // which part of the tile the wave owns (ONE: the half, from the grid)
    const uint32_t wq = ONE ? 0u : wave;                                 // ... and which of the workgroup's LDS sets
    ShadowLds<RS, P>* L;                                        // this wave's shadow-phase LDS (HALF: inside the wave's HalfTileLds)
    int32_t id; float t; V3 d;
    unsigned long long k0 = 0, k1 = 0; (void)k0; (void)k1;
    SRT_STAMP(k0);
    // Workgroups are dealt round-robin over the 8 XCDs (b and b + 8 share one, each XCD has its own 4 MiB L2).  When the
    // scene's records are far bigger than an L2 (XCD_ROWS; the host pads the grid's y extent to a multiple of 8 rows), every
    // XCD gets whole rows of tiles -- XCD j walks tile rows j, j + 8, ... left to right -- so that neighbouring tiles, which
    // read the same nodes and triangles, hit in the same L2: 1 M-triangle soup -15 %.  For a scene of a few MB the plain
    // order is as good or slightly better (K3: +1 % with the row deal, +2 % with a run-time switch), so it has its own build.
    const uint32_t gx = ONE ? (p.W + 7u) / 8u : span_on ? (p.W + 7u) / 8u : gridDim.x;      // tiles per row of the FRAME (ONE: only whole frames, and the grid counts half tiles): the shadow words and the quadrant list are indexed by tile
    uint32_t bx = span_bx, by = ROW_Z ? blockIdx.z : span_by;      // ROW_Z: a batch launched with the tile row in z and the frame in y
    if (XCD_ROWS) {
        const uint32_t w = blockIdx.y * gx + blockIdx.x, idx = w >> 3;
        by = (idx / gx) * 8u + (w & 7u); bx = idx % gx;
        if (by >= (p.rows + 7u) / 8u) return;
    }
    __shared__ uint32_t root_pass[64];
    const bool roots_done = !COUNT && !ROOTS_AGAIN && s.n_objects <= 32u;              // wave 0 tests every root for the tile's 64 rays first
    unsigned long long ka = 0, kb = 0; (void)ka; (void)kb;
    ShadowLds<RS, P>* lds_tile = nullptr;      // the four waves' shadow-phase LDS, for the wave that shades the tile (SHADE, never HALF)
    if constexpr (HALF) {
        __shared__ HalfTileLds<RS, P> half_all[NW];
        using Shadow = ShadowLds<RS, P>;
        static_assert(sizeof(half_all[0].closest) <= offsetof(Shadow, mask), "dir[] and best[] end at or before the root masks that wait in ShadowLds::mask");
        static_assert(sizeof(HalfTileLds<RS, P>) == sizeof(Shadow) && sizeof(Shadow) % 4 == 0, "the stride between the two waves' masks is counted in words");
        if constexpr (ONE) {
            // a half with no live pixel (the lower one of a last tile row that is cut at or above its middle) has nothing to write: its
            // shadow bits belong to pixels that do not exist.  Every other wave goes straight into the phase, which tests the roots of
            // its own rays (32 objects at most; more keep the queue path) -- a wave none of whose rays passes a root writes its misses
            // through the phase's write-out, and the shadow phase's quick exit leaves its half of the tile's words all-clear
            if (by * 8u + wave * 4u >= p.rows) return;
            SRT_STAMP(ka);
            closest_hit_phase<COUNT, NQCAP, 3, 2, FILTER, CAM, WIDE, true, true, WHOLE>(s, p, nq_all[0], tq_all[0], half_all[0].closest.best, half_all[0].closest.dir,
                                                                           hit_id, t_out, rgb_linear, rgb8, counters, id, t, d, bx, by, gx, wave, nullptr, nullptr, 0,
                                                                           nullptr, roots_done);
        } else {
        if (finish_background_tile<FILTER, CAM>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, bx, by, gx, half_all[0].shadow.mask, sizeof(HalfTileLds<RS, P>) / 4)) return;
        SRT_STAMP(ka);
        closest_hit_phase<COUNT, NQCAP, 3, 2, FILTER, CAM, WIDE, true>(s, p, nq_all[wave], tq_all[wave], half_all[wave].closest.best, half_all[wave].closest.dir,
                                                                 hit_id, t_out, rgb_linear, rgb8, counters, id, t, d, bx, by, gx, wave, nullptr, nullptr, 0,
                                                                 roots_done ? half_all[wave].shadow.mask : nullptr);
        }
        L = &half_all[wq].shadow;
        // `closest` is dead from here and `shadow` (but its mask) not yet written: the phases' accesses to the shared bytes stay on their
        // sides of this fence (no instruction: the LDS keeps a wave's accesses in order) and of the wave barrier below
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    } else {
    __shared__ unsigned long long best_all[NW][P];
    __shared__ float4 dir_all[NW][P];
    __shared__ ShadowLds<RS, P> lds_all[NW];
    if (!COUNT && finish_background_tile<FILTER, CAM>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, bx, by, gx, root_pass)) return;
    SRT_STAMP(ka);
    closest_hit_phase<COUNT, NQCAP, 2, 2, FILTER, CAM, WIDE>(s, p, nq_all[wave], tq_all[wave], best_all[wave], dir_all[wave],
                                                       hit_id, t_out, rgb_linear, rgb8, counters, id, t, d, bx, by, gx, wave, nullptr, nullptr, 0,
                                                       roots_done ? root_pass + wave * 16 : nullptr);
    L = &lds_all[wave]; lds_tile = lds_all;
    }
    __builtin_amdgcn_wave_barrier();
    SRT_STAMP(kb);
    shadow_phase<COUNT, NQCAP, FILTER, RS, true, WIDE, P, WHOLE>(s, p, nq_all[wq], tq_all[wq], *L, id, t, d, shadow_bits, counters, bx, by, gx, wave);
#ifdef SRT_DIAG
    SRT_STAMP(k1); diag_tile_record(rgb_linear, bx, by, gx, k0, k1, ka, kb);
#endif
    if (SHADE) {
        const uint32_t lane = threadIdx.x & 63;
        if (lane < NQ_P) { fin_id[wave * NQ_P + lane] = id; fin_t[wave * NQ_P + lane] = t; }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        uint32_t before = 0;
        if (lane == 0) before = atomicAdd(&fin_count, 1u);
        before = __builtin_amdgcn_readfirstlane(before);
        if (before != 3u) return;                          // a neighbour is still walking: it will shade the tile
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const uint32_t q = lane >> 4, pl = lane & 15u;       // lane -> (quadrant = the wave that traced it, pixel of the quadrant)
        const uint32_t px = bx * 8 + (q & 1u) * 4 + (pl & 3u), r = by * 8 + (q >> 1) * 4 + (pl >> 2);
        const int32_t hid = fin_id[lane];
        if (hid >= 0 && pixel_live(p, px, r)) {
            const uint32_t* mask = lds_tile[q].mask;
            shade_hit_pixel(s, p, hid, fin_t[lane], px, r, [&](uint32_t l) -> bool { return (mask[l] >> pl) & 1u; }, rgb_linear, rgb8);
        }
    }
}

template <bool COUNT, int NQCAP, bool FILTER, int MINW, int RS, bool XCD_ROWS = false, bool ROOTS_AGAIN = false, bool CAM = false, bool WIDE = false>
__global__ __launch_bounds__(256, MINW) void k_trace_nq(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                  float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                  unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters) {
    trace_nq_body<COUNT, NQCAP, FILTER, RS, XCD_ROWS, ROOTS_AGAIN, false, CAM, WIDE>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters);
}
// The half-tile form (trace_nq_body's HALF): workgroups of two waves, 8x4 pixels each.  Same arguments, same grid (one workgroup per 8x8
// tile), same outputs as k_trace_nq; launched with 128 threads.
template <int NQCAP, bool FILTER, int MINW, int RS>
__global__ __launch_bounds__(128, MINW) void k_trace_nq_half(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                       float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                       unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters);
}
// The same two kernels over a frame's tile spans (srt_tile_spans.h): grid (widest span, live tile rows), the table by value behind the
// other arguments.  Kernels of their own, so that a frame without a table runs the kernels above untouched: even one more scalar load in
// front of a wave's first instructions shows in the frame ("Tile spans").
template <int NQCAP, bool FILTER, int MINW, int RS>
__global__ __launch_bounds__(256, MINW) void k_trace_nq_spans(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                        float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                        unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                                                        const uint32_t* __restrict__ box_epoch, const TileSpans spans) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters, nullptr, nullptr, &spans, box_epoch);
}
template <int NQCAP, bool FILTER, int MINW, int RS>
__global__ __launch_bounds__(128, MINW) void k_trace_nq_half_spans(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                             float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                             unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                                                             const uint32_t* __restrict__ box_epoch, const TileSpans spans) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters, nullptr, nullptr, &spans, box_epoch);
}
// The half-tile form built for EIGHT waves per SIMD (64 VGPRs), and its twin over the tile spans.  Kernels of their own, not further
// instantiations of the two templates above, because they carry a target attribute: without packed f32 operations.  The SLP vectoriser
// pairs this body's f32 multiplies and adds into v_pk_mul_f32 / v_pk_add_f32, which need aligned register pairs and a trail of moves to
// form them -- about ten of the 72 VGPRs of the seven-wave build.  At the 64-register bound the paired code spills 26 registers; without
// the pairing the same source needs 64 and no scratch.  The attribute holds for these kernels alone (the compiler flag that switches the
// vectoriser off would change every kernel of the library).  The LDS side: a 384-entry node queue makes a workgroup 10,120 B, eight
// 1,280-byte granules, and sixteen workgroups -- 32 waves -- fill a CU's 128 granules ("Half tiles at eight waves per SIMD").
// No power of two is asked of NQCAP: the capacity checks are <=, and the roots are pushed NQCAP / (2 * rays) objects at a time.
#if defined(__HIP_DEVICE_COMPILE__)
#define SRT_NO_PACKED_F32 __attribute__((target("no-packed-fp32-ops")))
#else
#define SRT_NO_PACKED_F32      // (the host pass knows no such feature and would warn that it ignores the attribute)
#endif
template <int NQCAP, bool FILTER, int RS>
__global__ __launch_bounds__(128, 8) SRT_NO_PACKED_F32
void k_trace_nq_half8(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                      float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                      unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters);
}
template <int NQCAP, bool FILTER, int RS>
__global__ __launch_bounds__(128, 8) SRT_NO_PACKED_F32
void k_trace_nq_half8_spans(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                            float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                            unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                            const uint32_t* __restrict__ box_epoch, const TileSpans spans) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters, nullptr, nullptr, &spans, box_epoch);
}
// The eight-wave build over the tile spans as workgroups of ONE wave (trace_nq_body's ONE): launched with 64 threads on a grid twice as
// wide as the spans' (XCD_PAIRS, shipped: padded to groups of eight tiles, eight upper halves, then their lower halves; else blocks 2b and
// 2b + 1 the two halves of tile b).  A wave of the two-wave form's lower half waits at the launch-time
// barrier while wave 0 tests the tile's roots, and a workgroup's LDS -- sixteen workgroups fill a CU's -- stays taken until its slower
// wave is done; here a wave starts on its own rays at once and its slot and its four LDS granules (5,056 B: thirty-two workgroups a CU)
// are free the moment it ends.  Under the spans nearly every tile that reaches the phases is live, so the price -- the root tests run
// at 32 rays x 2 objects a pass instead of 64 rays a pass -- is paid where the tile-wide pass bought nothing.  There is no twin for frames
// without a table: there two thirds of the tiles are background, and one wave's 64 root tests beat two waves' 32 each.
// XCD_PAIRS: trace_nq_body's ONE == 2, a tile's halves on one XCD (what variant 0 launches; false: variant 32).
template <int NQCAP, bool FILTER, int RS, bool XCD_PAIRS = false>
__global__ __launch_bounds__(64, 8) SRT_NO_PACKED_F32
void k_trace_nq_wave8_spans(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                            float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                            unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                            const uint32_t* __restrict__ box_epoch, const TileSpans spans) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true, XCD_PAIRS ? 2 : 1>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters, nullptr, nullptr, &spans, box_epoch);
}
// The one-wave kernel for a WHOLE frame in the reference's ray form (trace_nq_body's WHOLE) -- what every frame over tile spans is: the same
// arguments, grid and outputs.  k_trace_nq_wave8_spans is the general frame's code: column tiles (three 32-bit divisions, three times
// over), three forms of scanline blocks, the camera matrix's twelve words and the experiment switches, behind wave-uniform branches a
// frame over spans never takes, in a kernel at the SGPR limit that parks 21 scalars in the lanes of a VGPR and reads them back through
// write-out and shadow set-up.  Here they are constants, and the triangle loops of both phases run over pairs of named records instead of
// rotating one into the other (17 moves a test).  Same rays, same tests in the same order: the same bits.
template <int NQCAP, bool FILTER, int RS, bool XCD_PAIRS = false>
__global__ __launch_bounds__(64, 8) SRT_NO_PACKED_F32
void k_trace_nq_whole8_spans(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                             float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                             unsigned long long* __restrict__ shadow_bits, unsigned long long* __restrict__ counters,
                             const uint32_t* __restrict__ box_epoch, const TileSpans spans) {
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, false, true, XCD_PAIRS ? 2 : 1, true>(s, p, hit_id, t_out, rgb_linear, rgb8, shadow_bits, counters, nullptr, nullptr, &spans, box_epoch);
}
// closest hit, shadow rays and shading of a frame in one launch (SHADE)
template <int NQCAP, bool FILTER, int MINW, int RS, bool XCD_ROWS = false>
__global__ __launch_bounds__(256, MINW) void k_trace_shade_nq(DevScene s, DevParams p, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                        float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                        unsigned long long* __restrict__ counters, unsigned long long* __restrict__ counters_next,
                                                        uint32_t* __restrict__ qcount) {
    trace_nq_body<false, NQCAP, FILTER, RS, XCD_ROWS, false, true>(s, p, hit_id, t_out, rgb_linear, rgb8, nullptr, counters, counters_next, qcount);
}

// ---- several frames in ONE launch (srt_render_device_batch): blockIdx.z selects the frame ------------------------------------
// The frames of an orbit are independent renders (own scene, own parameters, own outputs).  A tile on the bunny's silhouette keeps
// its workgroup busy for ~60 us (~80 with the CU fully occupied), and the chip holds 1,536 workgroups of this kernel at a time: a
// launch lasts a whole number of such rounds.  The 1080p frame has ~2,500 heavy tiles (1.6 rounds in 0.125 ms); the eighth of it
// that one of eight GPUs owns has ~310 and still takes 0.072 ms as its own launch, nine eighths launched together take 0.199 ms
// (two rounds) where 0.142 would be their share -- measured with tools/strip_probe.py, whatever the height of the scanline blocks.
// With ALL frames of a step in one grid the rounds are filled.  A frame's arguments are one entry (416 bytes) of a table that
// travels by value with the launch (FrameTab below), read with scalar loads: the index is the frame's grid coordinate.
struct FrameItem {
    DevScene s; DevParams p;
    int32_t* hit_id; float* t_out; float* rgb_linear; uint8_t* rgb8;
    unsigned long long* shadow_bits; unsigned long long* counters; unsigned long long* counters_next; uint32_t* qcount;
    uint32_t* qlist; uint32_t qcap, pad_;      // the frame's quadrant list (8+-sample pipeline)
};
static_assert(sizeof(FrameItem) == sizeof(DevScene) + sizeof(DevParams) + 9 * 8 + 8, "FrameItem has no implicit padding");
// The frames' arguments travel BY VALUE, in the kernel-argument segment (round 3).  Rounds 1-2 kept the table in device memory; a pointer
// that comes out of memory is a GENERIC pointer to the compiler, every access through it a flat_load / flat_store (both wait counters,
// no scalar form), where the same body with its arguments by value reads wave-uniform records with s_load and the rest with
// global_load -- measured on K4 with one whole frame per "batch": k_shadow_pk_batch 1.57 ms against k_shadow_pk 1.10, closest hit 0.257
// against 0.219, shading 0.135 against 0.122.  Pointer members of a by-value kernel argument are global pointers to the compiler
// (also behind a dynamic index), nothing has to be allocated, copied or kept alive for a captured graph.  The segment is ordinary
// memory on this stack (a 26 KB argument was launched and read back on the MI355X; there is no 4 KB ceiling as on other runtimes):
// 36 frames (the reference's orbit) = 15 KB a launch, a batch of more is issued as several launches -- and every launch boundary costs: the 36 share-frames of a
// K3 step at N = 8 in five launches of 8 took 0.81 ms a step, in one launch 0.64.
constexpr uint32_t FRAME_TAB_MAX = 36;
struct FrameTab { FrameItem it[FRAME_TAB_MAX]; };
static_assert(sizeof(FrameTab) <= 16384, "the frame table is copied into the kernel-argument segment at every launch");
// the unfused closest-hit launch of the 8+-sample pipeline over the frames of a batch (k_closest_hit_nq<false, NQCAP, 2, 2, FILTER>)
// ROW_Z: grid (tiles per row, frames, tile rows) instead of (tiles per row, tile rows, frames): workgroups are dispatched x, then y, then
// z, so the SAME tile row of all the batch's frames is in flight together -- frames of one scene read the same records there, where a
// share's consecutive tile rows (64 image rows apart at N = 8) read different ones.  Same box, shares of 8: K4 2.03 -> 1.86 ms per step,
// K3 0.625 -> 0.599, a quarter of K3 1.179 -> 1.128.  (The bench's frames of a step are one picture, which flatters this; the frames of
// an orbit are 10 degrees apart and still look at the same part of the scene in the same rows.)  Shipped as the only order.
template <int NQCAP, bool FILTER, bool ROW_Z = false>
__global__ __launch_bounds__(256, 7) void k_closest_hit_nq_batch(const FrameTab tab) {
    const FrameItem& it = tab.it[ROW_Z ? blockIdx.y : blockIdx.z];
    const uint32_t tile_row = ROW_Z ? blockIdx.z : blockIdx.y;
    __shared__ uint32_t nq_all[4][NQCAP];
    __shared__ uint32_t tq_all[4][LQ_WORDS];
    __shared__ unsigned long long best_all[4][NQ_P];
    __shared__ float4 dir_all[4][NQ_P];
    __shared__ uint32_t root_pass[64];
    const uint32_t wave = threadIdx.x >> 6;
    int32_t id; float t; V3 d;
    const bool roots_done = it.s.n_objects <= 32u;
    if (finish_background_tile<FILTER>(it.s, it.p, it.hit_id, it.t_out, it.rgb_linear, it.rgb8, nullptr, blockIdx.x, tile_row, gridDim.x, root_pass)) return;
    closest_hit_phase<false, NQCAP, 2, 2, FILTER, false, false>(it.s, it.p, nq_all[wave], tq_all[wave], best_all[wave], dir_all[wave],
                                                  it.hit_id, it.t_out, it.rgb_linear, it.rgb8, it.counters, id, t, d, blockIdx.x, tile_row, gridDim.x, wave,
                                                  it.qcount, it.qlist, it.qcap, roots_done ? root_pass + wave * 16 : nullptr);
}

template <int NQCAP, bool FILTER, int MINW, int RS, bool ROW_Z = false>
__global__ __launch_bounds__(256, MINW) void k_trace_nq_batch(const FrameTab tab) {
    const FrameItem& it = tab.it[ROW_Z ? blockIdx.y : blockIdx.z];
    trace_nq_body<false, NQCAP, FILTER, RS, false, false, false, false, false, ROW_Z>(it.s, it.p, it.hit_id, it.t_out, it.rgb_linear, it.rgb8, it.shadow_bits, it.counters);
}

// =================================================================================================
// Kernel 2b: shading, one thread per hit pixel (same tiles).  softShadow:348-401 (texture fetch,
// light-sample loop with in-order f32 sum, /5 for shadowed samples, Reinhard + gamma),
// phongIllumination:144-200, quantiser :447-449, black -> background (:518, drawImage:476-487).
// Pure ALU, no traversal; misses were finished by the closest-hit kernel.
// =================================================================================================
// SPANS: the kernel takes the frame's tile spans (k_shade_tile_spans), and then WRITES hit_id and t of the tiles outside them: HIT and T are
// its plain pointers there, the read-only restrict pointers of every other kernel otherwise
// WHOLE (with SPANS): a whole frame in the reference's ray form at compile time, as trace_nq_body's WHOLE (whole_frame_params)
template <bool INT_SHIN = false, bool SPANS = false, typename HIT = const int32_t* __restrict__, typename T = const float* __restrict__, bool WHOLE = false>
__device__ __forceinline__ void shade_tile_body(const DevScene& s, const DevParams& p_given, HIT hit_id,
                                                T t_in,
                                                const unsigned long long* __restrict__ shadow_bits,
                                                float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                unsigned long long* __restrict__ counters_next, uint32_t* __restrict__ qcount,
                                                unsigned long long* __restrict__ counters, const TileSpans* spans = nullptr,
                                                const uint32_t* __restrict__ box_epoch = nullptr) {
    // Tile spans on and this wave's tile outside them (wave-uniform): the trace launch never started a workgroup for it.  The wave writes
    // what background_test_wave writes for a tile no ray of which passes a root box, reads nothing, and counts as a wave of zero hits below.
    // (The tile's shadow words stay unwritten: they are only ever read for a pixel with a hit.)  Decided first, so that the two dependent
    // scalar loads are under way while the workgroup meets at its barrier.
    static_assert(!WHOLE || SPANS, "the whole-frame form is a frame over tile spans");
    const DevParams& p = frame_params<WHOLE>(p_given);
    bool outside = false;
    if constexpr (SPANS) {
        const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const uint32_t tx = blockIdx.x * 2u + (w & 1u), rel = blockIdx.y * 2u + (w >> 1) - spans->row0;      // rel: the tile row, counted from row0
        outside = rel >= spans->n_rows;
        if (!outside) { const TileSpan sp = spans->row[rel]; outside = tx - sp.x0 >= sp.n; }
        // a captured launch (trace_nq_body): the table is only as good as its epoch -- if the boxes have changed, the trace launch did every tile
        if (outside && box_epoch && *box_epoch != spans->epoch) outside = false;
    }
    __shared__ uint32_t wg_hits, wg_done;
    if (threadIdx.x == 0) { wg_hits = 0u; wg_done = 0u; }
    __syncthreads();
    if (counters_next) zero_next_counters(counters_next);
    // the quadrant list of this frame has been consumed by the shadow kernel before this launch: empty it for the next one
    if (qcount && blockIdx.x == 0 && blockIdx.y == 0) for (uint32_t i = threadIdx.x; i < (uint32_t)QL_COUNTERS; i += 256u) qcount[i * QL_STRIDE] = 0u;      // list lengths + units handed out
#ifdef SRT_DIAG
    rgb_linear = nullptr;       // holds the trace kernel's stamps in the diagnostic build
#endif
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t px, r;
    const bool live = tile_pixel(p, px, r);
    const size_t pix = (size_t)r * p.W + px;
    if constexpr (SPANS) if (outside && live) {
        hit_id[pix] = -1;
        t_in[pix] = __builtin_inff();
        store_miss(rgb_linear, rgb8, pix, p.bg);
    }
    const int32_t id = (SPANS ? live && !outside : live) ? hit_id[pix] : -1;
    const size_t tile_index = (size_t)(blockIdx.y * 2 + (wave >> 1)) * ((p.W + 7) / 8) + blockIdx.x * 2 + (wave & 1);   // 8x8 tile
    // The frame's hit statistic, here, where the launch overlaps the next frame's tracing.  The closest-hit phase used to add one global
    // atomic per 4x4 quadrant with hits (56 k a K3 frame): 4 % of the trace launch; one per 8x8 tile here (14 k) still made this launch
    // 3.5 us longer.  So the workgroup's four tiles are summed in LDS and the wave that arrives last adds the sum (4 k atomics a frame).
    if (counters && !(p.exp & 32u)) {
        const unsigned long long hm = __ballot(id >= 0);
        if (lane == 0) {
            if (hm) atomicAdd(&wg_hits, (uint32_t)__popcll(hm));
            if (atomicAdd(&wg_done, 1u) == 3u) {
                const uint32_t total = atomicAdd(&wg_hits, 0u);
                if (total) atomicAdd(counters + CTR_HIT_BASE + 8 * ((blockIdx.y * gridDim.x + blockIdx.x) & (HIT_SHARDS - 1)), (unsigned long long)total);
            }
        }
    }
    if (id < 0) return;
    const float t = t_in[pix];
    // shadow bits, tile-major (node-queue kernels): per tile and light sample one word, one 16-bit field per 4x4 quadrant (the wave
    // that traced it), bit = y * 4 + x inside the quadrant; pixel-major (packet shadow kernel): per pixel one word per 64 samples
    const uint32_t n_lch = (p.n_lights + 63u) >> 6;
    const unsigned long long* sb = p.shadow_px_major ? shadow_bits + pix * n_lch : shadow_bits + tile_index * p.n_lights;
    const uint32_t sbit = ((((lane >> 5) & 1u) * 2u + ((lane >> 2) & 1u)) << 4) + ((lane >> 3) & 3u) * 4u + (lane & 3u);
    unsigned long long word = 0ull;                        // pixel-major: the pixel's shadow bits of the current 64 samples, loaded once per 64
    const bool px_major = p.shadow_px_major != 0u;
    shade_hit_pixel<INT_SHIN>(s, p, id, t, px, r, [&](uint32_t l) -> bool {
        if (px_major) {
            if ((l & 63u) == 0u) word = sb[l >> 6];
            return (word >> (l & 63u)) & 1ull;
        }
        return (sb[l] >> sbit) & 1ull;
    }, rgb_linear, rgb8);
}

// INT_SHIN: every object of the scene has an integer shininess in [1, 64] (the reference's default is 15): the per-sample pow is the
// square-and-multiply form alone, and the kernel is built for eight waves per SIMD (the general pow's f64 temporaries cost 100 VGPRs)
template <int INT_SHIN>      // (an int: rocprofv3 consumers take "<true" in a kernel's name for a counting build)
__global__ __launch_bounds__(256, INT_SHIN ? 8 : 1) void k_shade_tile(DevScene s, DevParams p, const int32_t* __restrict__ hit_id,
                                                    const float* __restrict__ t_in,
                                                    const unsigned long long* __restrict__ shadow_bits,
                                                    float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                    unsigned long long* __restrict__ counters_next, uint32_t* __restrict__ qcount,
                                                    unsigned long long* __restrict__ counters) {
    shade_tile_body<INT_SHIN != 0>(s, p, hit_id, t_in, shadow_bits, rgb_linear, rgb8, counters_next, qcount, counters);
}
// k_shade_tile behind k_trace_nq_spans / k_trace_nq_half_spans: a wave whose tile lies outside the frame's spans writes the background
template <int INT_SHIN>
__global__ __launch_bounds__(256, INT_SHIN ? 8 : 1) void k_shade_tile_spans(DevScene s, DevParams p, int32_t* hit_id,
                                                          float* t_in,      // (both read AND written: no const, no restrict)
                                                          const unsigned long long* __restrict__ shadow_bits,
                                                          float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                          unsigned long long* __restrict__ counters_next, uint32_t* __restrict__ qcount,
                                                          unsigned long long* __restrict__ counters, const uint32_t* __restrict__ box_epoch,
                                                          const TileSpans spans) {
    shade_tile_body<INT_SHIN != 0, true, int32_t*, float*>(s, p, hit_id, t_in, shadow_bits, rgb_linear, rgb8, counters_next, qcount, counters, &spans, box_epoch);
}
// k_shade_tile_spans behind k_trace_nq_whole8_spans: the same launch with the whole frame's parameters as constants (shade_tile_body's WHOLE)
template <int INT_SHIN>
__global__ __launch_bounds__(256, INT_SHIN ? 8 : 1) void k_shade_tile_whole_spans(DevScene s, DevParams p, int32_t* hit_id,
                                                                float* t_in,
                                                                const unsigned long long* __restrict__ shadow_bits,
                                                                float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                                unsigned long long* __restrict__ counters_next, uint32_t* __restrict__ qcount,
                                                                unsigned long long* __restrict__ counters, const uint32_t* __restrict__ box_epoch,
                                                                const TileSpans spans) {
    shade_tile_body<INT_SHIN != 0, true, int32_t*, float*, true>(s, p, hit_id, t_in, shadow_bits, rgb_linear, rgb8, counters_next, qcount, counters, &spans, box_epoch);
}
template <int INT_SHIN>
__global__ __launch_bounds__(256, INT_SHIN ? 8 : 1) void k_shade_tile_batch(const FrameTab tab) {      // the shading of the frames k_trace_nq_batch traced
    const FrameItem& it = tab.it[blockIdx.z];
    shade_tile_body<INT_SHIN != 0>(it.s, it.p, it.hit_id, it.t_out, it.shadow_bits, it.rgb_linear, it.rgb8, it.counters_next, it.qcount, it.counters);
}

// =================================================================================================
// Supersampling extension (spp = n x n > 1; not in the reference): the sub-frames' pre-tone-map
// sums are added in sub-sample order, divided by spp, then tone-mapped / quantised once.
// =================================================================================================
// The sub-frames write the live pixels only: the padding of a tile deal is left alone here and in k_resolve (include/srt.h:
// "not written"), or the caller's padding would receive whatever the workspace holds.
__device__ __forceinline__ bool resolve_live(const DevParams& p, uint32_t i) {
    return !p.col_block || pixel_live(p, i % p.W, i / p.W);
}
// the records' box epoch word (SceneRecords::d_box_epoch): written in stream order by whatever changes the boxes on the device
__global__ void k_set_box_epoch(uint32_t* __restrict__ word, uint32_t value) { if (threadIdx.x == 0 && blockIdx.x == 0) *word = value; }

__global__ __launch_bounds__(256) void k_accumulate(DevParams p, float* __restrict__ acc, const float* __restrict__ sub, uint32_t n, int first) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && resolve_live(p, i / 3u)) acc[i] = first ? sub[i] : acc[i] + sub[i];
}
__global__ __launch_bounds__(256) void k_resolve(DevParams p, const float* __restrict__ acc, float spp, uint32_t n_pixels,
                                                 float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                 unsigned long long* __restrict__ counters_next) {
    if (blockIdx.x == 0) for (int i = threadIdx.x; i < NCTR; i += 256) counters_next[i] = 0ull;
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels || !resolve_live(p, i)) return;
    const V3 a = mk(acc[(size_t)i * 3] / spp, acc[(size_t)i * 3 + 1] / spp, acc[(size_t)i * 3 + 2] / spp);
    store_pixel(rgb_linear, rgb8, (size_t)i, a, true, p.reinhard, p.gamma, p.bg, p.exp);
}

// =================================================================================================
// f1, the device half of the per-frame rebuild (srt_scene_update_frame): the records of a frame from the transformed points in
// source order, the build's permutation and the node boxes.
// =================================================================================================
// Ray-independent prefix of rayTriangleIntersection:45-51 and calculateTriangleNormal:32-37 -- ONE definition for the host
// (srt_scene_create) and the device (srt_scene_update_frame); both are compiled with -ffp-contract=off and correctly rounded divide /
// sqrt, so the records are the same bits either way.
__host__ __device__ inline DevTri derive_triangle(const float* p) {
    DevTri t;
    const float P1x = p[0] / p[3], P1y = p[1] / p[3], P1z = p[2] / p[3];
    const float P2x = p[4] / p[7], P2y = p[5] / p[7], P2z = p[6] / p[7];
    const float P3x = p[8] / p[11], P3y = p[9] / p[11], P3z = p[10] / p[11];
    t.p1x = P1x; t.p1y = P1y; t.p1z = P1z;
    t.e1x = P2x - P1x; t.e1y = P2y - P1y; t.e1z = P2z - P1z;
    t.e2x = P3x - P1x; t.e2y = P3y - P1y; t.e2z = P3z - P1z;
    const float ax = p[4] - p[0], ay = p[5] - p[1], az = p[6] - p[2];       // raw xyz, no w-divide (:33-34)
    const float bx = p[8] - p[0], by = p[9] - p[1], bz = p[10] - p[2];
    const float cx = ay * bz - by * az, cy = az * bx - bz * ax, cz = ax * by - bx * ay;
    const float s = 1.0f / sqrtf((cx * cx + cy * cy) + cz * cz);
    t.nx = cx * s; t.ny = cy * s; t.nz = cz * s;
    return t;
}
// tvec = o - P1 with o = 0 (:53) and qvec = cross(tvec, e1) (:58, glm::cross) for rays from the origin
__host__ __device__ inline DevTriO derive_triangle_origin(const DevTri& t) {
    DevTriO r;
    r.tx = 0.0f - t.p1x; r.ty = 0.0f - t.p1y; r.tz = 0.0f - t.p1z;
    r.e1x = t.e1x; r.e1y = t.e1y; r.e1z = t.e1z; r.e2x = t.e2x; r.e2y = t.e2y; r.e2z = t.e2z;
    r.qx = r.ty * t.e1z - t.e1y * r.tz;
    r.qy = r.tz * t.e1x - t.e1z * r.tx;
    r.qz = r.tx * t.e1y - t.e1x * r.ty;
    return r;
}

// visit-order triangle g <- source triangle first[obj] + order[g]: records derived, attributes permuted
__global__ __launch_bounds__(256) void k_update_tris(uint32_t n_tris, const int32_t* __restrict__ tri_obj, const int32_t* __restrict__ obj_tri_first,
                                                     const float4* __restrict__ src_points, const uint32_t* __restrict__ order,
                                                     DevTri* __restrict__ tris, DevTriO* __restrict__ tris_o,
                                                     const float* __restrict__ src_tc, float* __restrict__ tri_tc,
                                                     const float* __restrict__ src_nrm, float* __restrict__ tri_nrm,
                                                     const int32_t* __restrict__ src_tex, int32_t* __restrict__ tri_tex) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_tris) return;
    const int32_t ob = tri_obj[g], f0 = obj_tri_first[ob], cnt = obj_tri_first[ob + 1] - f0;
    const uint32_t oi = order[g];
    const size_t src = (size_t)f0 + (oi < (uint32_t)cnt ? oi : (uint32_t)(cnt - 1));      // (an index outside the object -- a caller's error -- must not become an access outside the buffers)
    const float4 a = src_points[3 * src], b = src_points[3 * src + 1], c = src_points[3 * src + 2];
    const float p[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    const DevTri t = derive_triangle(p);
    tris[g] = t;
    tris_o[g] = derive_triangle_origin(t);
    if (tri_tc && src_tc) for (int k = 0; k < 6; k++) tri_tc[(size_t)g * 6 + k] = src_tc[src * 6 + k];
    if (tri_nrm && src_nrm) for (int k = 0; k < 9; k++) tri_nrm[(size_t)g * 9 + k] = src_nrm[src * 9 + k];
    if (tri_tex) tri_tex[g] = src_tex ? src_tex[src] : -1;
}
// node i: its box into the 32 B record (skip / leaf stay), into its parent's 64 B record (the record of inner node i holds its
// CHILDREN's boxes: written by the parent's thread from the box array), and the roots into the contiguous root table
__global__ __launch_bounds__(256) void k_update_nodes(uint32_t n_nodes, const float* __restrict__ box_min, const float* __restrict__ box_max,
                                                      DevNode* __restrict__ nodes, DevWide* __restrict__ wide, const int32_t* __restrict__ widx) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_nodes) return;
    DevNode n = nodes[i];
    n.minx = box_min[3 * (size_t)i]; n.miny = box_min[3 * (size_t)i + 1]; n.minz = box_min[3 * (size_t)i + 2];
    n.maxx = box_max[3 * (size_t)i]; n.maxy = box_max[3 * (size_t)i + 1]; n.maxz = box_max[3 * (size_t)i + 2];
    nodes[i] = n;
    if (n.leaf < 0) {
        const size_t l = (size_t)i + 1, r = (size_t)(~n.leaf);
        DevWide& q = wide[widx[i]];
        q.lminx = box_min[3 * l]; q.lminy = box_min[3 * l + 1]; q.lminz = box_min[3 * l + 2];
        q.lmaxx = box_max[3 * l]; q.lmaxy = box_max[3 * l + 1]; q.lmaxz = box_max[3 * l + 2];
        q.rminx = box_min[3 * r]; q.rminy = box_min[3 * r + 1]; q.rminz = box_min[3 * r + 2];
        q.rmaxx = box_max[3 * r]; q.rmaxy = box_max[3 * r + 1]; q.rmaxz = box_max[3 * r + 2];
    }
}
__global__ void k_update_roots(uint32_t n_objects, const int2* __restrict__ obj_range, const float* __restrict__ box_min, const float* __restrict__ box_max,
                               const DevNode* __restrict__ nodes, DevNode* __restrict__ root_nodes) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_objects) return;
    const int32_t r = obj_range[k].x;
    DevNode n = nodes[r];                  // (skip / leaf: static; the box from the array, whatever k_update_nodes has written so far)
    n.minx = box_min[3 * (size_t)r]; n.miny = box_min[3 * (size_t)r + 1]; n.minz = box_min[3 * (size_t)r + 2];
    n.maxx = box_max[3 * (size_t)r]; n.maxy = box_max[3 * (size_t)r + 1]; n.maxz = box_max[3 * (size_t)r + 2];
    root_nodes[k] = n;
}

// =================================================================================================
// Pose (srt_scene_pose, an extension): one matrix per object, the hierarchy REFITTED on the device -- tree shape and triangle order
// stay, the points move, the boxes are recomputed.  Data goes from one stage to the next at kernel boundaries on the stream, or
// inside ONE workgroup behind __syncthreads(); no workgroup ever waits for another inside a launch (the per-XCD L2s are not coherent).
//   k_pose_tris       one lane per triangle: p' = M[object] * p, both triangle records, the triangle's own box (24 B)
//   k_pose_boxes      one workgroup per bottom subtree (height <= POSE_SUB_HEIGHT): leaf boxes from the triangles' boxes, the climb in LDS
//   k_pose_top        one workgroup per object: the few nodes above the bottom subtrees, height by height
//   k_update_nodes / k_update_roots (above) put the boxes into the 32 B, 64 B and root records; k_pose_scene_box folds the root boxes.
// A box is a chain of compares that keeps the LEFT operand on ties (fold: `if (v < mn) mn = v; if (mx < v) mx = v;`, Object.cpp:205-221;
// combine(a, b): `b < a ? b : a`), which is associative: folding triangles into their own boxes first and combining those in visit
// order, leaf by leaf and then child by child, gives the value of the reference's one fold over the node's triangles.  A NaN coordinate
// never enters a box (both compares are false); a leaf without triangles keeps (+FLT_MAX, -FLT_MAX).
// =================================================================================================
constexpr int POSE_SUB_HEIGHT = 6;                                  // a bottom subtree has at most 2^6 leaves ...
constexpr int POSE_SUB_NODES = (2 << POSE_SUB_HEIGHT) - 1;          // ... and 127 nodes, a contiguous run in pre-order

// glm's mat4 * vec4 (type_mat4x4.inl:562-573) per component: (m0 * x + m1 * y) + (m2 * z + m3 * w); m = 16 floats, column-major
__host__ __device__ inline float4 pose_point(const float* m, const float4 p) {
    float4 r;
    r.x = (m[0] * p.x + m[4] * p.y) + (m[8] * p.z + m[12] * p.w);
    r.y = (m[1] * p.x + m[5] * p.y) + (m[9] * p.z + m[13] * p.w);
    r.z = (m[2] * p.x + m[6] * p.y) + (m[10] * p.z + m[14] * p.w);
    r.w = (m[3] * p.x + m[7] * p.y) + (m[11] * p.z + m[15] * p.w);
    return r;
}
struct PoseBox { float mn[3], mx[3]; };
__device__ __forceinline__ PoseBox pose_box_empty() { PoseBox b; for (int a = 0; a < 3; a++) { b.mn[a] = 3.402823466e+38f; b.mx[a] = -3.402823466e+38f; } return b; }
__device__ __forceinline__ void pose_box_point(PoseBox& b, const float4 p) {      // raw xyz, no w-divide (Object.cpp:205-221)
    const float v[3] = { p.x, p.y, p.z };
    for (int a = 0; a < 3; a++) { if (v[a] < b.mn[a]) b.mn[a] = v[a]; if (b.mx[a] < v[a]) b.mx[a] = v[a]; }
}
__device__ __forceinline__ void pose_box_combine(PoseBox& l, const float* rmn, const float* rmx) {      // l = combine(l, r): l stays on ties
    for (int a = 0; a < 3; a++) { if (rmn[a] < l.mn[a]) l.mn[a] = rmn[a]; if (l.mx[a] < rmx[a]) l.mx[a] = rmx[a]; }
}

__global__ __launch_bounds__(256) void k_pose_tris(uint32_t n_tris, const int32_t* __restrict__ tri_obj, const float* __restrict__ obj_matrix,
                                                   const float4* __restrict__ src_points, DevTri* __restrict__ tris, DevTriO* __restrict__ tris_o,
                                                   float2* __restrict__ tri_box) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_tris) return;
    // triangles are in object order: all lanes of a wave belong to one object except where two objects meet, so the matrix comes
    // through the scalar cache from a wave-uniform address; a wave that straddles objects gathers per lane
    const int32_t ob = tri_obj[g], ob0 = __builtin_amdgcn_readfirstlane(ob);
    float m[16];
    if (__all(ob == ob0)) {
        const float* M = obj_matrix + 16 * (size_t)ob0;
#pragma unroll
        for (int k = 0; k < 16; k++) m[k] = M[k];
    } else {
        const float4* M = (const float4*)(obj_matrix + 16 * (size_t)ob);
#pragma unroll
        for (int c = 0; c < 4; c++) { const float4 q = M[c]; m[4 * c] = q.x; m[4 * c + 1] = q.y; m[4 * c + 2] = q.z; m[4 * c + 3] = q.w; }
    }
    const float4 a = pose_point(m, src_points[3 * (size_t)g]), b = pose_point(m, src_points[3 * (size_t)g + 1]), c = pose_point(m, src_points[3 * (size_t)g + 2]);
    const float p[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    const DevTri t = derive_triangle(p);
    tris[g] = t;
    tris_o[g] = derive_triangle_origin(t);
    PoseBox bx = pose_box_empty();
    pose_box_point(bx, a); pose_box_point(bx, b); pose_box_point(bx, c);
    tri_box[3 * (size_t)g] = make_float2(bx.mn[0], bx.mn[1]); tri_box[3 * (size_t)g + 1] = make_float2(bx.mn[2], bx.mx[0]);
    tri_box[3 * (size_t)g + 2] = make_float2(bx.mx[1], bx.mx[2]);
}

// Refit from device points (srt_scene_refit_device): the front end of the same refit for points the CALLER holds in device memory --
// no matrix, no arithmetic on a point: each triangle's three points are fetched, both records derived as above, its own box folded.
//   INDEXED   point j of triangle g is points[tri_vertex[3 g + j]] (indices validated on the host, once); else points[3 g + j]
//   STRIDE4   a point is xyzw; else xyz with w = 1.0f, read as exactly 12 bytes
//   WIDE      STRIDE4 and a 16-byte aligned buffer: one 16-byte load a point; else 4-byte loads (any float-aligned address)
//   NORMALS   the 36 B normal row too: direct n_tris x 9 (a flat copy), indexed the three gathered n_verts x 3 rows
// Direct points that are not WIDE are a run of 36 (or 48) bytes a lane: read per lane, every one of the 9 loads would touch all 18
// cache lines of the wave's 2304 bytes.  The workgroup instead reads its contiguous 256 x 36 bytes with consecutive lanes on
// consecutive dwords into LDS and each lane takes its 9 floats from there (a stride of 9 dwords: no two lanes of a half-wave on one bank).
template <bool INDEXED, bool STRIDE4, bool WIDE, bool NORMALS>
__global__ __launch_bounds__(256) void k_refit_tris(uint32_t n_tris, const float* __restrict__ points, const uint32_t* __restrict__ tri_vertex,
                                                    const float* __restrict__ normals, DevTri* __restrict__ tris, DevTriO* __restrict__ tris_o,
                                                    float2* __restrict__ tri_box, float* __restrict__ tri_nrm) {
    static_assert(!WIDE || STRIDE4, "16-byte loads are for xyzw points");
    constexpr int PF = STRIDE4 ? 4 : 3;                              // floats a point
    constexpr bool STAGED = !INDEXED && !WIDE;
    __shared__ float s_pts[STAGED ? 256 * 3 * PF : 1];
    const uint32_t g0 = blockIdx.x * 256, g = g0 + threadIdx.x;
    const uint32_t n_here = n_tris - g0 < 256u ? n_tris - g0 : 256u;  // triangles of this workgroup (the grid covers n_tris: g0 < n_tris)
    if (STAGED) {
        const float* src = points + (size_t)g0 * (3 * PF);
#pragma unroll
        for (int k = 0; k < 3 * PF; k++) { const uint32_t i = threadIdx.x + 256u * k; if (i < n_here * (3 * PF)) s_pts[i] = src[i]; }
        __syncthreads();
    }
    if (NORMALS && !INDEXED) {
        const float* src = normals + (size_t)g0 * 9; float* dst = tri_nrm + (size_t)g0 * 9;
#pragma unroll
        for (int k = 0; k < 9; k++) { const uint32_t i = threadIdx.x + 256u * k; if (i < n_here * 9) dst[i] = src[i]; }
    }
    if (g >= n_tris) return;
    float4 a, b, c;
    uint32_t v[3] = { 3 * g, 3 * g + 1, 3 * g + 2 };                 // (n_tris x 3 fits 32 bits: the scene's own arrays are indexed so)
    if (INDEXED) { v[0] = tri_vertex[3 * (size_t)g]; v[1] = tri_vertex[3 * (size_t)g + 1]; v[2] = tri_vertex[3 * (size_t)g + 2]; }
    if (STAGED) {
        const float* q = s_pts + threadIdx.x * (3 * PF);
        a = make_float4(q[0], q[1], q[2], STRIDE4 ? q[3] : 1.0f);
        b = make_float4(q[PF], q[PF + 1], q[PF + 2], STRIDE4 ? q[PF + 3] : 1.0f);
        c = make_float4(q[2 * PF], q[2 * PF + 1], q[2 * PF + 2], STRIDE4 ? q[2 * PF + 3] : 1.0f);
    } else if (WIDE) {
        const float4* q = (const float4*)points;
        a = q[v[0]]; b = q[v[1]]; c = q[v[2]];
    } else {
        const float* qa = points + (size_t)PF * v[0]; const float* qb = points + (size_t)PF * v[1]; const float* qc = points + (size_t)PF * v[2];
        a = make_float4(qa[0], qa[1], qa[2], STRIDE4 ? qa[3] : 1.0f);
        b = make_float4(qb[0], qb[1], qb[2], STRIDE4 ? qb[3] : 1.0f);
        c = make_float4(qc[0], qc[1], qc[2], STRIDE4 ? qc[3] : 1.0f);
    }
    const float p[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    const DevTri t = derive_triangle(p);
    tris[g] = t;
    tris_o[g] = derive_triangle_origin(t);
    PoseBox bx = pose_box_empty();
    pose_box_point(bx, a); pose_box_point(bx, b); pose_box_point(bx, c);
    tri_box[3 * (size_t)g] = make_float2(bx.mn[0], bx.mn[1]); tri_box[3 * (size_t)g + 1] = make_float2(bx.mn[2], bx.mx[0]);
    tri_box[3 * (size_t)g + 2] = make_float2(bx.mx[1], bx.mx[2]);
    if (NORMALS && INDEXED) {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const float* q = normals + 3 * (size_t)v[j];
            tri_nrm[9 * (size_t)g + 3 * j] = q[0]; tri_nrm[9 * (size_t)g + 3 * j + 1] = q[1]; tri_nrm[9 * (size_t)g + 3 * j + 2] = q[2];
        }
    }
}

// Workgroup b owns the bottom subtree rooted at node sub_root[b]: nodes [r, skip[r]), at most POSE_SUB_NODES of them.  `height`: 0 for
// a leaf, 1 + max(children) for an inner node (static, derived on the host from the tree's shape).
__global__ __launch_bounds__(128) void k_pose_boxes(const int32_t* __restrict__ sub_root, const DevNode* __restrict__ nodes, const uint8_t* __restrict__ height,
                                                    const float2* __restrict__ tri_box, float* __restrict__ box_min, float* __restrict__ box_max) {
    __shared__ float s_mn[POSE_SUB_NODES][3], s_mx[POSE_SUB_NODES][3];
    const int32_t r = sub_root[blockIdx.x];
    int32_t n = nodes[r].skip - r;
    if (n > POSE_SUB_NODES) n = POSE_SUB_NODES;                      // (cannot happen for a height <= POSE_SUB_HEIGHT; keeps every LDS index in range)
    const int32_t j = (int32_t)threadIdx.x;                          // 128 lanes >= 127 nodes: one node per lane
    int32_t leaf = 0, h = 0;
    if (j < n) {
        leaf = nodes[r + j].leaf; h = height[r + j];
        if (leaf >= 0) {
            PoseBox bx = pose_box_empty();
            const size_t first = (size_t)(leaf >> LEAF_SHIFT); const int32_t cnt = leaf & LEAF_MAX;
            for (int32_t i = 0; i < cnt; i++) {
                const float2 q0 = tri_box[3 * (first + i)], q1 = tri_box[3 * (first + i) + 1], q2 = tri_box[3 * (first + i) + 2];
                const float mn[3] = { q0.x, q0.y, q1.x }, mx[3] = { q1.y, q2.x, q2.y };
                pose_box_combine(bx, mn, mx);
            }
            for (int a = 0; a < 3; a++) { s_mn[j][a] = bx.mn[a]; s_mx[j][a] = bx.mx[a]; }
        }
    }
    const int32_t H = height[r];
    for (int32_t lv = 1; lv <= H && lv <= POSE_SUB_HEIGHT; lv++) {
        __syncthreads();
        if (j < n && leaf < 0 && h == lv) {
            const int32_t l = j + 1, rr = ~leaf - r;
            if (l < n && rr > l && rr < n) {
                PoseBox bx; for (int a = 0; a < 3; a++) { bx.mn[a] = s_mn[l][a]; bx.mx[a] = s_mx[l][a]; }
                pose_box_combine(bx, s_mn[rr], s_mx[rr]);
                for (int a = 0; a < 3; a++) { s_mn[j][a] = bx.mn[a]; s_mx[j][a] = bx.mx[a]; }
            }
        }
    }
    __syncthreads();
    if (j < n) for (int a = 0; a < 3; a++) { box_min[3 * (size_t)(r + j) + a] = s_mn[j][a]; box_max[3 * (size_t)(r + j) + a] = s_mx[j][a]; }
}

// Workgroup k owns object k's nodes ABOVE the bottom subtrees: top_nodes[top_off[k] .. top_off[k + 1]), sorted by height.  A child is
// either the root of a bottom subtree (its box was written by the launch before this one) or a node this workgroup wrote one height
// earlier, behind a __syncthreads() (which orders the workgroup's global stores and loads as well as its LDS).
__global__ __launch_bounds__(256) void k_pose_top(const int32_t* __restrict__ top_off, const int32_t* __restrict__ top_nodes, const DevNode* __restrict__ nodes,
                                                  const uint8_t* __restrict__ height, float* box_min, float* box_max) {
    const int32_t b = top_off[blockIdx.x], e = top_off[blockIdx.x + 1];
    if (b == e) return;
    const int32_t H = height[top_nodes[e - 1]];                      // the root: the highest node, last in the list
    for (int32_t lv = POSE_SUB_HEIGHT + 1; lv <= H; lv++) {
        for (int32_t i = b + (int32_t)threadIdx.x; i < e; i += 256) {
            const int32_t j = top_nodes[i];
            if (height[j] != lv) continue;
            const size_t l = (size_t)j + 1, r = (size_t)(~nodes[j].leaf);
            PoseBox bx; for (int a = 0; a < 3; a++) { bx.mn[a] = box_min[3 * l + a]; bx.mx[a] = box_max[3 * l + a]; }
            pose_box_combine(bx, box_min + 3 * r, box_max + 3 * r);
            for (int a = 0; a < 3; a++) { box_min[3 * (size_t)j + a] = bx.mn[a]; box_max[3 * (size_t)j + a] = bx.mx[a]; }
        }
        __syncthreads();
    }
}

// The union of the root boxes (what union_of_roots computes on the host, compare for compare, objects in order): one workgroup; lane t
// folds a contiguous run of objects, lane 0 folds the 256 partial boxes in lane order.
__global__ __launch_bounds__(256) void k_pose_scene_box(uint32_t n_objects, const int2* __restrict__ obj_range, const float* __restrict__ box_min,
                                                        const float* __restrict__ box_max, float* __restrict__ scene_box) {
    __shared__ float s_lo[256][3], s_hi[256][3];
    const uint32_t per = (n_objects + 255) / 256, k0 = threadIdx.x * per, k1 = k0 + per < n_objects ? k0 + per : n_objects;
    float lo[3] = { 3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f }, hi[3] = { -3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f };
    for (uint32_t k = k0; k < k1; k++) {
        const size_t r = (size_t)obj_range[k].x;
        for (int a = 0; a < 3; a++) { const float mn = box_min[3 * r + a], mx = box_max[3 * r + a]; if (mn < lo[a]) lo[a] = mn; if (mx > hi[a]) hi[a] = mx; }
    }
    for (int a = 0; a < 3; a++) { s_lo[threadIdx.x][a] = lo[a]; s_hi[threadIdx.x][a] = hi[a]; }
    __syncthreads();
    if (threadIdx.x) return;
    const uint32_t n_part = (n_objects + per - 1) / per;          // lanes that had objects (<= 256); the others hold the start values
    for (uint32_t t = 1; t < n_part; t++) for (int a = 0; a < 3; a++) { if (s_lo[t][a] < lo[a]) lo[a] = s_lo[t][a]; if (s_hi[t][a] > hi[a]) hi[a] = s_hi[t][a]; }
    scene_box[0] = lo[0]; scene_box[1] = lo[1]; scene_box[2] = lo[2]; scene_box[3] = hi[0]; scene_box[4] = hi[1]; scene_box[5] = hi[2]; scene_box[6] = 0.f; scene_box[7] = 0.f;
}

// =================================================================================================
// The chip's VALU issue rate, measured (srt_debug_valu_rate): every wave runs `iters` x 64 v_fma_f32 over 16 independent accumulators
// between two pairs of stamps (s_memtime = shader cycles, s_memrealtime = the constant 100 MHz counter all CUs share) and notes the
// SIMD it ran on.  With several such waves per SIMD the SIMDs issue back to back, so a SIMD's instructions over the cycles between its
// first wave's start and its last wave's end is what ONE SIMD issues per cycle -- the yardstick bench.py's roofline prices VALU work
// against (MI355X_MICROARCH.md: SIMD-32, a wave64 VALU instruction over 2 cycles -> 0.5; measured: 0.45).
// =================================================================================================
// PACKED: the same count of v_pk_fma_f32 (two f32 fused multiply-adds per lane and instruction): do they issue at the rate of v_fma_f32?
template <bool PACKED>
__global__ __launch_bounds__(256) void k_valu_rate(uint32_t iters, float* __restrict__ sink, unsigned long long* __restrict__ stamps) {
    typedef float v2f __attribute__((ext_vector_type(2)));
    float a[16];
#pragma unroll
    for (int k = 0; k < 16; k++) a[k] = (float)(threadIdx.x + k) * 1.0e-3f;
    const float b = 0.99999f, c = 1.0e-7f;
    v2f pa[16]; const v2f pb = { b, b }, pc = { c, c };
#pragma unroll
    for (int k = 0; k < 16; k++) pa[k] = v2f{ a[k], a[k] + 1.0f };
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    for (uint32_t i = 0; i < iters; i++) {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                if (PACKED) asm volatile("v_pk_fma_f32 %0, %0, %1, %2" : "+v"(pa[k]) : "v"(pb), "v"(pc));
                else        asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[k]) : "v"(b), "v"(c));
            }
    }
    if (PACKED) {
#pragma unroll
        for (int k = 0; k < 16; k++) a[k] = pa[k].x + pa[k].y;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    __builtin_amdgcn_s_waitcnt(0xC07F);
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 16; k++) sum += a[k];
    sink[(size_t)blockIdx.x * 256 + threadIdx.x] = sum;
    if ((threadIdx.x & 63) == 0) {      // + where the wave ran: HW_ID (wave / SIMD / CU / SH / SE) and XCC_ID
        unsigned long long* o = stamps + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8;
        o[0] = t0; o[1] = t1; o[2] = r0; o[3] = r1;
        o[4] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
    }
}

// =================================================================================================
// Known-answer kernels: the device leaf functions on caller-supplied vectors (srt_kat_* in the ABI),
// so that the reference's KAT fixtures pin the DEVICE code paths directly.
// =================================================================================================
__global__ void k_kat_ray_aabb(uint32_t n, const float* __restrict__ ray_od, const float* __restrict__ box,
                               uint8_t* __restrict__ exact, uint8_t* __restrict__ branchless,
                               uint8_t* __restrict__ filtered, uint8_t* __restrict__ ambiguous) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = ray_od + 6 * (size_t)i; const float* b = box + 6 * (size_t)i;
    const V3 o = mk(r[0], r[1], r[2]), d = mk(r[3], r[4], r[5]);
    exact[i] = ray_aabb(o, d, b[0], b[1], b[2], b[3], b[4], b[5]) ? 1 : 0;
    branchless[i] = ray_aabb_nb(o, d, b[0], b[1], b[2], b[3], b[4], b[5]) ? 1 : 0;
    bool amb;
    filtered[i] = ray_aabb_filtered(o, ray_rcp(d), b[0], b[1], b[2], b[3], b[4], b[5], amb) ? 1 : 0;
    ambiguous[i] = amb ? 1 : 0;
}
__global__ void k_kat_ray_triangle(uint32_t n, const float* __restrict__ ray_od, const DevTri* __restrict__ tris, float* __restrict__ t) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = ray_od + 6 * (size_t)i; const DevTri q = tris[i];
    t[i] = ray_triangle(mk(r[0], r[1], r[2]), mk(r[3], r[4], r[5]), mk(q.p1x, q.p1y, q.p1z), mk(q.e1x, q.e1y, q.e1z), mk(q.e2x, q.e2y, q.e2z));
}
// the test every primary ray runs: a ray from the origin on the record that carries tvec and qvec
__global__ void k_kat_ray_triangle_origin(uint32_t n, const float* __restrict__ dir, const DevTriO* __restrict__ tris_o, float* __restrict__ t) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* r = dir + 3 * (size_t)i; const DevTriO q = tris_o[i];
    t[i] = ray_triangle_origin(mk(r[0], r[1], r[2]), mk(q.tx, q.ty, q.tz), mk(q.e1x, q.e1y, q.e1z), mk(q.e2x, q.e2y, q.e2z), mk(q.qx, q.qy, q.qz));
}
// in15: the triangle's points (12) and the point whose coordinates are asked for (3)
__global__ void k_kat_barycentric(uint32_t n, const float* __restrict__ in15, const DevTri* __restrict__ tris, float* __restrict__ out3) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in15 + 15 * (size_t)i; const DevTri tr = tris[i];
    const V3 b = barycentric(mk(tr.p1x, tr.p1y, tr.p1z), mk(tr.e1x, tr.e1y, tr.e1z), mk(tr.e2x, tr.e2y, tr.e2z), mk(q[12], q[13], q[14]));
    out3[i * 3] = b.x; out3[i * 3 + 1] = b.y; out3[i * 3 + 2] = b.z;
}
// in: ray_od(6) normal-from-DevTri(3 via tris) light(3) color(3) props(3) t(1)
__global__ void k_kat_phong(uint32_t n, const float* __restrict__ in, const DevTri* __restrict__ tris, float* __restrict__ rgb) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in + 28 * (size_t)i; const DevTri tr = tris[i];
    const V3 c = phong(mk(tr.nx, tr.ny, tr.nz), mk(q[0], q[1], q[2]), mk(q[3], q[4], q[5]), mk(q[18], q[19], q[20]),
                       mk(q[21], q[22], q[23]), q[24], q[25], q[26], q[27]);
    rgb[i * 3] = c.x; rgb[i * 3 + 1] = c.y; rgb[i * 3 + 2] = c.z;
}
__global__ void k_kat_interp_normal(uint32_t n, const float* __restrict__ in12, float* __restrict__ out3) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* q = in12 + 12 * (size_t)i;
    const V3 r = normalize3(mk((q[9] * q[0] + q[10] * q[3]) + q[11] * q[6], (q[9] * q[1] + q[10] * q[4]) + q[11] * q[7],
                               (q[9] * q[2] + q[10] * q[5]) + q[11] * q[8]));
    out3[i * 3] = r.x; out3[i * 3 + 1] = r.y; out3[i * 3 + 2] = r.z;
}
// pow_like_host against the f64 library pow on the same inputs: out[0] = fast path result, out[1] = (float)pow(double)
__global__ void k_kat_pow(uint32_t n, const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ fast, float* __restrict__ lib) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fast[i] = pow_like_host(x[i], y[i]);
    lib[i] = (float)pow((double)x[i], (double)y[i]);
}
__global__ void k_kat_tonemap(uint32_t n, const float* __restrict__ lin, float reinhard, float gamma, float* __restrict__ tone, int32_t* __restrict__ q) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 3 * n) return;
    const float c = tone1(lin[i], reinhard, gamma);
    tone[i] = c; q[i] = quant1(c);
}
// The tone map's filter (quant_tone, srt_device.h) beside what it replaces.  Values go through quant_tone three at a time, as store_pixel's
// do (the last triple repeats the last value): q = what store_pixel writes, q_filter = the filter's candidate (-1 where it decided
// nothing), decided = 1 where the filter alone decided.
__global__ void k_kat_tone_filter(uint32_t n, const float* __restrict__ lin, float reinhard, float gamma, int32_t* __restrict__ q, int32_t* __restrict__ q_filter,
                                  uint8_t* __restrict__ decided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (3ull * i >= n) return;
    const uint32_t i0 = 3u * i, i1 = i0 + 1u < n ? i0 + 1u : n - 1u, i2 = i0 + 2u < n ? i0 + 2u : n - 1u;
    const float c[3] = {lin[i0], lin[i1], lin[i2]};
    const uint32_t at[3] = {i0, i1, i2};
    int e[3];
    quant_tone<3>(c, reinhard, gamma, false, e);
    const ToneFilter f = tone_filter(reinhard, gamma);
    for (int k = 0; k < 3; k++) {
        int qf; float cand, rel;
        const bool dec = tone_candidate(f, c[k], reinhard, gamma, qf, cand, rel);
        q[at[k]] = e[k]; q_filter[at[k]] = dec ? qf : -1; decided[at[k]] = dec ? 1 : 0;
    }
}
// Every float whose bit pattern is first + [0, count) through both forms, reduced here: out[0] values, [1] undecided by the filter,
// [2] decided and different from quant1(tone1()), [3] quant_tone's result (after the fallback) different from it, [4] the largest
// |cand / s - 1| over decided values, s = tone1() * 255 in f32 as quant1 forms it, [5] the largest of that deviation over the shipped
// margin rel (a double's bits each: non-negative doubles order as their bits do).  [4] and [5] leave out s < 1e-30: both forms are far
// below 1 there, and beneath 3e-36 the tone itself is a subnormal whose rounding is no longer relative.  One atomic per workgroup and
// figure (2,048 workgroups at most).
__global__ __launch_bounds__(256) void k_kat_tone_sweep(uint32_t first, unsigned long long count, float reinhard, float gamma, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4][6];
    const ToneFilter f = tone_filter(reinhard, gamma);
    unsigned long long v[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    double dev = 0.0, ratio = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < count; i += stride) {
        const float c[1] = {__uint_as_float(first + (uint32_t)i)};
        const float tone = tone1(c[0], reinhard, gamma), s = tone * 255.0f;
        const int exact = quant1(tone);
        int qf, e[1]; float cand, rel;
        const bool dec = tone_candidate(f, c[0], reinhard, gamma, qf, cand, rel);
        quant_tone<1>(c, reinhard, gamma, false, e);
        v[0]++; v[1] += dec ? 0u : 1u; v[2] += (dec && qf != exact) ? 1u : 0u; v[3] += e[0] != exact ? 1u : 0u;
        if (dec && s >= 1.0e-30f) {
            const double dv = __builtin_fabs((double)cand / (double)s - 1.0), rt = dv / (double)rel;
            dev = dv > dev ? dv : dev; ratio = rt > ratio ? rt : ratio;
        }
    }
    v[4] = (unsigned long long)__double_as_longlong(dev); v[5] = (unsigned long long)__double_as_longlong(ratio);
    for (int k = 0; k < 6; k++)
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(v[k], off, 64);
            v[k] = k < 4 ? v[k] + o : (o > v[k] ? o : v[k]);
        }
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) for (int k = 0; k < 6; k++) part[wave][k] = v[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        unsigned long long a = part[0][k];
        for (int w = 1; w < 4; w++) a = k < 4 ? a + part[w][k] : (part[w][k] > a ? part[w][k] : a);
        if (k < 4) atomicAdd(out + k, a); else atomicMax(out + k, a);
    }
}
