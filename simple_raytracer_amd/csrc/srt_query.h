// srt_query.h -- ray queries (include/srt.h, RAY QUERIES): closest hit and occlusion for rays the CALLER supplies.  Included by
// srt_hip.hip only, after srt_kernels.h.
//
// The unit of work is a ray, not a pixel of a tile: lane i of the grid owns ray i (origin xyz, direction xyz, 24 B), whatever its
// neighbours are.  Nothing here may assume a common origin, so there is no tile, no root mask and no union-box shortcut; what is kept
// of the render kernels is the walk itself -- the stackless pre-order walk over the 32 B DevNode records with skip links, the slab
// test through slab_pass (reciprocal filter, exact fallback) -- and, for the closest hit, the per-wave triangle queue of
// k_closest_hit_q.  The candidate set of a ray is the reference's (every leaf whose ancestors all pass the literal slab test, no t
// pruning) and the merge is the order-independent (t, id) minimum, so a ray's result depends on the ray alone, never on its place in
// the batch.  RANGE builds of the two kernels bound t per ray (load_range below); they visit the same nodes and test the same triangles.
#pragma once
#include "srt_kernels.h"

// A ray as lane `i` reads it.  wide: the array is 8-byte aligned, so the 24 B are three dwordx2 loads (a wave reads its 1.5 KB
// contiguously either way); a caller's pointer that is only float-aligned takes six dword loads.
__device__ __forceinline__ void load_ray(const float* __restrict__ rays, size_t i, bool wide, V3& o, V3& d) {
    if (wide) {
        const float2* r2 = reinterpret_cast<const float2*>(rays) + 3 * i;
        const float2 a = r2[0], b = r2[1], c = r2[2];
        o = mk(a.x, a.y, b.x); d = mk(b.y, c.x, c.y);
    } else {
        const float* r = rays + 6 * i;
        o = mk(r[0], r[1], r[2]); d = mk(r[3], r[4], r[5]);
    }
}

// The t interval of ray `i` (include/srt.h, "A t interval per ray"): t_range = n x 2 floats (t_min, t_max), read like the rays -- one
// dwordx2 load where the array is 8-byte aligned, two dword loads where it is only float-aligned.  A candidate is IN RANGE iff
// !(t < t_min) && !(t > t_max): the interval is closed, a NaN bound bounds nothing, a NaN t is in range.  The interval never prunes the
// walk: the candidate set and the nodes visited are those of the unbounded query.
struct QueryRange { const float* t; uint32_t wide; };
__device__ __forceinline__ void load_range(const QueryRange tr, size_t i, float& t_min, float& t_max) {
    if (tr.wide) {
        const float2 a = reinterpret_cast<const float2*>(tr.t)[i];
        t_min = a.x; t_max = a.y;
    } else {
        t_min = tr.t[2 * i]; t_max = tr.t[2 * i + 1];
    }
}

// =================================================================================================
// The statements AROUND the walk, each stated once: every query kernel below is these pieces in its own order, with its own walk
// (query_walk, any_hit_range) or phase 2 between them.
// Why they fill objects the caller declares, and take no __restrict__: DESIGN.md s5, "One statement of the code around the walk".
// =================================================================================================
// A lane's place in a 1-D launch of 256 threads -- its number in its wave, the wave's number in the workgroup -- and the contiguous
// deal of rays to waves: the wave's first ray, and ray base + lane as the launch's own thread number for a kernel that needs no base.
__device__ __forceinline__ uint32_t wave_lane() { return threadIdx.x & 63; }
__device__ __forceinline__ uint32_t wave_index() { return threadIdx.x >> 6; }
__device__ __forceinline__ size_t wave_base(const uint32_t wave) { return (size_t)blockIdx.x * 256 + wave * 64; }
__device__ __forceinline__ size_t lane_ray() { return (size_t)blockIdx.x * 256 + threadIdx.x; }
// The deal of the shaded calls (QueryShade::spread, QueryAo::spread): without spread the contiguous one; with it a wave owns 8 groups
// of 8 consecutive rays, the groups a 64th of the batch apart.  The shadow walks of a batch are few long ones among many short ones, and
// the long ones sit together (the pixels in one object's shadow); a wave of 64 such neighbours walks them one round after the other
// while the rest of the machine has left.  Groups of 8 neighbours keep most of phase 1's coherence and put a region's hits into 8 times
// as many waves.  Called with any lane of the wave: the transposed row stores need the rays of other lanes.
struct RayDeal {
    uint32_t spread;
    size_t n_waves, wv;
    __device__ __forceinline__ size_t operator()(const uint32_t l) const { return spread ? ((size_t)(l >> 3) * n_waves + wv) * 8 + (l & 7u) : wv * 64 + l; }
};
__device__ __forceinline__ RayDeal ray_deal(const uint32_t spread, const uint32_t wave) {
    return RayDeal{ spread, (size_t)gridDim.x * 4, (size_t)blockIdx.x * 4 + wave };
}

// What a lane loads before its walk: its ray, its t interval and its visibility mask.  A lane without a ray gets a ray that is never
// walked.  Two conventions for the interval: query_ray<RANGE> is the compile-time one -- the builds without RANGE load nothing and carry
// (0, 0), which nothing reads; query_ray_opt is the run-time one of the kernels that always run the RANGE walk -- a NULL tr.t runs as
// (NaN, NaN), which bounds nothing.  ray_mask: the per-ray masks of the masked calls (NULL: all ones).
struct QueryRay { V3 o, d; float t_min, t_max; uint32_t m; };
template <bool OPT, bool RANGE>
__device__ __forceinline__ void load_query_ray(QueryRay& r, const float* rays, const uint32_t wide, const QueryRange tr, const size_t ri, const bool live,
                                               const uint32_t* ray_mask) {
    r.o = mk(0.0f, 0.0f, 0.0f); r.d = mk(0.0f, 0.0f, 1.0f);
    r.t_min = OPT ? __builtin_nanf("") : 0.0f; r.t_max = r.t_min;
    r.m = 0xFFFFFFFFu;
    if (live) load_ray(rays, ri, wide != 0, r.o, r.d);
    if ((OPT ? tr.t != nullptr : RANGE) && live) load_range(tr, ri, r.t_min, r.t_max);
    if (ray_mask && live) r.m = ray_mask[ri];
}
template <bool RANGE>
__device__ __forceinline__ void query_ray(QueryRay& r, const float* rays, const uint32_t wide, const QueryRange tr, const size_t ri, const bool live) {
    load_query_ray<false, RANGE>(r, rays, wide, tr, ri, live, nullptr);
}
__device__ __forceinline__ void query_ray_opt(QueryRay& r, const float* rays, const uint32_t wide, const QueryRange tr, const size_t ri, const bool live,
                                              const uint32_t* ray_mask = nullptr) {
    load_query_ray<true, true>(r, rays, wide, tr, ri, live, ray_mask);
}

// A merged key (hit_key below; ~0: a miss) as the lane that owns the ray reads it.  winner_of: whether the ray hit, and the triangle.
// winner_at: also the winner's t with its own bits (incl. the sign of a zero, which the key does not hold) -- the walk's function on the
// walk's inputs, the lane's own ray, so the walk's value and hence in range -- and, BARY, calculateBarycentricCoords at that hit point.
struct Winner { bool is_hit; int32_t id; };
__device__ __forceinline__ Winner winner_of(const unsigned long long key) {
    const bool is_hit = key != ~0ull;
    return Winner{ is_hit, is_hit ? (int32_t)(uint32_t)key : -1 };
}
struct WinnerAt { int32_t id; float t; V3 bc; };      // (a miss: -1, +inf, zeros)
template <bool BARY>
__device__ __forceinline__ void winner_at(WinnerAt& w, const float4* tris4, const unsigned long long key, const V3 o, const V3 d) {
    w.id = -1;
    w.t = __builtin_inff();
    w.bc = mk(0.0f, 0.0f, 0.0f);
    if (key != ~0ull) {
        w.id = (int32_t)(uint32_t)key;
        V3 p1, e1, e2;
        load_tri_edges(tris4, (size_t)w.id, p1, e1, e2);
        w.t = ray_triangle(o, d, p1, e1, e2);
        if (BARY) w.bc = barycentric(p1, e1, e2, o + d * w.t);
    }
}

// The hit_id / t row of a ray; either output may be NULL.  Called by the lanes that have a row.
__device__ __forceinline__ void store_hit(int32_t* hit_id, float* t_out, const size_t at, const int32_t id, const float t) {
    if (hit_id) hit_id[at] = id;
    if (t_out) t_out[at] = t;
}

// The counters a kernel leaves with (COUNT), laid out like a render's: [1] / [2] node / triangle tests of the closest-hit walks, and,
// for the kernels with a phase 2, [3] / [4] those of its occlusion walks.  (The hit rays go to their shard through count_hits.)
template <bool COUNT>
__device__ __forceinline__ void count_walks(unsigned long long* counters, const unsigned long long& n_node, const unsigned long long& n_tri) {
    if (COUNT) { wave_add(counters + 1, n_node); wave_add(counters + 2, n_tri); }
}
template <bool COUNT>
__device__ __forceinline__ void count_walks(unsigned long long* counters, const unsigned long long& n_node, const unsigned long long& n_tri,
                                            const unsigned long long& n_node_s, const unsigned long long& n_tri_s) {
    if (COUNT) { wave_add(counters + 1, n_node); wave_add(counters + 2, n_tri); wave_add(counters + 3, n_node_s); wave_add(counters + 4, n_tri_s); }
}

// The surface of a lane without a hit: black, no normal, no material.  sh = 1 where it goes on into shading (it shades to nothing),
// sh = 0 where it is a miss row of the surface outputs.
__device__ __forceinline__ void no_surface(Surface& f, const float sh) {
    f.color = mk(0.0f, 0.0f, 0.0f); f.nrm = f.color; f.ka = 0.0f; f.ks = 0.0f; f.sh = sh;
}

// =================================================================================================
// Closest hit of caller-supplied rays: the oracle's closest_in_tree over the objects in order, with the ray's own origin.
// One ray per lane.  The lanes of a wave walk on their own (the rays may be unrelated); a lane whose ray passes a leaf's box pushes
// (triangle, lane) pairs into the wave's LDS queue, and whenever 64 pairs are queued the whole wave runs the general Moller-Trumbore
// test on them, one pair per lane, with the OWNING lane's ray (kept in LDS), and merges with a 64-bit LDS atomicMin on
// (t bits << 32 | triangle id) -- k_closest_hit_q's scheme, +-0 handling included.
// counters: null, or a set laid out like a render's -- [1] / [2] node / triangle tests (COUNT), [8 + 8 * shard] hit rays.
// =================================================================================================
// The walk and the merge for the 64 rays of one wave, shared by k_query_closest and k_query_shade: on return best[lane] holds the
// lane's minimum of (t bits << 32 | triangle id), ~0 on a miss.  q (QCAP words), best (64 words) and wray (the wave's rays) are the
// wave's own LDS.
// RANGE: the lane's t interval goes into two more rows of wray (8 rows instead of 6) -- a queued pair is tested by whichever lane draws
// it, so the interval has to live where the ray lives -- and a result joins the merge only if it is in range of its OWNER's interval.
// What is kept of the qualifying candidates is the MERGE's business (MergeClosest here, MergeMulti below): init(lane) before the walk by
// the owning lane, offer(owner, triangle, t) by whichever lane tested the pair -- so a merge is atomic in LDS and independent of order.
__device__ __forceinline__ unsigned long long hit_key(const float t, const uint32_t tri) {
    const uint32_t tb = (t == 0.0f) ? 0u : __float_as_uint(t);     // -0.0 ties with +0.0
    return ((unsigned long long)tb << 32) | tri;
}
struct MergeClosest {
    unsigned long long* best;     // 64 words: the lane's minimum of (t bits << 32 | triangle id), ~0 on a miss
    __device__ __forceinline__ void init(const uint32_t lane) const { best[lane] = ~0ull; }
    __device__ __forceinline__ void offer(const uint32_t src, const uint32_t tri, const float t) const { atomicMin(&best[src], hit_key(t, tri)); }
};

// The visibility masks of a masked call (include/srt.h, "Visibility masks"), their own kernel argument: the scene's table (NULL = all
// ones), the per-ray masks of the closest-hit and occlusion queries (NULL = all ones), and the three masks per ray KIND of the shaded calls.
struct QueryMask { const uint32_t* obj; const uint32_t* ray; uint32_t primary, bounce, shadow; };
// The object cursor of a masked walk: `root` is the index of the next object's root and `k` that object's number.  Called with the node
// the lane is about to go to: while that node is a root, the cursor moves on, and a hidden object -- (obj_mask[k] & m) == 0 -- moves
// `next` to the end of its range, which is the next root.  One 4-byte mask load and one 8-byte range load, independent of each other, per
// object per ray; no node record of a hidden object is read.  An object without nodes is passed over either way.
struct ObjCursor { int32_t root; uint32_t k; };
__device__ __forceinline__ int32_t skip_hidden(const DevScene& s, const uint32_t* __restrict__ obj_mask, const uint32_t m, ObjCursor& c, int32_t next) {
    while (next == c.root && c.k < s.n_objects) {
        const int2 r = s.obj_range[c.k];
        const uint32_t om = obj_mask ? obj_mask[c.k] : 0xFFFFFFFFu;
        c.k++;
        c.root = r.y;
        if (!(om & m)) next = r.y;
    }
    return next;
}

// The node test of a walk: the ray's slab test, or the policy's own (query_walk below).
template <bool RAY, typename Tests>
__device__ __forceinline__ bool node_pass(const Tests& ts, const V3 o, const V3 d, const RayRcp rc, const float4 a, const float4 b) {
    if constexpr (RAY) return slab_pass<true>(o, d, rc, a.x, a.y, a.z, a.w, b.x, b.y);
    else return ts.node(a, b);
}

// MASK: only the objects k with (obj_mask[k] & ray_m) != 0 are walked (skip_hidden); the builds without it never read the two arguments.
// TESTS: what is walked.  The queue, the prefix sum, the leaf slices, the flush and the tail are stated here once; the two leaf functions
// and the owner's LDS rows are a policy.  WalkRay, the default, is the ray's: 6 rows (o, d), 8 with RANGE, slab_pass and ray_triangle --
// the statements this function always had, left where they were, so that every ray kernel compiles to the code it compiled to before the
// policy existed (profiles/point_query_kernels.txt).  Any other policy (WalkPoint, at the end of this file) brings
//     init(rows, lane)                          the owning lane's operands into the wave's rows (`wray`)
//     node(a, b)                                the lane's own test of a node record's box
//     leaf(rows, src, p1, e1, e2, tri, mg)      the triangle test with the operands of owner `src`; a qualifying result is offered to mg
// and is walked with o, d, t_min and t_max unread.
// walk_shrinks<Tests>: node() of this policy may give another answer for the same node later in the walk (WalkNearest); no other policy does.
struct WalkRay {};
template <typename Tests> struct walk_shrinks : std::false_type {};
template <bool COUNT, bool RANGE, typename Merge, bool MASK = false, typename Tests = WalkRay>
__device__ __forceinline__ void query_walk(const DevScene& s, const bool live, const V3 o, const V3 d, const uint32_t lane, uint32_t* q,
                                           const Merge mg, float (*wray)[64], unsigned long long& n_node, unsigned long long& n_tri,
                                           const float t_min = 0.0f, const float t_max = 0.0f, const uint32_t* __restrict__ obj_mask = nullptr,
                                           const uint32_t ray_m = 0u, const Tests ts = Tests{}) {
    constexpr bool RAY = std::is_same<Tests, WalkRay>::value;
    mg.init(lane);
    if constexpr (RAY) {
        wray[0][lane] = o.x; wray[1][lane] = o.y; wray[2][lane] = o.z;
        wray[3][lane] = d.x; wray[4][lane] = d.y; wray[5][lane] = d.z;
        if (RANGE) { wray[6][lane] = t_min; wray[7][lane] = t_max; }
    } else ts.init(wray, lane);
    const RayRcp rc = ray_rcp(o, d);
    const float4* nodes4 = reinterpret_cast<const float4*>(s.nodes);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    const int32_t n = (int32_t)s.n_nodes;
    int32_t i = live ? 0 : n;
    ObjCursor cur = { 0, 0u };
    if (MASK && i < n) i = skip_hidden(s, obj_mask, ray_m, cur, i);      // (the first object may be hidden: node 0 is not tested then)
    int32_t leaf_off = 0;
    uint32_t qn = 0;                                    // wave-uniform queue length
    float4 na = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nb = na;      // node i (valid while i < n)
    if (MASK) { if (i < n) { na = nodes4[2 * (size_t)i]; nb = nodes4[2 * (size_t)i + 1]; } }
    else if (i < n) { na = nodes4[0]; nb = nodes4[1]; } // (a lane without a ray, or a scene without nodes, reads no record)
    __builtin_amdgcn_wave_barrier();
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
                // (a leaf pushed in slices is tested again per slice: same ray, same box, same answer)
                if (node_pass<RAY>(ts, o, d, rc, a, b)) {
                    next = i + 1;
                    if (leaf >= 0) {
                        const int32_t c = (leaf & LEAF_MAX) - leaf_off;
                        first = (uint32_t)((leaf >> LEAF_SHIFT) + leaf_off);
                        cnt = (uint32_t)(c < PUSH_MAX ? c : PUSH_MAX);
                        if (c > PUSH_MAX) { leaf_off += PUSH_MAX; stay = true; } else leaf_off = 0;
                    }
                } else {
                    next = skip;
                    if constexpr (walk_shrinks<Tests>::value) leaf_off = 0;      // (a bound that moved can fail a LATER slice of a leaf: the rest is not taken)
                }
                if (!stay) {
                    if (MASK) next = skip_hidden(s, obj_mask, ray_m, cur, next);      // (a slice of a leaf stays: the cursor does not move)
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
                if constexpr (RAY) {
                    const V3 os = mk(wray[0][src], wray[1][src], wray[2][src]), ds = mk(wray[3][src], wray[4][src], wray[5][src]);
                    float lo = 0.0f, hi = 0.0f;
                    if (RANGE) { lo = wray[6][src]; hi = wray[7][src]; }
                    V3 p1, e1, e2;
                    load_tri_edges(tris4, tri, p1, e1, e2);
                    if (COUNT) n_tri++;
                    const float t = ray_triangle(os, ds, p1, e1, e2);
                    // candidate iff t != -inf && t < +inf (the initial distanceComparison, :408); NaN fails '<'
                    if (t != SRT_NEG_INF && t < __builtin_inff() && (!RANGE || (!(t < lo) && !(t > hi)))) mg.offer(src, tri, t);
                } else {
                    V3 p1, e1, e2;
                    load_tri_edges(tris4, tri, p1, e1, e2);
                    if (COUNT) n_tri++;
                    ts.leaf(wray, src, p1, e1, e2, tri, mg);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// The body of k_query_closest and k_query_closest_masked, as query_path_rays is the path kernels'.
// RANGE: the closest hit among the candidates in range of the ray's own interval tr (the winner is in range, so its recomputed t is too).
// MASK (srt_trace_rays_masked): ray i is walked with qm.ray[i] (a NULL array: all ones) against qm.obj; a mask that selects nothing leaves
// the lane without a node to test, so it is a miss.  The MASK build is a RANGE build under the run-time convention: a NULL interval runs
// as (NaN, NaN), which bounds nothing, as in k_query_multi.  counters: of the walk as it runs -- a hidden object's root is neither tested
// nor counted.
template <bool COUNT, bool BARY, bool RANGE, bool MASK>
__device__ __forceinline__ void query_closest_rays(const DevScene& s, const uint32_t n_rays, const float* __restrict__ rays, const uint32_t wide,
                                                   int32_t* __restrict__ hit_id, float* __restrict__ t_out, float* __restrict__ bary,
                                                   unsigned long long* __restrict__ counters, const QueryRange tr, const QueryMask qm = QueryMask{}) {
    static_assert(RANGE || !MASK, "the masked walk is the RANGE walk");
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][RANGE ? 8 : 6][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    const size_t ri = lane_ray();
    const bool live = ri < (size_t)n_rays;
    unsigned long long n_node = 0, n_tri = 0;
    QueryRay r;
    if (MASK) query_ray_opt(r, rays, wide, tr, ri, live, qm.ray);
    else query_ray<RANGE>(r, rays, wide, tr, ri, live);
    const V3 o = r.o, d = r.d;
    query_walk<COUNT, RANGE, MergeClosest, MASK>(s, live, o, d, lane, q_all[wave], MergeClosest{ best }, ray_all[wave], n_node, n_tri, r.t_min, r.t_max, qm.obj, r.m);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    WinnerAt h;
    winner_at<BARY>(h, tris4, live ? best[lane] : ~0ull, o, d);
    if (live) {
        store_hit(hit_id, t_out, ri, h.id, h.t);
        if (BARY) { bary[ri * 3] = h.bc.x; bary[ri * 3 + 1] = h.bc.y; bary[ri * 3 + 2] = h.bc.z; }
    }
    if (counters) count_hits(counters, h.id >= 0, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri);
}
template <bool COUNT, bool BARY, bool RANGE>
__global__ __launch_bounds__(256) void k_query_closest(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide,
                                                       int32_t* __restrict__ hit_id, float* __restrict__ t_out, float* __restrict__ bary,
                                                       unsigned long long* __restrict__ counters, QueryRange tr) {
    query_closest_rays<COUNT, BARY, RANGE, false>(s, n_rays, rays, wide, hit_id, t_out, bary, counters, tr);
}
template <bool COUNT, bool BARY>
__global__ __launch_bounds__(256) void k_query_closest_masked(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide,
                                                              int32_t* __restrict__ hit_id, float* __restrict__ t_out, float* __restrict__ bary,
                                                              unsigned long long* __restrict__ counters, QueryRange tr, QueryMask qm) {
    query_closest_rays<COUNT, BARY, true, true>(s, n_rays, rays, wide, hit_id, t_out, bary, counters, tr, qm);
}

// =================================================================================================
// The K nearest hits of caller-supplied rays (srt_trace_rays_multi): query_walk as it stands -- the same nodes, the same pairs, the same
// tests with the owner's ray and interval -- with a merge that keeps more than the minimum.
// MergeMulti: k slots of 64 keys per wave (slot[j][owner], all ~0 at the start) and one counter per ray.  A key is carried down the slots:
//     old = atomicMin(&slot[j][owner], carry); carry = max(old, carry);        stop at carry == ~0
// Slot j keeps the minimum of everything offered to it and passes on everything else (and one ~0), so by induction it ends as the
// (j + 1)-th smallest key of the ray, whatever the interleaving of the lanes that offer; keys of one ray differ because ids differ, and
// a qualifying t is >= 0 or -0 (srt_device.h), so key order is (t with -0 as +0, id) order.  What falls off slot k - 1 is dropped.
// After the walk the owning lane turns each kept key into (id, t) through winner_at, as k_query_closest does for its winner: t is
// recomputed from the lane's own ray, because the key holds -0 as +0.  Rows leave TRANSPOSED: the (id, t bits) pairs go back into the
// lane's own slots, and the wave then stores its 64 x k ids and its 64 x k t as 64 consecutive words per instruction (row i of the output IS words i*k .. i*k+k-1);
// SRT_MULTI_LANE_STORES builds the other choice, every lane storing its own row (measured: DESIGN.md s5).  bary, 3 floats a hit, is
// stored by the owning lane either way.
// KB: the slots the build reserves (k <= KB): 4, 8 or 16 -- 8, 16 or 32 KB of LDS a workgroup -- so that a small k keeps its occupancy.
// A NULL interval runs the RANGE walk with (NaN, NaN), which bounds nothing.
// counters: as k_query_closest's; a hit ray is one with n_hits > 0.
// =================================================================================================
struct MergeMulti {
    unsigned long long (*slot)[64];
    uint32_t* cnt;                // 64 words: qualifying candidates of the lane's ray
    uint32_t k;
    __device__ __forceinline__ void init(const uint32_t lane) const {
        for (uint32_t j = 0; j < k; j++) slot[j][lane] = ~0ull;
        cnt[lane] = 0u;
    }
    __device__ __forceinline__ void offer(const uint32_t src, const uint32_t tri, const float t) const {
        atomicAdd(&cnt[src], 1u);
        unsigned long long carry = hit_key(t, tri);
        for (uint32_t j = 0; j < k && carry != ~0ull; j++) {
            const unsigned long long old = atomicMin(&slot[j][src], carry);
            carry = old > carry ? old : carry;
        }
    }
};

template <bool COUNT, bool BARY, int KB>
__global__ __launch_bounds__(256) void k_query_multi(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryRange tr, uint32_t k,
                                                     uint32_t* __restrict__ n_hits, int32_t* __restrict__ hit_id, float* __restrict__ t_out,
                                                     float* __restrict__ bary, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long slot_all[4][KB][64];
    __shared__ uint32_t cnt_all[256];
    __shared__ float ray_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long (*slot)[64] = slot_all[wave];
    uint32_t* cnt = cnt_all + wave * 64;
    k = k < (uint32_t)KB ? k : (uint32_t)KB;            // (the host picks KB >= k)
    const size_t base = wave_base(wave), ri = base + lane;
    const bool live = ri < (size_t)n_rays;
    unsigned long long n_node = 0, n_tri = 0;
    QueryRay r;
    query_ray_opt(r, rays, wide, tr, ri, live);
    const V3 o = r.o, d = r.d;
    query_walk<COUNT, true>(s, live, o, d, lane, q_all[wave], MergeMulti{ slot, cnt, k }, ray_all[wave], n_node, n_tri, r.t_min, r.t_max);
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    const bool is_hit = live && cnt[lane] != 0u;
    if (n_hits && live) n_hits[ri] = cnt[lane];
    if (hit_id || t_out || BARY) {
        for (uint32_t j = 0; j < k; j++) {
            WinnerAt h;
            winner_at<BARY>(h, tris4, slot[j][lane], o, d);      // (t and bary of THIS hit)
            if (live) {
                const size_t at = ri * k + j;
#ifdef SRT_MULTI_LANE_STORES
                store_hit(hit_id, t_out, at, h.id, h.t);
#endif
                if (BARY) { bary[at * 3] = h.bc.x; bary[at * 3 + 1] = h.bc.y; bary[at * 3 + 2] = h.bc.z; }
            }
#ifndef SRT_MULTI_LANE_STORES
            slot[j][lane] = ((unsigned long long)__float_as_uint(h.t) << 32) | (uint32_t)h.id;
#endif
        }
#ifndef SRT_MULTI_LANE_STORES
        __builtin_amdgcn_wave_barrier();
        if (base < (size_t)n_rays) {                    // wave-uniform
            const size_t left = (size_t)n_rays - base;
            const uint32_t words = (uint32_t)(left < 64 ? left : 64) * k;      // the wave's rows are words [base * k, base * k + words)
            for (uint32_t w = lane; w < words; w += 64u) {
                const uint32_t r = w / k, j = w - r * k;
                const unsigned long long v = slot[j][r];
                if (hit_id) hit_id[base * k + w] = (int32_t)(uint32_t)v;
                if (t_out) t_out[base * k + w] = __uint_as_float((uint32_t)(v >> 32));
            }
        }
#endif
    }
    if (counters) count_hits(counters, is_hit, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri);
}

// =================================================================================================
// Occlusion of caller-supplied rays: shadowIntersection:321-342 over every object but skip_obj[i] -- the oracle's anyhit_in_tree.
// One ray per lane, each on its own walk (any_hit_range, filtered slab test; the skipped object's node range is stepped over).
// An entry of skip_obj outside [0, n_objects) skips nothing.
// RANGE: only a result in range of the ray's own interval tr blocks.
// MASK (srt_occluded_masked): the MASK walk with qm.ray[i] against qm.obj; skip_obj still leaves its object out, on top of the masks.  One
// build: the RANGE walk under the run-time convention, a NULL interval running as (NaN, NaN).
// The loads keep this order -- the ray, the skipped object's range, the interval, the mask -- and so do not go through query_ray: the
// order is what the compiler schedules, and k_query_any_masked, the one query kernel that is no template, lies among the render kernels.
// =================================================================================================
template <bool RANGE, bool MASK>
__device__ __forceinline__ void query_any_rays(const DevScene& s, const uint32_t n_rays, const float* __restrict__ rays, const uint32_t wide,
                                               const int32_t* __restrict__ skip_obj, uint8_t* __restrict__ occluded, const QueryRange tr, const QueryMask qm = QueryMask{}) {
    static_assert(RANGE || !MASK, "the masked walk is the RANGE walk");
    const size_t ri = lane_ray();
    if (ri >= (size_t)n_rays) return;
    V3 o, d;
    load_ray(rays, ri, wide != 0, o, d);
    int2 self = make_int2(-1, -1);
    if (skip_obj) {
        const int32_t k = skip_obj[ri];
        if (k >= 0 && (uint32_t)k < s.n_objects) self = s.obj_range[k];
    }
    float t_min = MASK ? __builtin_nanf("") : 0.0f, t_max = t_min;
    if (MASK ? tr.t != nullptr : RANGE) load_range(tr, ri, t_min, t_max);
    const uint32_t m = MASK && qm.ray ? qm.ray[ri] : 0xFFFFFFFFu;
    unsigned long long n_node = 0, n_tri = 0;
    occluded[ri] = any_hit_range<false, true, RANGE, MASK>(s, self, o, d, n_node, n_tri, t_min, t_max, qm.obj, m) ? 1 : 0;
}
template <bool RANGE>
__global__ __launch_bounds__(256) void k_query_any(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide,
                                                   const int32_t* __restrict__ skip_obj, uint8_t* __restrict__ occluded, QueryRange tr) {
    query_any_rays<RANGE, false>(s, n_rays, rays, wide, skip_obj, occluded, tr);
}
__global__ __launch_bounds__(256) void k_query_any_masked(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide,
                                                          const int32_t* __restrict__ skip_obj, uint8_t* __restrict__ occluded, QueryRange tr, QueryMask qm) {
    query_any_rays<true, true>(s, n_rays, rays, wide, skip_obj, occluded, tr, qm);
}

// =================================================================================================
// Shaded colour of caller-supplied rays (srt_shade_rays): per ray the one pixel of the oracle's 1 x 1 camera-mode frame -- closest hit,
// softShadow:348-401 (shadow rays, Phong, the light-sample sum), tone map, quantiser, background rule -- in ONE launch: hit id and t stay
// in registers between the two phases, so the call needs no buffer of its own.
// Phase 1 is k_query_closest's walk (query_walk with MergeClosest).
// Phase 2, a wave at a time and with no barrier between waves: the wave's h hit rays are ranked (ballot + mbcnt) and leave their shadow
// origin so = o + d * t and their object's node range in the wave's LDS, by rank (the rays' slots: phase 1 is over).  The light samples go
// in chunks of up to 64, in light order; a chunk's h * m work items (rank, sample) are dealt to the 64 lanes round after round --
// consecutive lanes take consecutive samples of one hit, so a round's rays leave few points -- each lane runs any_hit_range for its item
// and ORs the answer into the hit's 64-bit word in LDS.  After a chunk every hit's own lane adds the chunk's samples with the chunk's
// mask (add_light_samples).  A wave with 3 hits and 16 samples so keeps 48 lanes walking where one lane per ray would keep 3.
// The surface (surface_at) is fetched once per hit, before the first chunk; the pixel leaves through store_pixel.
// RANGE (srt_shade_rays_range): phase 1 keeps the closest candidate in range of the ray's own interval tr, as k_query_closest<.., true> does;
// phase 2 is the same code on that hit -- the origin is not moved, the shadow rays stay unbounded.
// counters: as k_query_closest's, and [3] / [4] node / triangle tests of the shadow rays (COUNT).
// =================================================================================================
struct QueryShade {
    const float* lights;          // device, n_lights x 3
    uint32_t n_lights;
    float shadow_div, reinhard, gamma;
    uint32_t bg;                  // r | g << 8 | b << 16
    uint32_t spread;              // a wave owns 8 groups of 8 consecutive rays, the groups a 64th of the batch apart, instead of 64 consecutive rays
};

// Phase 2 of a shading query (the header comment above) for the 64 rays of one wave after their walk, as functions: the path kernels
// shade every segment and every side ray through them, k_query_ao and k_render_ao call the first.  k_query_shade below still carries the
// same statements inline: called from there the functions keep its VGPR, scratch and LDS figures, but its RANGE builds measured 1.5 ..
// 3 % slower on row-major rays, twice (profiles/query_refactor_probe.txt), so that kernel was left as it was.  Whoever changes one changes the
// other: tests/test_gpu_shade_paths.py compares the two bit for bit.  Two steps, because a kernel stores hit_id and t between them.
// shade_hits_rank: the wave's hits are ranked; a hit gets its t (the winner's own bits) and its surface, and leaves its shadow origin and
// its object's node range in the wave's LDS by rank.  A lane without a hit gets t = +inf and a surface that shades to nothing.
struct WaveHits { uint32_t nh, rank; };       // hits in the wave; this lane's rank among them
// The shadow rule of the srt_*_paths_shadow calls (include/srt.h, "Shadow rays with an end") as the SHADOW builds receive it: a shadow ray
// blocks only inside the closed (t_min, t_max), in units of L - so, and with self != 0 the hit object's own tree is walked too.  self costs
// nothing in the walk: shade_hits_rank leaves (-1, -1) -- "skip no object", as k_query_any has it -- where the object's node range would go.
struct ShadowRule { float t_min, t_max; uint32_t self; };
// GIVEN (k_query_ao on hits the caller brings): t comes in with the hit and is taken as it is -- nothing recomputes it, a lane without a hit
// keeps what it was given.
template <bool SMOOTH, bool SHADOW = false, bool GIVEN = false>
__device__ __forceinline__ WaveHits shade_hits_rank(const DevScene& s, const bool is_hit, const int32_t id, const V3 o, const V3 d, float& t, Surface& f,
                                                    float (*wray)[64], const uint32_t walk_self = 0u) {
    if (!GIVEN) t = __builtin_inff();
    no_surface(f, 1.0f);
    const unsigned long long hm = __ballot(is_hit);
    const uint32_t nh = (uint32_t)__popcll(hm), rank = lane_prefix(hm);
    __builtin_amdgcn_wave_barrier();                    // every lane has read its key: the slots are free
    if (is_hit) {
        if (!GIVEN) {
            V3 p1, e1, e2;
            load_tri_edges(reinterpret_cast<const float4*>(s.tris), (size_t)id, p1, e1, e2);
            t = ray_triangle(o, d, p1, e1, e2);         // the winner's t with its own bits (incl. the sign of a zero); the walk's value, hence in range
        }
        const V3 P = o + d * t;                         // shadowIntersection:325-326 in camera mode: so = o + d * t
        int2 self = s.obj_range[s.tri_obj[id]];
        if (SHADOW && walk_self) self = make_int2(-1, -1);
        wray[0][rank] = P.x; wray[1][rank] = P.y; wray[2][rank] = P.z;
        wray[3][rank] = __int_as_float(self.x); wray[4][rank] = __int_as_float(self.y);
        f = surface_at(s, id, o, d, t, SMOOTH);
    }
    return WaveHits{ nh, rank };
}
// shade_hits_lights: the shadow rays of the wave's hits in chunks of 64 light samples, dealt to all 64 lanes, and each hit's light-sample sum.
// SHADOW: a shadow ray blocks only in range of (sh_min, sh_max) -- any_hit_range's RANGE walk, the one k_query_any<true> runs.
// MASK: every shadow ray is walked with sh_mask against obj_mask -- any_hit_range's MASK walk, the one k_query_any_masked runs.
template <bool COUNT, bool INT_SHIN, bool SHADOW = false, bool MASK = false>
__device__ __forceinline__ V3 shade_hits_lights(const DevScene& s, const QueryShade& p, const uint32_t lane, const bool is_hit, const WaveHits wh, const V3 o, const V3 d,
                                                const float t, const Surface& f, float (*wray)[64], unsigned long long* best, unsigned long long& n_node_s,
                                                unsigned long long& n_tri_s, const float sh_min = 0.0f, const float sh_max = 0.0f,
                                                const uint32_t* __restrict__ obj_mask = nullptr, const uint32_t sh_mask = 0u) {
    const uint32_t nh = wh.nh, rank = wh.rank;
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t l0 = 0; l0 < p.n_lights; l0 += 64u) {                                             // wave-uniform
        const uint32_t m = p.n_lights - l0 < 64u ? p.n_lights - l0 : 64u;
        if (is_hit) best[rank] = 0ull;
        __builtin_amdgcn_wave_barrier();
        const uint32_t items = nh * m;                                                              // <= 4096
        for (uint32_t w = lane; w < items; w += 64u) {
            const uint32_t r = w / m, k = w - r * m;
            const V3 so = mk(wray[0][r], wray[1][r], wray[2][r]);
            const int2 self = make_int2(__float_as_int(wray[3][r]), __float_as_int(wray[4][r]));
            const float* lp = p.lights + (size_t)(l0 + k) * 3;
            const V3 sd = mk(lp[0], lp[1], lp[2]) - so;
            if (any_hit_range<COUNT, true, SHADOW, MASK>(s, self, so, sd, n_node_s, n_tri_s, sh_min, sh_max, obj_mask, sh_mask)) atomicOr(&best[r], 1ull << k);
        }
        __builtin_amdgcn_wave_barrier();
        if (is_hit) {
            const unsigned long long mask = best[rank];
            add_light_samples<INT_SHIN>(sum, f, o, d, t, p.lights, l0, m, p.shadow_div, [&](uint32_t l) -> bool { return (mask >> (l - l0)) & 1ull; });
        }
        __builtin_amdgcn_wave_barrier();
    }
    return sum;
}

template <bool COUNT, bool SMOOTH, bool INT_SHIN, bool RANGE>
__global__ __launch_bounds__(256) void k_query_shade(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p,
                                                     int32_t* __restrict__ hit_id, float* __restrict__ t_out, float* __restrict__ rgb_linear,
                                                     uint8_t* __restrict__ rgb8, unsigned long long* __restrict__ counters, QueryRange tr) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][RANGE ? 8 : 6][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    float (*wray)[64] = ray_all[wave];
    const size_t ri = ray_deal(p.spread, wave)(lane);
    const bool live = ri < (size_t)n_rays;
    unsigned long long n_node = 0, n_tri = 0, n_node_s = 0, n_tri_s = 0;
    QueryRay r;
    query_ray<RANGE>(r, rays, wide, tr, ri, live);
    const V3 o = r.o, d = r.d;
    query_walk<COUNT, RANGE>(s, live, o, d, lane, q_all[wave], MergeClosest{ best }, wray, n_node, n_tri, r.t_min, r.t_max);
    const Winner h = winner_of(live ? best[lane] : ~0ull);
    const bool is_hit = h.is_hit;
    const int32_t id = h.id;
    float t = __builtin_inff();
    Surface f;
    no_surface(f, 1.0f);
    const unsigned long long hm = __ballot(is_hit);
    const uint32_t nh = (uint32_t)__popcll(hm), rank = lane_prefix(hm);
    __builtin_amdgcn_wave_barrier();                    // every lane has read its key: the slots are free
    if (is_hit) {
        V3 p1, e1, e2;
        load_tri_edges(reinterpret_cast<const float4*>(s.tris), (size_t)id, p1, e1, e2);
        t = ray_triangle(o, d, p1, e1, e2);             // the winner's t with its own bits (incl. the sign of a zero); the walk's value, hence in range
        const V3 P = o + d * t;                         // shadowIntersection:325-326 in camera mode: so = o + d * t
        const int2 self = s.obj_range[s.tri_obj[id]];
        wray[0][rank] = P.x; wray[1][rank] = P.y; wray[2][rank] = P.z;
        wray[3][rank] = __int_as_float(self.x); wray[4][rank] = __int_as_float(self.y);
        f = surface_at(s, id, o, d, t, SMOOTH);
    }
    if (live) store_hit(hit_id, t_out, ri, id, t);
    V3 sum = mk(0.0f, 0.0f, 0.0f);
    for (uint32_t l0 = 0; l0 < p.n_lights; l0 += 64u) {                                             // wave-uniform
        const uint32_t m = p.n_lights - l0 < 64u ? p.n_lights - l0 : 64u;
        if (is_hit) best[rank] = 0ull;
        __builtin_amdgcn_wave_barrier();
        const uint32_t items = nh * m;                                                              // <= 4096
        for (uint32_t w = lane; w < items; w += 64u) {
            const uint32_t r = w / m, k = w - r * m;
            const V3 so = mk(wray[0][r], wray[1][r], wray[2][r]);
            const int2 self = make_int2(__float_as_int(wray[3][r]), __float_as_int(wray[4][r]));
            const float* lp = p.lights + (size_t)(l0 + k) * 3;
            const V3 sd = mk(lp[0], lp[1], lp[2]) - so;
            if (any_hit_range<COUNT, true>(s, self, so, sd, n_node_s, n_tri_s)) atomicOr(&best[r], 1ull << k);
        }
        __builtin_amdgcn_wave_barrier();
        if (is_hit) {
            const unsigned long long mask = best[rank];
            add_light_samples<INT_SHIN>(sum, f, o, d, t, p.lights, l0, m, p.shadow_div, [&](uint32_t l) -> bool { return (mask >> (l - l0)) & 1ull; });
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) store_pixel(rgb_linear, rgb8, ri, sum, is_hit, p.reinhard, p.gamma, p.bg, 0u);
    if (counters) count_hits(counters, is_hit, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}

// =================================================================================================
// The surface at a hit (srt_surface_rays, srt_surface_hits): what k_query_shade looks up for its Phong and then drops -- the owning
// object, the point o + d * t, the normal, the colour (the object's or the texel), the material -- and the mirrored ray, as arrays of
// their own.  Neither kernel restates anything: the walk is query_walk with MergeClosest as k_query_closest instantiates it, the surface
// is surface_at, and both kernels leave through surface_store, so that the two entry points cannot drift apart.
// The mirrored direction is glm::reflect's association, d - (N * dot(N, d)) * 2 with dot = (x + y) + z, in f32 without contraction; it
// is the same under N -> -N, so the normal needs no orientation.  A miss row: obj -1, every float 0.
// The stores: an n x 3 (n x 6) output is 12 B (24 B) a row, a stride no lane-per-row store coalesces.  Rows leave TRANSPOSED instead, as
// k_query_multi's do: every lane puts its row into `stage` -- 64 * 6 words of the wave's own LDS, the rays' slots once the walk is over
// -- and the wave writes the 192 (384) words of its rows as 3 (6) stores of 64 consecutive words; words lane * 3 + c fall on distinct
// banks.  SRT_SURFACE_LANE_STORES builds the other choice, every lane storing its own row (measured: DESIGN.md s5).  obj, one word a
// row, is coalesced as it stands.  A NULL output costs a wave-uniform branch on a kernel argument.
// =================================================================================================
// rows: the wave's live rays (its first `rows` lanes), base: the wave's first ray; K words a row from v[] to dst[(base + lane) * K ..].
template <int K>
__device__ __forceinline__ void store_rows(float* __restrict__ dst, const size_t base, const uint32_t lane, const uint32_t rows, const float (&v)[K], float* stage) {
#ifdef SRT_SURFACE_LANE_STORES
    if (lane < rows) {
        #pragma unroll
        for (int c = 0; c < K; c++) dst[(base + lane) * K + c] = v[c];
    }
#else
    #pragma unroll
    for (int c = 0; c < K; c++) stage[lane * K + c] = v[c];
    __builtin_amdgcn_wave_barrier();
    #pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t w = (uint32_t)j * 64u + lane;
        if (w < rows * K) dst[base * K + w] = stage[w];
    }
    __builtin_amdgcn_wave_barrier();                    // the next output reuses the stage
#endif
}

// The mirrored direction of d at a surface with normal N (srt_surface_out.bounce, and the next segment of k_query_path).
__device__ __forceinline__ V3 mirror_dir(const V3 d, const V3 N) {
    const float k = (d.x * N.x + d.y * N.y) + d.z * N.z;
    return mk(d.x - (N.x * k) * 2.0f, d.y - (N.y * k) * 2.0f, d.z - (N.z * k) * 2.0f);
}

// The transmitted direction of d at a surface with outward normal N and index of refraction n (include/srt.h, "Refracting paths"): Snell's
// law in glm::normalize's and glm::refract's operations, every step f32 without contraction.  c < 0: the ray enters the solid (eta = 1 / n),
// otherwise it leaves it (the normal flipped, eta = n).  The result is scaled back to d's length, so that t of the next segment stays in the
// caller's units.  k < 0 is total internal reflection: mirror_dir(d, N), d not normalised; a NaN k goes the refracted way and stays NaN.
// Straight-line code: the choices are selects, and nothing here is live once the direction is returned.
__device__ __forceinline__ V3 refract_dir(const V3 d, const V3 N, const float n) {
    const float L = sqrtf(dot3(d, d)), inv = 1.0f / L;
    const V3 I = mk(d.x * inv, d.y * inv, d.z * inv);
    const float c = dot3(N, I);
    const bool entering = c < 0.0f;
    const V3 Nf = entering ? N : neg(N);
    const float dv = entering ? c : -c, eta = entering ? 1.0f / n : n;
    const float k = 1.0f - (eta * eta) * (1.0f - dv * dv);
    const float sn = eta * dv + sqrtf(k);
    const V3 r = mk((eta * I.x - sn * Nf.x) * L, (eta * I.y - sn * Nf.y) * L, (eta * I.z - sn * Nf.z) * L);
    const V3 m = mirror_dir(d, N);
    const bool tir = k < 0.0f;
    return mk(tir ? m.x : r.x, tir ? m.y : r.y, tir ? m.z : r.z);
}

// refract_dir's statements with three of their intermediates returned beside the direction: `entering`, `dv` and `k` are what the Fresnel
// weight of the FRESNEL builds is made of (schlick_weight).  refract_dir itself is left as it is: as a call of this
// function with the three dropped, the REFRACT path builds measured 1 % slower at 16 light samples (profiles/query_refactor_probe.txt).
// So whoever changes one changes the other: tests/test_gpu_fresnel.py compares the two calls bit for bit.
__device__ __forceinline__ V3 refract_dir_parts(const V3 d, const V3 N, const float n, bool& entering, float& dv, float& k) {
    const float L = sqrtf(dot3(d, d)), inv = 1.0f / L;
    const V3 I = mk(d.x * inv, d.y * inv, d.z * inv);
    const float c = dot3(N, I);
    entering = c < 0.0f;
    const V3 Nf = entering ? N : neg(N);
    dv = entering ? c : -c;
    const float eta = entering ? 1.0f / n : n;
    k = 1.0f - (eta * eta) * (1.0f - dv * dv);
    const float sn = eta * dv + sqrtf(k);
    const V3 r = mk((eta * I.x - sn * Nf.x) * L, (eta * I.y - sn * Nf.y) * L, (eta * I.z - sn * Nf.z) * L);
    const V3 m = mirror_dir(d, N);
    const bool tir = k < 0.0f;
    return mk(tir ? m.x : r.x, tir ? m.y : r.y, tir ? m.z : r.z);
}

// Schlick's weight of the reflected share at a glass hit (include/srt.h, "Fresnel split"): x is the cosine on the thin side -- the
// incident one going in, the transmitted one going out.  A polynomial, f32 without contraction; nothing is clamped.
__device__ __forceinline__ float schlick_weight(const float f0, const bool entering, const float dv, const float k) {
    const float x = entering ? -dv : sqrtf(k);
    const float m = 1.0f - x, m2 = m * m, m5 = (m2 * m2) * m;
    return f0 + (1.0f - f0) * m5;
}

// (is_hit, id, o, d, t, the surface there) -> the row of every wanted output.  Called by the whole wave (base < n_rays is wave-uniform).
__device__ __forceinline__ void surface_store(const DevScene& s, const srt_surface_out& out, const size_t base, const uint32_t lane, const uint32_t rows,
                                              const bool is_hit, const int32_t id, const V3 o, const V3 d, const float t, const Surface& f, float* stage) {
    const V3 zero = mk(0.0f, 0.0f, 0.0f);
    const V3 P = is_hit ? o + d * t : zero;
    const V3 N = is_hit ? f.nrm : zero;
    if (out.obj && lane < rows) out.obj[base + lane] = is_hit ? s.tri_obj[id] : -1;
    if (out.point) { const float v[3] = { P.x, P.y, P.z }; store_rows<3>(out.point, base, lane, rows, v, stage); }
    if (out.normal) { const float v[3] = { N.x, N.y, N.z }; store_rows<3>(out.normal, base, lane, rows, v, stage); }
    if (out.color) {
        const V3 c = is_hit ? f.color : zero;
        const float v[3] = { c.x, c.y, c.z };
        store_rows<3>(out.color, base, lane, rows, v, stage);
    }
    if (out.material) {
        const float v[3] = { is_hit ? f.ka : 0.0f, is_hit ? f.ks : 0.0f, is_hit ? f.sh : 0.0f };
        store_rows<3>(out.material, base, lane, rows, v, stage);
    }
    if (out.bounce) {
        const V3 r = is_hit ? mirror_dir(d, N) : zero;
        const float v[6] = { P.x, P.y, P.z, r.x, r.y, r.z };
        store_rows<6>(out.bounce, base, lane, rows, v, stage);
    }
}

// srt_surface_rays: k_query_closest's walk and winner, then the surface under it.  RANGE: as k_query_closest<.., true>.
// counters: as k_query_closest's.
template <bool COUNT, bool SMOOTH, bool RANGE>
__global__ __launch_bounds__(256) void k_query_surface(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, int32_t* __restrict__ hit_id,
                                                       float* __restrict__ t_out, srt_surface_out out, unsigned long long* __restrict__ counters, QueryRange tr) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][RANGE ? 8 : 6][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    float (*wray)[64] = ray_all[wave];
    const size_t base = wave_base(wave), ri = base + lane;
    const bool live = ri < (size_t)n_rays;
    unsigned long long n_node = 0, n_tri = 0;
    QueryRay r;
    query_ray<RANGE>(r, rays, wide, tr, ri, live);
    const V3 o = r.o, d = r.d;
    query_walk<COUNT, RANGE>(s, live, o, d, lane, q_all[wave], MergeClosest{ best }, wray, n_node, n_tri, r.t_min, r.t_max);
    WinnerAt h;
    winner_at<false>(h, reinterpret_cast<const float4*>(s.tris), live ? best[lane] : ~0ull, o, d);
    const bool is_hit = h.id >= 0;
    Surface f;
    no_surface(f, 0.0f);
    if (is_hit) f = surface_at(s, h.id, o, d, h.t, SMOOTH);
    if (live) store_hit(hit_id, t_out, ri, h.id, h.t);
    if (base < (size_t)n_rays) {                        // wave-uniform; the walk is over: the rays' slots are the stage
        const size_t left = (size_t)n_rays - base;
        surface_store(s, out, base, lane, (uint32_t)(left < 64 ? left : 64), is_hit, h.id, o, d, h.t, f, &wray[0][0]);
    }
    if (counters) count_hits(counters, is_hit, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri);
}

// srt_surface_hits: the same rows for hits the caller already holds -- no walk, no node record, no queue; one lane per row.  A row whose
// id is outside [0, n_tris) is a miss row; t is taken as given (the texel index is clamped, so any t is memory-safe).
template <bool SMOOTH>
__global__ __launch_bounds__(256) void k_query_surface_hits(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide,
                                                            const int32_t* __restrict__ hit_id, const float* __restrict__ t_in, srt_surface_out out) {
    __shared__ float stage_all[4][6 * 64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    const size_t base = wave_base(wave), ri = base + lane;
    if (base >= (size_t)n_rays) return;                 // wave-uniform
    const bool live = ri < (size_t)n_rays;
    V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    int32_t id = -1;
    float t = __builtin_inff();
    if (live) { load_ray(rays, ri, wide != 0, o, d); id = hit_id[ri]; t = t_in[ri]; }
    const bool is_hit = id >= 0 && (uint32_t)id < s.n_tris;
    Surface f;
    no_surface(f, 0.0f);
    if (is_hit) f = surface_at(s, id, o, d, t, SMOOTH);
    const size_t left = (size_t)n_rays - base;
    surface_store(s, out, base, lane, (uint32_t)(left < 64 ? left : 64), is_hit, id, o, d, t, f, stage_all[wave]);
}

// =================================================================================================
// Ambient occlusion (srt_ao_rays, srt_ao_hits): per hit, n_dirs occlusion rays from the hit point along a table of directions given in the
// hit's own frame, and how many of them are blocked -- in ONE launch: the AO rays are made in registers and never reach memory.
// One template covers both entry points.  Phase 1 -- HITS == false: query_walk exactly as query_closest_rays' MASK build instantiates it (the RANGE
// + MASK build, a NULL interval running as (NaN, NaN)) with the mask qm.primary; HITS == true: the caller's hit_id / t are loaded, an id
// outside [0, n_tris) is a miss, and nothing is walked (the build has no queue).
// Phase 2 is k_query_shade's, a wave at a time with no barrier between waves: shade_hits_rank ranks the wave's hits and leaves P and the
// skip range ((-1, -1) unless SRT_AO_SKIP_SELF) in the wave's LDS by rank; the hit's own lane adds Nf, the normal that faces the ray, in
// the three rows that are left -- the walk's 8 x 64 slots hold P (3), the range (2) and Nf (3) exactly.  The directions go in chunks of up
// to 64; a chunk's nh x m items (rank, direction) are dealt to the 64 lanes round after round, consecutive lanes taking consecutive
// directions of one hit; each lane builds the frame from Nf (ao_frame: about 15 VALU operations and one divide per item; keeping T and
// B in LDS instead would take 6 more rows a wave, 6 KB a workgroup on top of k_query_closest_masked's 20 KB, for 6 more LDS reads per
// item in their place), forms w, runs any_hit_range<COUNT, true, true, true> with qm.shadow and ORs its bit into the hit's 64-bit word
// (`best`).
// After a chunk the ray's own lane adds popcll to its count and stores the chunk's two words of occ_bits; a lane without a hit stores zeros.
// dirs is read from global memory per item: 12 B at consecutive addresses for consecutive lanes, the whole table at most 12 KB.
// The deal of rays to waves is ray_deal, as in k_query_shade, QueryAo::spread included.
// counters: as k_query_shade's -- [1] / [2] of phase 1 (0 under HITS), [3] / [4] of the AO walks (COUNT), the hit shards.
// =================================================================================================
struct QueryAo {
    const float* dirs;            // device, n_dirs x 3; n_dirs == 0: no phase 2 (nothing of srt_ao_out is wanted)
    uint32_t n_dirs;
    float t_min, t_max;           // the AO rays' interval
    uint32_t skip_self;           // SRT_AO_SKIP_SELF
    uint32_t spread;              // QueryShade::spread
};
struct QueryHits { const int32_t* hit_id; const float* t; };      // srt_ao_hits: the hits the caller brings

// The tangent and the bitangent of the frame whose third axis is n (include/srt.h, "Ambient occlusion"): no branch, no transcendental;
// every step f32 without contraction.
__device__ __forceinline__ void ao_frame(const V3 n, V3& T, V3& B) {
    const float s = __builtin_copysignf(1.0f, n.z), a = -1.0f / (s + n.z), b = (n.x * n.y) * a;
    T = mk(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    B = mk(b, s + (n.y * n.y) * a, -n.y);
}
// The normal that faces the ray d, and the AO ray's direction for the table entry (u, v, z) in the frame of that normal
__device__ __forceinline__ V3 ao_facing(const V3 d, const V3 N) {
    const float k = (d.x * N.x + d.y * N.y) + d.z * N.z;       // mirror_dir's dot
    return k > 0.0f ? neg(N) : N;
}
__device__ __forceinline__ V3 ao_ray_dir(const V3 Nf, const float u, const float v, const float z) {
    V3 T, B;
    ao_frame(Nf, T, B);
    return mk((T.x * u + B.x * v) + Nf.x * z, (T.y * u + B.y * v) + Nf.y * z, (T.z * u + B.z * v) + Nf.z * z);
}

// The rotation of a table entry about the frame's third axis (include/srt.h, "Ambient occlusion in a frame"): (u, v) -> (c * u - s * v,
// s * u + c * v), each product rounded on its own.
__device__ __forceinline__ void ao_rotate(const float c, const float sn, float& u, float& v) {
    const float u0 = u, v0 = v;
    u = c * u0 - sn * v0;
    v = sn * u0 + c * v0;
}
// What ao_hits_dirs calls after each chunk when the caller wants nothing of it
struct AoNoChunk { __device__ __forceinline__ void operator()(uint32_t, uint32_t, unsigned long long) const {} };

// Phase 2 for the 64 rays of one wave after shade_hits_rank, as shade_hits_lights is for light samples.  wray[5..7][rank] is written here.
// Returns the lane's blocked directions; every live lane stores its row of occ_bits chunk by chunk.
// ROT (k_render_ao): every hit turns the table by its own (c, sn) before the frame is applied; the hit's lane leaves the pair in
// wrot[0..1][rank], two more rows of the wave's LDS, where the lanes that take its items read it.  The builds without ROT never touch wrot.
// chunk(l0, m, mask): called by every lane after each chunk with the chunk's first direction, its length and the lane's own mask (0 for a
// lane without a hit) -- k_render_ao's bent sum.
template <bool COUNT, bool ROT = false, typename Chunk = AoNoChunk>
__device__ __forceinline__ uint32_t ao_hits_dirs(const DevScene& s, const QueryAo& p, const QueryMask& qm, const uint32_t lane, const bool live, const bool is_hit,
                                                 const WaveHits wh, const V3 d, const V3 N, const size_t ri, uint32_t* __restrict__ occ_bits, float (*wray)[64],
                                                 unsigned long long* best, unsigned long long& n_node_s, unsigned long long& n_tri_s,
                                                 float (*wrot)[64] = nullptr, const float c = 0.0f, const float sn = 0.0f, const Chunk chunk = Chunk{}) {
    const uint32_t nh = wh.nh, rank = wh.rank, W = (p.n_dirs + 31u) >> 5;
    if (is_hit) {
        const V3 Nf = ao_facing(d, N);
        wray[5][rank] = Nf.x; wray[6][rank] = Nf.y; wray[7][rank] = Nf.z;
        if constexpr (ROT) { wrot[0][rank] = c; wrot[1][rank] = sn; }
    }
    uint32_t blocked = 0;
    for (uint32_t l0 = 0; l0 < p.n_dirs; l0 += 64u) {                                               // wave-uniform
        const uint32_t m = p.n_dirs - l0 < 64u ? p.n_dirs - l0 : 64u;
        if (is_hit) best[rank] = 0ull;
        __builtin_amdgcn_wave_barrier();
        const uint32_t items = nh * m;                                                              // <= 4096
        for (uint32_t w = lane; w < items; w += 64u) {
            const uint32_t r = w / m, k = w - r * m;
            const V3 P = mk(wray[0][r], wray[1][r], wray[2][r]);
            const int2 self = make_int2(__float_as_int(wray[3][r]), __float_as_int(wray[4][r]));
            const V3 Nf = mk(wray[5][r], wray[6][r], wray[7][r]);
            const float* dp = p.dirs + (size_t)(l0 + k) * 3;
            float u = dp[0], v = dp[1];
            const float z = dp[2];
            if constexpr (ROT) ao_rotate(wrot[0][r], wrot[1][r], u, v);
            const V3 wd = ao_ray_dir(Nf, u, v, z);
            if (any_hit_range<COUNT, true, true, true>(s, self, P, wd, n_node_s, n_tri_s, p.t_min, p.t_max, qm.obj, qm.shadow)) atomicOr(&best[r], 1ull << k);
        }
        __builtin_amdgcn_wave_barrier();
        const unsigned long long mask = is_hit ? best[rank] : 0ull;
        blocked += (uint32_t)__popcll(mask);
        chunk(l0, m, mask);
        if (occ_bits && live) {
            const uint32_t w0 = l0 >> 5;                                                            // the chunk's two words: w0 (< W) and w0 + 1
            occ_bits[ri * W + w0] = (uint32_t)mask;
            if (w0 + 1u < W) occ_bits[ri * W + w0 + 1u] = (uint32_t)(mask >> 32);
        }
        __builtin_amdgcn_wave_barrier();
    }
    return blocked;
}

template <bool COUNT, bool SMOOTH, bool HITS>
__global__ __launch_bounds__(256) void k_query_ao(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryRange tr, QueryMask qm, QueryAo p,
                                                  QueryHits given, int32_t* __restrict__ hit_id, float* __restrict__ t_out, srt_ao_out out,
                                                  unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    float (*wray)[64] = ray_all[wave];
    const size_t ri = ray_deal(p.spread, wave)(lane);
    const bool live = ri < (size_t)n_rays;
    unsigned long long n_node = 0, n_tri = 0, n_node_s = 0, n_tri_s = 0;
    QueryRay r;
    query_ray_opt(r, rays, wide, HITS ? QueryRange{ nullptr, 0u } : tr, ri, live);       // (HITS: nothing is walked, no interval is read)
    const V3 o = r.o, d = r.d;
    bool is_hit;
    int32_t id = -1;
    float t = __builtin_inff();
    if constexpr (HITS) {
        if (live) { id = given.hit_id[ri]; t = given.t[ri]; }
        is_hit = id >= 0 && (uint32_t)id < s.n_tris;
    } else {
        __shared__ uint32_t q_all[4][QCAP];             // the walk's queue: the HITS builds have none
        query_walk<COUNT, true, MergeClosest, true>(s, live, o, d, lane, q_all[wave], MergeClosest{ best }, wray, n_node, n_tri, r.t_min, r.t_max, qm.obj, qm.primary);
        const Winner h = winner_of(live ? best[lane] : ~0ull);
        is_hit = h.is_hit; id = h.id;
    }
    Surface f;
    const WaveHits wh = shade_hits_rank<SMOOTH, true, HITS>(s, is_hit, id, o, d, t, f, wray, p.skip_self ? 0u : 1u);
    if (!HITS && live) store_hit(hit_id, t_out, ri, id, t);
    if (p.n_dirs) {                                     // wave-uniform
        const uint32_t blocked = ao_hits_dirs<COUNT>(s, p, qm, lane, live, is_hit, wh, d, f.nrm, ri, out.occ_bits, wray, best, n_node_s, n_tri_s);
        if (live) {
            if (out.n_occluded) out.n_occluded[ri] = blocked;
            if (out.ao) out.ao[ri] = (float)(p.n_dirs - blocked) / (float)p.n_dirs;
        }
    }
    if (counters) count_hits(counters, is_hit, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}

// =================================================================================================
// Mirror paths (srt_shade_paths): a ray followed through up to path.depth mirror bounces in ONE launch, every segment shaded as
// srt_shade_rays_range shades it, the segments mixed by a per-object reflectance, the finished pixel written.  The kernel restates nothing:
// a segment is query_walk<COUNT, true, MergeClosest> (a NULL interval runs as (NaN, NaN), as in k_query_multi), then k_query_shade's
// phase 2 as it stands (shade_hits_rank, shade_hits_lights), and the next segment's ray is (o + d * t, mirror_dir(d, f.nrm)) -- the
// bounce row of surface_store -- with the interval (bounce_t_min, +inf).  What the chain of launches hands on through HBM -- the mirrored
// ray, the interval, the object, the colour -- stays in registers here, and each mirrored ray is walked once instead of twice.
// The loop over segments is wave-uniform.  A lane whose path has ended goes into the walk with live = false (no node is read, no pair
// pushed; it still tests queued pairs of its neighbours) and has no hit, so phase 2 gives it no work; the wave leaves the loop when no
// lane is alive and then writes the miss rows of the segments left.  The walks are purely geometric: reflectance ends no path and
// skips no walk.
// The mix runs from the near end, so that a lane carries acc (3), W (1) and ONE pending segment (its sum, 3, and its reflectance, 1)
// instead of an array of depth colours: segment b's weight W * (1 - k_b) needs to know whether segment b + 1 hit, so b's sum waits
// while b + 1 is walked and is added then; the last pending segment is added after the loop with k = 0.
// LDS: k_query_shade<.., RANGE = true>'s, reused per segment.  The rays' 8 x 64 slots are, in turn, the walk's rays, phase 2's ranked
// hits and the stage of the transposed row stores.  The deal of rays to waves is ray_deal, as in k_query_shade, QueryShade::spread included; under
// spread a wave's rays are 8 groups of 8 consecutive rays, so rows go out through store_rows_dealt, which is store_rows with the ray of
// a lane given by the deal instead of base + lane (without spread the addresses are store_rows' own).
// seg's rows are segment-major: row b of a field starts n_rays elements (x 3, x 6) after row b - 1.
// counters: as k_query_shade's, summed over the segments walked; a hit counts once per segment.
// Refracting paths (srt_shade_paths_refract): the REFRACT build of the same statements.  The one thing that differs is the direction of
// the next segment after a hit on an object k with ior[k] > 0: refract_dir instead of mirror_dir, from the same point, with the same
// interval.  The walk does not skip the hit's own object, so a ray that enters a solid finds its far side.
// Fresnel split (srt_shade_paths_fresnel): the FRESNEL build on top of REFRACT.  A glass hit of an object with f0 >= 0 also sends a depth-1
// side ray along mirror_dir, walked and shaded by the same statements at the end of the segment's iteration; its sum enters the near-end
// mix with Schlick's weight (path_segments).
// =================================================================================================
template <int K, typename RayOf>
__device__ __forceinline__ void store_rows_dealt(float* __restrict__ dst, const uint32_t lane, const size_t n_rays, const float (&v)[K], float* stage, RayOf ray_of) {
#ifdef SRT_SURFACE_LANE_STORES
    const size_t r = ray_of(lane);
    if (r < n_rays) {
        #pragma unroll
        for (int c = 0; c < K; c++) dst[r * K + c] = v[c];
    }
#else
    #pragma unroll
    for (int c = 0; c < K; c++) stage[lane * K + c] = v[c];
    __builtin_amdgcn_wave_barrier();
    #pragma unroll
    for (int j = 0; j < K; j++) {
        const uint32_t w = (uint32_t)j * 64u + lane, l = w / (uint32_t)K, c = w - l * (uint32_t)K;      // word w of the stage: lane l's component c
        const size_t r = ray_of(l);
        if (r < n_rays) dst[r * K + c] = stage[w];
    }
    __builtin_amdgcn_wave_barrier();                    // the next output reuses the stage
#endif
}

// The Fresnel table and the side rays' rows of the FRESNEL builds, their own kernel argument: f0, n_objects floats; out, laid out as
// srt_path_out's hit_id, t and rgb_linear (all NULL = no rows).
struct QueryFresnel { const float* f0; srt_fresnel_out out; };

// The segments of the paths of one wave's 64 rays (the header comment above), shared by k_query_path and k_render_path: the walk, phase 2,
// the per-segment rows, the mirrored ray and the near-end mix.  ri: the lane's row in every output (seg's rows are n apart), ray_of: the
// same for any lane of the wave (>= n: a lane without a ray) -- the transposed row stores need it.  seg: all NULL = no per-segment rows.
// shard: where the wave's hits are counted.  Returns the mixed sum; hit0: whether segment 0 hit.
// SHADOW: every segment's shadow rays run under `rule` (the builds without it never read it).
// MASK: segment 0 is walked with qm.primary, every later segment with qm.bounce, every shadow ray with qm.shadow, all against qm.obj
// (the builds without it never read qm).
// REFRACT: a hit on an object k with ior[k] > 0 sends the next segment along refract_dir instead of mirror_dir, chosen per lane by a
// select (the builds without it never read ior; ior is non-NULL in the builds with it).
// FRESNEL (on top of REFRACT; include/srt.h, "Fresnel split"): a hit on an object that SPLITS -- ior[k] > 0 and f0[k] >= 0 -- that is not
// totally reflected and is not the path's last segment also sends a depth-1 SIDE RAY along mirror_dir from the same point.  At the end of
// segment b's iteration, when the row stores are out and q, best and wray are free, the wave tests __ballot(split) and, if any lane
// splits, walks its side rays with the statements of a segment: query_walk with qm.bounce and (bounce_t_min, +inf), shade_hits_rank,
// shade_hits_lights under the same rule.  Across segment b + 1's walk a lane then carries the side hit's sum (3), the weight F and the
// side-hit flag beside pend / pend_k, and the mix of segment b, made when b + 1's hit is known, gives the side sum its share.  A wave
// without a split pays the ballot.  The builds without FRESNEL never read fr (fr.f0 is non-NULL in the builds with it).
template <bool COUNT, bool SMOOTH, bool INT_SHIN, bool SHADOW, bool MASK = false, bool REFRACT = false, bool FRESNEL = false, typename RayOf>
__device__ __forceinline__ V3 path_segments(const DevScene& s, const QueryShade& p, const srt_path_desc& path, const srt_path_out& seg, const size_t n, const size_t ri,
                                            const bool live, V3 o, V3 d, float t_min, float t_max, const uint32_t lane, uint32_t* q, unsigned long long* best,
                                            float (*wray)[64], const RayOf ray_of, unsigned long long* __restrict__ counters, const uint32_t shard, bool& hit0,
                                            unsigned long long& n_node, unsigned long long& n_tri, unsigned long long& n_node_s, unsigned long long& n_tri_s,
                                            const ShadowRule rule, const QueryMask qm = QueryMask{}, const float* __restrict__ ior = nullptr,
                                            const QueryFresnel fr = QueryFresnel{}) {
    static_assert(!FRESNEL || REFRACT, "a side ray is taken at a transmitting hit");
    float* stage = &wray[0][0];
    V3 acc = mk(0.0f, 0.0f, 0.0f), pend = acc;          // the mix so far; the sum of the segment that waits for its weight
    float W = 1.0f, pend_k = 0.0f;                      // the weight of what follows; the waiting segment's reflectance
    V3 side_sum = acc;                                  // FRESNEL: the waiting segment's side ray -- its hit's sum, its weight, whether it hit
    float side_F = 0.0f;
    bool side = false;
    bool alive = live, waiting = false;
    hit0 = false;
    uint32_t b = 0;
    for (; b < path.depth && __ballot(alive); b++) {                                                // wave-uniform
        query_walk<COUNT, true, MergeClosest, MASK>(s, alive, o, d, lane, q, MergeClosest{ best }, wray, n_node, n_tri, t_min, t_max, qm.obj, b == 0 ? qm.primary : qm.bounce);
        const Winner h = winner_of(alive ? best[lane] : ~0ull);
        const bool is_hit = h.is_hit;
        const int32_t id = h.id;
        float t;
        Surface f;
        const WaveHits wh = shade_hits_rank<SMOOTH, SHADOW>(s, is_hit, id, o, d, t, f, wray, rule.self);
        const int32_t obj = is_hit ? s.tri_obj[id] : -1;
        const size_t row = (size_t)b * n;
        if (live) {                                     // (not store_hit: seg's pointers are read where they are tested, not ahead of both tests)
            if (seg.hit_id) seg.hit_id[row + ri] = id;
            if (seg.t) seg.t[row + ri] = t;
            if (seg.obj) seg.obj[row + ri] = obj;
        }
        const V3 sum = shade_hits_lights<COUNT, INT_SHIN, SHADOW, MASK>(s, p, lane, is_hit, wh, o, d, t, f, wray, best, n_node_s, n_tri_s, rule.t_min, rule.t_max, qm.obj, qm.shadow);
        __builtin_amdgcn_wave_barrier();                // phase 2 is over: the rays' slots are the stage
        if (seg.rgb_linear) { const float v[3] = { sum.x, sum.y, sum.z }; store_rows_dealt<3>(seg.rgb_linear + row * 3, lane, n, v, stage, ray_of); }
        if (seg.rays) {
            const float v[6] = { alive ? o.x : 0.0f, alive ? o.y : 0.0f, alive ? o.z : 0.0f, alive ? d.x : 0.0f, alive ? d.y : 0.0f, alive ? d.z : 0.0f };
            store_rows_dealt<6>(seg.rays + row * 6, lane, n, v, stage, ray_of);
        }
        if (counters) count_hits(counters, is_hit, shard);
        if (waiting) {                                  // segment b - 1 hit: its weight is known now
            if (FRESNEL) {                              // a branch that misses gives its share to the other; no side ray: W = Wk * 1
                const float k = (is_hit || side) ? pend_k : 0.0f, a = W * (1.0f - k), Wk = W * k;
                acc = mk(acc.x + a * pend.x, acc.y + a * pend.y, acc.z + a * pend.z);
                const float Fe = side ? (is_hit ? side_F : 1.0f) : 0.0f;
                if (side) {
                    const float g = Wk * Fe;
                    acc = mk(acc.x + g * side_sum.x, acc.y + g * side_sum.y, acc.z + g * side_sum.z);
                }
                W = Wk * (1.0f - Fe);
            } else {
                const float k = is_hit ? pend_k : 0.0f, a = W * (1.0f - k);
                acc = mk(acc.x + a * pend.x, acc.y + a * pend.y, acc.z + a * pend.z);
                W = W * k;
            }
        }
        waiting = is_hit;
        if (b == 0) hit0 = is_hit;
        bool split = false;                             // FRESNEL: this lane's hit takes a side ray, along sdir, with the weight F
        V3 sdir = mk(0.0f, 0.0f, 0.0f);
        float F = 0.0f;
        if (is_hit) {
            pend = sum;
            pend_k = path.reflectance ? path.reflectance[obj] : 0.0f;
            const V3 P = o + d * t;                     // the bounce row of surface_store: the point, not moved, and the mirrored direction
            if (FRESNEL) {
                const float n_obj = ior[obj], f0 = fr.f0[obj];
                bool entering;
                float dv, k;
                const V3 m = mirror_dir(d, f.nrm), r = refract_dir_parts(d, f.nrm, n_obj, entering, dv, k);
                const bool glass = n_obj > 0.0f;
                d = mk(glass ? r.x : m.x, glass ? r.y : m.y, glass ? r.z : m.z);
                split = glass && f0 >= 0.0f && !(k < 0.0f) && b + 1 < path.depth;      // (a negative or NaN f0: no split; a NaN k splits)
                if (split) { sdir = m; F = schlick_weight(f0, entering, dv, k); }
            } else if (REFRACT) {
                const float n_obj = ior[obj];           // (0, negative, NaN: the object mirrors)
                const V3 m = mirror_dir(d, f.nrm), r = refract_dir(d, f.nrm, n_obj);
                const bool glass = n_obj > 0.0f;
                d = mk(glass ? r.x : m.x, glass ? r.y : m.y, glass ? r.z : m.z);
            } else {
                d = mirror_dir(d, f.nrm);
            }
            o = P;
            t_min = path.bounce_t_min; t_max = __builtin_inff();
        }
        alive = is_hit;
        if (FRESNEL) {
            // the side rays of segment b: from the hit point (o by now), not moved, along the mirrored direction
            int32_t sid = -1;
            float st = __builtin_inff();
            V3 ssum = mk(0.0f, 0.0f, 0.0f);
            side = false;
            if (__ballot(split)) {                      // wave-uniform
                query_walk<COUNT, true, MergeClosest, MASK>(s, split, o, sdir, lane, q, MergeClosest{ best }, wray, n_node, n_tri, path.bounce_t_min, __builtin_inff(),
                                                            qm.obj, qm.bounce);
                const Winner sh = winner_of(split ? best[lane] : ~0ull);
                side = sh.is_hit; sid = sh.id;
                Surface sf;
                const WaveHits swh = shade_hits_rank<SMOOTH, SHADOW>(s, side, sid, o, sdir, st, sf, wray, rule.self);
                ssum = shade_hits_lights<COUNT, INT_SHIN, SHADOW, MASK>(s, p, lane, side, swh, o, sdir, st, sf, wray, best, n_node_s, n_tri_s, rule.t_min, rule.t_max,
                                                                        qm.obj, qm.shadow);
                __builtin_amdgcn_wave_barrier();        // phase 2 is over: the rays' slots are the stage
                if (counters) count_hits(counters, side, shard);
            }
            if (live) {
                if (fr.out.hit_id) fr.out.hit_id[row + ri] = sid;
                if (fr.out.t) fr.out.t[row + ri] = st;
                if (fr.out.fresnel) fr.out.fresnel[row + ri] = F;
            }
            if (fr.out.rgb_linear) { const float v[3] = { ssum.x, ssum.y, ssum.z }; store_rows_dealt<3>(fr.out.rgb_linear + row * 3, lane, n, v, stage, ray_of); }
            side_sum = ssum; side_F = F;
        }
    }
    if (waiting) {                                      // the last segment that hit: nothing follows it, k = 0
        const float a = W * (1.0f - 0.0f);
        acc = mk(acc.x + a * pend.x, acc.y + a * pend.y, acc.z + a * pend.z);
    }
    for (; b < path.depth; b++) {                       // wave-uniform: the segments no lane of the wave walked are miss rows
        const size_t row = (size_t)b * n;
        if (live) {
            if (seg.hit_id) seg.hit_id[row + ri] = -1;
            if (seg.t) seg.t[row + ri] = __builtin_inff();
            if (seg.obj) seg.obj[row + ri] = -1;
        }
        if (seg.rgb_linear) { const float v[3] = { 0.0f, 0.0f, 0.0f }; store_rows_dealt<3>(seg.rgb_linear + row * 3, lane, n, v, stage, ray_of); }
        if (seg.rays) { const float v[6] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f }; store_rows_dealt<6>(seg.rays + row * 6, lane, n, v, stage, ray_of); }
        if (FRESNEL) {
            if (live) {
                if (fr.out.hit_id) fr.out.hit_id[row + ri] = -1;
                if (fr.out.t) fr.out.t[row + ri] = __builtin_inff();
                if (fr.out.fresnel) fr.out.fresnel[row + ri] = 0.0f;
            }
            if (fr.out.rgb_linear) { const float v[3] = { 0.0f, 0.0f, 0.0f }; store_rows_dealt<3>(fr.out.rgb_linear + row * 3, lane, n, v, stage, ray_of); }
        }
    }
    return acc;
}

// The body of both k_query_path kernels: k_query_path is what a call without a shadow rule launches, argument for argument what it was;
// k_query_path_shadow takes the rule as one more argument and is the SHADOW build of the same statements.
template <bool COUNT, bool SMOOTH, bool INT_SHIN, bool SHADOW, bool MASK = false, bool REFRACT = false, bool FRESNEL = false>
__device__ __forceinline__ void query_path_rays(const DevScene& s, const uint32_t n_rays, const float* __restrict__ rays, const uint32_t wide, const QueryShade& p,
                                                const QueryRange tr, const srt_path_desc& path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8,
                                                const srt_path_out& seg, unsigned long long* __restrict__ counters, const ShadowRule rule,
                                                const QueryMask qm = QueryMask{}, const float* __restrict__ ior = nullptr,
                                                const QueryFresnel fr = QueryFresnel{}) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    const size_t n = (size_t)n_rays;
    const RayDeal ray_of = ray_deal(p.spread, wave);
    const size_t ri = ray_of(lane);
    const bool live = ri < n;
    unsigned long long n_node = 0, n_tri = 0, n_node_s = 0, n_tri_s = 0;
    // query_ray_opt's statements, kept here: through the helper the FRESNEL builds order two register moves the other way
    V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    float t_min = __builtin_nanf(""), t_max = __builtin_nanf("");
    if (live) load_ray(rays, ri, wide != 0, o, d);
    if (tr.t && live) load_range(tr, ri, t_min, t_max);
    bool hit0;
    const V3 acc = path_segments<COUNT, SMOOTH, INT_SHIN, SHADOW, MASK, REFRACT, FRESNEL>(s, p, path, seg, n, ri, live, o, d, t_min, t_max, lane, q_all[wave],
                                                                                          best_all + wave * 64, ray_all[wave], ray_of, counters, blockIdx.x, hit0, n_node, n_tri,
                                                                                          n_node_s, n_tri_s, rule, qm, ior, fr);
    if (live) store_pixel(rgb_linear, rgb8, ri, acc, hit0, p.reinhard, p.gamma, p.bg, 0u);
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_query_path(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p, QueryRange tr,
                                                    srt_path_desc path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                    unsigned long long* __restrict__ counters) {
    query_path_rays<COUNT, SMOOTH, INT_SHIN, false>(s, n_rays, rays, wide, p, tr, path, rgb_linear, rgb8, seg, counters, ShadowRule{ 0.0f, 0.0f, 0u });
}
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_query_path_shadow(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p, QueryRange tr,
                                                           srt_path_desc path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                           unsigned long long* __restrict__ counters, ShadowRule rule) {
    query_path_rays<COUNT, SMOOTH, INT_SHIN, true>(s, n_rays, rays, wide, p, tr, path, rgb_linear, rgb8, seg, counters, rule);
}

// srt_shade_paths_masked: the SHADOW build of the same statements on the MASK walks.  A call without a rule sends the reference's rule
// as one: no bound -- (NaN, NaN) -- and the hit's object skipped.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_query_path_masked(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p, QueryRange tr,
                                                           srt_path_desc path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                           unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm) {
    query_path_rays<COUNT, SMOOTH, INT_SHIN, true, true>(s, n_rays, rays, wide, p, tr, path, rgb_linear, rgb8, seg, counters, rule, qm);
}

// srt_shade_paths_refract: the SHADOW + MASK + REFRACT build of the same statements.  A call without a rule sends the reference's rule, a
// call without masks all ones with a NULL table; ior, n_objects floats, travels by value beside the path description.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_query_path_refract(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p, QueryRange tr,
                                                            srt_path_desc path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                            unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm, const float* __restrict__ ior) {
    query_path_rays<COUNT, SMOOTH, INT_SHIN, true, true, true>(s, n_rays, rays, wide, p, tr, path, rgb_linear, rgb8, seg, counters, rule, qm, ior);
}

// srt_shade_paths_fresnel: the FRESNEL build on top of k_query_path_refract's; f0 and the side rays' rows travel by value as one more argument.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_query_path_fresnel(DevScene s, uint32_t n_rays, const float* __restrict__ rays, uint32_t wide, QueryShade p, QueryRange tr,
                                                            srt_path_desc path, float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                            unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm, const float* __restrict__ ior,
                                                            QueryFresnel fr) {
    query_path_rays<COUNT, SMOOTH, INT_SHIN, true, true, true, true>(s, n_rays, rays, wide, p, tr, path, rgb_linear, rgb8, seg, counters, rule, qm, ior, fr);
}

// =================================================================================================
// Mirror paths in a frame (srt_render_paths): k_query_path's paths for the rays of a frame's own pixels.  The front end is the render
// kernels': a wave owns one 8 x 8 pixel tile and a workgroup 16 x 16 (tile_pixel), the grid is 2-D over the call's local output, and a
// pixel's ray is primary_dir / ray_origin under the call's block or tile deal -- nothing is loaded per ray, and the 64 rays of a wave are
// neighbours that walk the same nodes.  Everything behind the ray is path_segments as k_query_path calls it; a lane's row in every output
// is its local pixel r * W + px, so the transposed stores write a tile row's 8 pixels as one 96 B (192 B) run.  Padding pixels of a tile
// deal and pixels beyond the frame are lanes without a ray: they walk nothing and write nothing.
// spp = m x m > 1: the sub-samples run one after the other in this launch (the loop is wave-uniform), each with srt_render_device's
// offsets added to dir.xy before the matrix; their mixed sums are added in order starting from sub-sample 0's, divided by (float)spp,
// and the pixel leaves once, as k_accumulate / k_resolve make it (tone-mapped whatever was hit: a black quotient is the background).
// seg's rows are sub-sample 0's.  counters: as k_query_path's, over all sub-samples; the hit shard is the 2-D workgroup number.
// =================================================================================================
// The front end of the frame kernels (k_render_path*, k_render_ao), as wave_lane / ray_deal / query_ray are the batch kernels': the lane's
// pixel (px, r) of the call's local output and whether it has one (live), its image row y, its row ri in every output (of n), the deal
// ray_of for any lane of the wave (~0: a lane without a pixel) and the shard where the workgroup's hits are counted.
struct FrameDeal {
    unsigned long long live_mask;
    uint32_t tile_x, tile_r, W;
    __device__ __forceinline__ size_t operator()(const uint32_t l) const { return (live_mask >> l) & 1ull ? (size_t)(tile_r + (l >> 3)) * W + tile_x + (l & 7u) : ~(size_t)0; }
};
struct FramePixel { uint32_t px, r, y, shard; bool live; size_t n, ri; FrameDeal ray_of; };
__device__ __forceinline__ void frame_pixel(FramePixel& at, const DevParams& fp, const uint32_t wave) {
    at.live = tile_pixel(fp, at.px, at.r);
    at.ray_of.live_mask = __ballot(at.live);
    at.ray_of.tile_x = blockIdx.x * 16 + (wave & 1) * 8; at.ray_of.tile_r = blockIdx.y * 16 + (wave >> 1) * 8; at.ray_of.W = fp.W;
    at.n = (size_t)fp.rows * fp.W; at.ri = (size_t)at.r * fp.W + at.px;
    at.shard = blockIdx.y * gridDim.x + blockIdx.x; at.y = at.live ? image_row(fp, at.r) : 0u;
}
// Sub-sample k of spp = spp_m x spp_m: srt_render_device's offsets, added to dir.xy before the matrix.  spp == 1 leaves the frame's own.
__device__ __forceinline__ void frame_sub_sample(DevParams& fp, const uint32_t spp, const uint32_t spp_m, const uint32_t k) {
    if (spp > 1) {
        fp.sub_x = ((float)(k % spp_m) + 0.5f) / (float)spp_m - 0.5f;
        fp.sub_y = ((float)(k / spp_m) + 0.5f) / (float)spp_m - 0.5f;
    }
}

// The body of both k_render_path kernels, as query_path_rays is k_query_path's.  fp: the frame's geometry; sub_x / sub_y change per sub-sample.
template <bool COUNT, bool SMOOTH, bool INT_SHIN, bool SHADOW, bool MASK = false, bool REFRACT = false, bool FRESNEL = false>
__device__ __forceinline__ void render_path_pixels(const DevScene& s, DevParams& fp, const uint32_t spp, const uint32_t spp_m, const QueryShade& p, const srt_path_desc& path,
                                                   float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, const srt_path_out& seg,
                                                   unsigned long long* __restrict__ counters, const ShadowRule rule, const QueryMask qm = QueryMask{},
                                                   const float* __restrict__ ior = nullptr, const QueryFresnel fr = QueryFresnel{}) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    FramePixel at;
    frame_pixel(at, fp, wave);
    const bool live = at.live;
    unsigned long long n_node = 0, n_tri = 0, n_node_s = 0, n_tri_s = 0;
    const V3 o = ray_origin(fp);
    V3 total = mk(0.0f, 0.0f, 0.0f);
    bool hit0 = false;
    for (uint32_t k = 0; k < spp; k++) {                                                            // wave-uniform
        frame_sub_sample(fp, spp, spp_m, k);
        const V3 d = live ? primary_dir(fp, at.px, at.y) : mk(0.0f, 0.0f, 1.0f);
        bool h;
        const V3 acc = path_segments<COUNT, SMOOTH, INT_SHIN, SHADOW, MASK, REFRACT, FRESNEL>(s, p, path, k == 0 ? seg : srt_path_out{}, at.n, at.ri, live, o, d,
                                                                                              __builtin_nanf(""), __builtin_nanf(""), lane, q_all[wave], best_all + wave * 64,
                                                                                              ray_all[wave], at.ray_of, counters, at.shard, h, n_node, n_tri, n_node_s, n_tri_s,
                                                                                              rule, qm, ior, k == 0 ? fr : QueryFresnel{ fr.f0, srt_fresnel_out{} });
        if (k == 0) { total = acc; hit0 = h; }
        else total = mk(total.x + acc.x, total.y + acc.y, total.z + acc.z);
    }
    if (spp > 1) { const float f = (float)spp; total = mk(total.x / f, total.y / f, total.z / f); hit0 = true; }
    if (live) store_pixel(rgb_linear, rgb8, at.ri, total, hit0, p.reinhard, p.gamma, p.bg, 0u);
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_render_path(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryShade p, srt_path_desc path,
                                                     float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                     unsigned long long* __restrict__ counters) {
    render_path_pixels<COUNT, SMOOTH, INT_SHIN, false>(s, fp, spp, spp_m, p, path, rgb_linear, rgb8, seg, counters, ShadowRule{ 0.0f, 0.0f, 0u });
}
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_render_path_shadow(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryShade p, srt_path_desc path,
                                                            float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                            unsigned long long* __restrict__ counters, ShadowRule rule) {
    render_path_pixels<COUNT, SMOOTH, INT_SHIN, true>(s, fp, spp, spp_m, p, path, rgb_linear, rgb8, seg, counters, rule);
}
// srt_render_paths_masked: as k_query_path_masked is k_query_path_shadow's.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_render_path_masked(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryShade p, srt_path_desc path,
                                                            float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                            unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm) {
    render_path_pixels<COUNT, SMOOTH, INT_SHIN, true, true>(s, fp, spp, spp_m, p, path, rgb_linear, rgb8, seg, counters, rule, qm);
}
// srt_render_paths_refract: as k_query_path_refract is k_query_path_masked's.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_render_path_refract(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryShade p, srt_path_desc path,
                                                             float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                             unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm, const float* __restrict__ ior) {
    render_path_pixels<COUNT, SMOOTH, INT_SHIN, true, true, true>(s, fp, spp, spp_m, p, path, rgb_linear, rgb8, seg, counters, rule, qm, ior);
}
// srt_render_paths_fresnel: as k_query_path_fresnel is k_query_path_refract's.  The side rays' rows are sub-sample 0's, as seg's are.
template <bool COUNT, bool SMOOTH, bool INT_SHIN>
__global__ __launch_bounds__(256) void k_render_path_fresnel(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryShade p, srt_path_desc path,
                                                             float* __restrict__ rgb_linear, uint8_t* __restrict__ rgb8, srt_path_out seg,
                                                             unsigned long long* __restrict__ counters, ShadowRule rule, QueryMask qm, const float* __restrict__ ior,
                                                             QueryFresnel fr) {
    render_path_pixels<COUNT, SMOOTH, INT_SHIN, true, true, true, true>(s, fp, spp, spp_m, p, path, rgb_linear, rgb8, seg, counters, rule, qm, ior, fr);
}

// =================================================================================================
// Ambient occlusion in a frame (srt_render_ao, srt_render_ao_hits): k_query_ao's hemisphere visibility for the rays of a frame's own
// pixels, with a rotation of the table chosen by the pixel and the bent normal.  The front end is k_render_path's: a wave owns one 8 x 8
// tile (tile_pixel), the grid is 2-D over the call's local output, a pixel's ray is primary_dir / ray_origin under the call's block or
// tile deal, its row in every output is its local pixel r * W + px; padding pixels and pixels beyond the frame are lanes without a ray,
// which walk nothing and write nothing; the sub-sample loop is wave-uniform.  The back end is k_query_ao's as it stands: query_walk as
// k_query_closest_masked instantiates it with qm.primary (HITS: the caller's hit_id / t, laid out as srt_render_device writes them; no
// queue, one sub-sample), shade_hits_rank, ao_hits_dirs.
// ROT: the pixel's (c, s) is rot[((y % h) * w + x % w) * 2 ..] of its IMAGE pixel, loaded once by the pixel's own lane before the
// sub-sample loop.  The lanes that take a hit's (rank, direction) items find it in two more LDS rows a wave (ao_hits_dirs' wrot): 2 KB a
// workgroup on top of k_query_ao's 10 KB + the queue, two LDS reads an item.  The other way -- one row that names the hit's lane, the
// pixel recovered from it, two integer remainders and an 8-byte gather from the table per item -- saves 1 KB and costs registers for
// the tile's origin and the table's shape inside the item loop, the loop whose any_hit_range walk sets the kernel's register count -- and
// the ROT build of the ray form stands at 127 / 128 VGPRs, the last count at which a SIMD holds four waves (the kernel asks the compiler
// for that occupancy, amdgpu_waves_per_eu: left alone it took 129 / 130 and a SIMD held three, profiles/render_ao_kernels.txt; the COUNT
// builds, 131 .. 138, and the HITS builds, 80 .. 90, are left to it).  The LDS is not what bounds the waves here: 22.5 KB a
// workgroup of four waves is seven workgroups a CU.  Without ROT no arithmetic is applied to the table and the kernel has no such rows.
// bent: the hit's own lane adds, after each chunk and from the chunk's mask, the directions that are not blocked in ascending j --
// ao_ray_dir on the table entry it turns itself, the statements the item's lane ran, so the sum is of the directions as walked.  The
// loop runs only where bent is wanted and costs the lane up to 64 steps a chunk beside the chunk's walks.
// Stores: bent through store_rows_dealt (a tile row's 8 pixels are one 96 B run); occ_bits as ao_hits_dirs stores it, chunk by chunk;
// n_occluded, ao and ao8 by lane.  hit_id, t, n_occluded, occ_bits and bent are sub-sample 0's; ao is the sub-samples' sum in order
// over (float)spp.
// counters: as k_query_ao's, over all sub-samples; the hit shard is the 2-D workgroup number.
// =================================================================================================
struct QueryAoRot { const float* rot; uint32_t w, h; };      // device, h x w x 2 (c, s); read by the ROT builds only

template <bool COUNT, bool SMOOTH, bool HITS, bool ROT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(COUNT || HITS ? 1 : 4)))
void k_render_ao(DevScene s, DevParams fp, uint32_t spp, uint32_t spp_m, QueryMask qm, QueryAo p, QueryAoRot rt, QueryHits given, int32_t* __restrict__ hit_id,
                 float* __restrict__ t_out, srt_ao_frame_out out, unsigned long long* __restrict__ counters) {
    __shared__ unsigned long long best_all[256];
    __shared__ float ray_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    float (*wray)[64] = ray_all[wave];
    float (*wrot)[64] = nullptr;
    if constexpr (ROT) {
        __shared__ float rot_all[4][2][64];
        wrot = rot_all[wave];
    }
    uint32_t* queue = nullptr;
    if constexpr (!HITS) {
        __shared__ uint32_t q_all[4][QCAP];             // the walk's queue: the HITS builds have none
        queue = q_all[wave];
    }
    FramePixel at;
    frame_pixel(at, fp, wave);
    const bool live = at.live;
    const size_t ri = at.ri;
    float c = 1.0f, sn = 0.0f;
    if constexpr (ROT) {
        if (live) {
            const float* e = rt.rot + ((size_t)(at.y % rt.h) * rt.w + image_col(fp, at.px, at.y) % rt.w) * 2;
            c = e[0]; sn = e[1];
        }
    }
    unsigned long long n_node = 0, n_tri = 0, n_node_s = 0, n_tri_s = 0;
    const V3 o = ray_origin(fp);
    const uint32_t n_sub = HITS ? 1u : spp;             // a render's hits are sub-sample 0's
    float total = 0.0f;
    for (uint32_t k = 0; k < n_sub; k++) {                                                          // wave-uniform
        frame_sub_sample(fp, spp, spp_m, k);
        const V3 d = live ? primary_dir(fp, at.px, at.y) : mk(0.0f, 0.0f, 1.0f);
        bool is_hit;
        int32_t id = -1;
        float t = __builtin_inff();
        if constexpr (HITS) {
            if (live) { id = given.hit_id[ri]; t = given.t[ri]; }
            is_hit = id >= 0 && (uint32_t)id < s.n_tris;
        } else {
            query_walk<COUNT, true, MergeClosest, true>(s, live, o, d, lane, queue, MergeClosest{ best }, wray, n_node, n_tri, __builtin_nanf(""), __builtin_nanf(""),
                                                        qm.obj, qm.primary);
            const Winner h = winner_of(live ? best[lane] : ~0ull);
            is_hit = h.is_hit; id = h.id;
        }
        Surface f;
        const WaveHits wh = shade_hits_rank<SMOOTH, true, HITS>(s, is_hit, id, o, d, t, f, wray, p.skip_self ? 0u : 1u);
        if (!HITS && live && k == 0) store_hit(hit_id, t_out, ri, id, t);
        if (p.n_dirs) {                                 // wave-uniform
            const bool want_bent = out.bent && k == 0;  // wave-uniform
            const V3 Nf = ao_facing(d, f.nrm);
            V3 bent = mk(0.0f, 0.0f, 0.0f);
            const auto bent_chunk = [&](const uint32_t l0, const uint32_t m, const unsigned long long mask) {
                if (!want_bent || !is_hit) return;
                for (uint32_t j = 0; j < m; j++) {
                    if ((mask >> j) & 1ull) continue;
                    const float* dp = p.dirs + (size_t)(l0 + j) * 3;
                    float u = dp[0], v = dp[1];
                    const float z = dp[2];
                    if constexpr (ROT) ao_rotate(c, sn, u, v);
                    const V3 wd = ao_ray_dir(Nf, u, v, z);
                    bent = mk(bent.x + wd.x, bent.y + wd.y, bent.z + wd.z);
                }
            };
            const uint32_t blocked = ao_hits_dirs<COUNT, ROT>(s, p, qm, lane, live, is_hit, wh, d, f.nrm, ri, k == 0 ? out.occ_bits : nullptr, wray, best, n_node_s, n_tri_s,
                                                              wrot, c, sn, bent_chunk);
            const float a = (float)(p.n_dirs - blocked) / (float)p.n_dirs;
            if (k == 0) {
                total = a;
                if (out.n_occluded && live) out.n_occluded[ri] = blocked;
                if (want_bent) { const float v[3] = { bent.x, bent.y, bent.z }; store_rows_dealt<3>(out.bent, lane, at.n, v, &wray[0][0], at.ray_of); }
            } else total = total + a;
        }
        if (counters) count_hits(counters, is_hit, at.shard);
    }
    if (p.n_dirs && live) {
        if (n_sub > 1) total = total / (float)spp;
        if (out.ao) out.ao[ri] = total;
        if (out.ao8) out.ao8[ri] = (uint8_t)(int)(total * 255.0f + 0.5f);
    }
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}

// =================================================================================================
// Closest point (srt_closest_points, include/srt_points.h): for a point p with radius r, the triangle nearest to p within r.
// The walk is query_walk as it stands -- the same node records, the same queue of (triangle, owning lane) pairs, the same slices, the same
// (value bits << 32 | id) atomicMin -- with the point's tests: a point-box distance test in the place of slab_pass, Ericson's closest
// point on a triangle in the place of ray_triangle, on the operands load_tri_edges gives the ray test (P1, e1, e2).  The radius is the
// caller's and never shrinks: the candidate set, and with it the counters, are a function of the scene and the point alone
// (why a shrinking radius is not bit-safe: DESIGN.md s5, "Closest point").
// WalkPoint keeps 4 rows a wave: p.xyz and r2.
// =================================================================================================
// Closest point on triangle (P1, P1 + e1, P1 + e2) to p, Real-Time Collision Detection 5.1.5, f32 without contraction.  The regions in
// the header's order, the first true one wins; `region`: 0 face, 1 edge 1-2, 2 edge 2-3, 3 edge 1-3, 4..6 vertex 1..3.  Each of (v, w) is
// one IEEE divide of the winning region's own operands (or a literal): the operands are selected first, so a lane divides twice, not seven
// times; a quotient no region reads may be anything.
struct ClosestPoint { float v, w, dist2; V3 point; uint32_t region; };
__device__ __forceinline__ void closest_point(ClosestPoint& c, const V3 p, const V3 p1, const V3 e1, const V3 e2) {
    const V3 ap = p - p1;
    const float d1 = dot3(e1, ap), d2 = dot3(e2, ap);
    const V3 bp = ap - e1;
    const float d3 = dot3(e1, bp), d4 = dot3(e2, bp);
    const V3 cp = ap - e2;
    const float d5 = dot3(e1, cp), d6 = dot3(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float g = d4 - d3, h = d5 - d6;
    const bool r4 = d1 <= 0.0f && d2 <= 0.0f;
    const bool r5 = d3 >= 0.0f && d4 <= d3;
    const bool r1 = vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f;
    const bool r6 = d6 >= 0.0f && d5 <= d6;
    const bool r3 = vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f;
    const bool r2 = va <= 0.0f && g >= 0.0f && h >= 0.0f;
    const uint32_t region = r4 ? 4u : r5 ? 5u : r1 ? 1u : r6 ? 6u : r3 ? 3u : r2 ? 2u : 0u;
    const float den = (va + vb) + vc;
    // v's divide: edge 1-2 d1 / (d1 - d3), face vb / den;  w's: edge 1-3 d2 / (d2 - d6), edge 2-3 g / (g + h), face vc / den
    const float vn = region == 1u ? d1 : vb, vd = region == 1u ? d1 - d3 : den;
    const float wn = region == 3u ? d2 : region == 2u ? g : vc, wd = region == 3u ? d2 - d6 : region == 2u ? g + h : den;
    const float vq = vn / vd, wq = wn / wd;
    float v, w;
    switch (region) {
        case 4u: v = 0.0f; w = 0.0f; break;
        case 5u: v = 1.0f; w = 0.0f; break;
        case 1u: v = vq; w = 0.0f; break;
        case 6u: v = 0.0f; w = 1.0f; break;
        case 3u: v = 0.0f; w = wq; break;
        case 2u: w = wq; v = 1.0f - w; break;
        default: v = vq; w = wq; break;
    }
    const V3 q = mk(e1.x * v + e2.x * w, e1.y * v + e2.y * w, e1.z * v + e2.z * w);
    const V3 rr = ap - q;
    c.v = v; c.w = w; c.region = region;
    c.dist2 = (rr.x * rr.x + rr.y * rr.y) + rr.z * rr.z;
    c.point = p1 + q;
}

// The point's tests (query_walk's TESTS).  node: the squared distance from p to the box, per axis max(mn - p, p - mx, 0) by the header's two
// comparisons (what a NaN does to them is part of the definition); a node passes iff !(b2 > r2).  leaf: a candidate qualifies iff dist2 <= r2 (a NaN fails); dist2 is a sum of
// squares and never -0, so hit_key's order is (dist2, id) order.
struct WalkPoint {
    V3 p;
    float r2;
    __device__ __forceinline__ void init(float (*rows)[64], const uint32_t lane) const {
        rows[0][lane] = p.x; rows[1][lane] = p.y; rows[2][lane] = p.z; rows[3][lane] = r2;
    }
    static __device__ __forceinline__ float axis(const float mn, const float mx, const float x) {
        const float e = mn - x, f = x - mx;
        const float dx = e > f ? e : f;
        return dx > 0.0f ? dx : 0.0f;
    }
    __device__ __forceinline__ bool node(const float4 a, const float4 b) const {
        const float dx = axis(a.x, a.w, p.x), dy = axis(a.y, b.x, p.y), dz = axis(a.z, b.y, p.z);
        const float b2 = (dx * dx + dy * dy) + dz * dz;
        return !(b2 > r2);
    }
    template <typename Merge>
    __device__ __forceinline__ void leaf(float (*rows)[64], const uint32_t src, const V3 p1, const V3 e1, const V3 e2, const uint32_t tri, const Merge& mg) const {
        ClosestPoint c;
        closest_point(c, mk(rows[0][src], rows[1][src], rows[2][src]), p1, e1, e2);
        if (c.dist2 <= rows[3][src]) mg.offer(src, tri, c.dist2);
    }
};

// k_query_points: one point per lane.  radius NULL: +inf; a point whose radius is negative or NaN walks nothing.  MASK: point i is walked with
// qm.ray[i] (NULL: all ones) against qm.obj, as k_query_closest_masked walks a ray; the build without MASK reads neither.
// Phase 2, as winner_at for rays: the owning lane recomputes the winner's (v, w, region, point, dist2) from the key's triangle and its own p
// -- the walk's function on the walk's operands, hence the walk's bits.  point and vw leave transposed through the wave's rows (store_rows).
// counters: [1] / [2] node / triangle tests (COUNT), [8 + 8 * shard] the points that found a triangle.
// The body is stated once, as SRT_QUERY_POINTS_BODY(TESTS), for this kernel and k_query_nearest below: TESTS is the walk's policy and nothing
// else differs.  (A macro and not a function template: through a function the compiler allocates k_query_points' registers in another
// order, and this file's rule is that a kernel nobody meant to change keeps its bytes -- profiles/nearest_kernels.txt.)
// In it: a NaN radius fails `r >= 0`; once the walk is over the points' rows are the stage of store_rows (the branch is wave-uniform).
// It comes in four pieces -- the wave's LDS with ROWS rows, the point's loads, the walk with the winner recomputed, the stores -- because
// k_query_signed at the end of this file runs the same pieces around its sign rays; the body expands to the tokens it always had.
#define SRT_QUERY_POINTS_LDS(ROWS)                                                                                                                      \
    __shared__ uint32_t q_all[4][QCAP];                                                                                                                 \
    __shared__ unsigned long long best_all[256];                                                                                                        \
    __shared__ float row_all[4][ROWS][64];                                                                                                              \
    const uint32_t lane = wave_lane(), wave = wave_index();                                                                                             \
    unsigned long long* best = best_all + wave * 64;                                                                                                    \
    float (*rows)[64] = row_all[wave];
#define SRT_QUERY_POINTS_LOAD                                                                                                                           \
    const size_t base = wave_base(wave), ri = base + lane;                                                                                              \
    const bool live = ri < (size_t)n_points;                                                                                                            \
    unsigned long long n_node = 0, n_tri = 0;                                                                                                           \
    V3 p = mk(0.0f, 0.0f, 0.0f);                                                                                                                        \
    float r = __builtin_inff();                                                                                                                         \
    uint32_t m = 0xFFFFFFFFu;                                                                                                                           \
    if (live) {                                                                                                                                         \
        const float* pp = points + 3 * ri;                                                                                                              \
        p = mk(pp[0], pp[1], pp[2]);                                                                                                                    \
        if (radius) r = radius[ri];                                                                                                                     \
        if (MASK && qm.ray) m = qm.ray[ri];                                                                                                             \
    }
#define SRT_QUERY_POINTS_FIND(TESTS)                                                                                                                    \
    const bool walks = live && r >= 0.0f;                                                                                                               \
    query_walk<COUNT, false, MergeClosest, MASK>(s, walks, p, p, lane, q_all[wave], MergeClosest{ best }, rows, n_node, n_tri, 0.0f, 0.0f, qm.obj, m, TESTS);\
    const Winner h = winner_of(live ? best[lane] : ~0ull);                                                                                              \
    ClosestPoint c;                                                                                                                                     \
    c.v = 0.0f; c.w = 0.0f; c.dist2 = __builtin_inff(); c.point = mk(0.0f, 0.0f, 0.0f); c.region = 0u;                                                  \
    if (h.is_hit) {                                                                                                                                     \
        V3 p1, e1, e2;                                                                                                                                  \
        load_tri_edges(reinterpret_cast<const float4*>(s.tris), (size_t)h.id, p1, e1, e2);                                                              \
        closest_point(c, p, p1, e1, e2);                                                                                                                \
    }
#define SRT_QUERY_POINTS_STORE                                                                                                                          \
    if (live) {                                                                                                                                         \
        if (out.tri) out.tri[ri] = h.id;                                                                                                                \
        if (out.dist2) out.dist2[ri] = c.dist2;                                                                                                         \
        if (out.region) out.region[ri] = (uint8_t)c.region;                                                                                             \
    }                                                                                                                                                   \
    if (base < (size_t)n_points) {                                                                                                                      \
        const size_t left = (size_t)n_points - base;                                                                                                    \
        const uint32_t live_rows = (uint32_t)(left < 64 ? left : 64);                                                                                   \
        __builtin_amdgcn_wave_barrier();                                                                                                                \
        if (out.point) { const float v[3] = { c.point.x, c.point.y, c.point.z }; store_rows<3>(out.point, base, lane, live_rows, v, &rows[0][0]); }     \
        if (out.vw) { const float v[2] = { c.v, c.w }; store_rows<2>(out.vw, base, lane, live_rows, v, &rows[0][0]); }                                  \
    }
#define SRT_QUERY_POINTS_BODY(TESTS)                                                                                                                    \
    SRT_QUERY_POINTS_LDS(4) SRT_QUERY_POINTS_LOAD SRT_QUERY_POINTS_FIND(TESTS) SRT_QUERY_POINTS_STORE                                                   \
    if (counters) count_hits(counters, h.is_hit, blockIdx.x);                                                                                           \
    count_walks<COUNT>(counters, n_node, n_tri);
template <bool COUNT, bool MASK>
__global__ __launch_bounds__(256) void k_query_points(DevScene s, uint32_t n_points, const float* __restrict__ points, const float* __restrict__ radius,
                                                      srt_point_out out, unsigned long long* __restrict__ counters, QueryMask qm) {
    SRT_QUERY_POINTS_BODY((WalkPoint{ p, r * r }))
}

// =================================================================================================
// Nearest point (srt_nearest_points, include/srt_nearest.h): k_query_points with a bound that shrinks.  The policy is WalkPoint's plus
// one more reason for a node to fail: the header's `low` of the node's box exceeds the best dist2 offered so far for the lane's point.
// That best is the high word of the lane's own best[lane], where MergeClosest keeps (dist2 bits << 32 | id); the initial ~0 reads as a
// NaN and `low > NaN` is false, so "no bound yet" needs no case of its own.  The word moves only when the wave's queue flushes (64 pairs,
// or no lane active), which is query_walk's schedule as it stands -- no statement of query_walk knows about the bound.
// Why the result is k_query_points' bit for bit, and when it is not: the header, and DESIGN.md s5 "Nearest point".
// =================================================================================================
struct WalkNearest {
    WalkPoint pt;
    float mp, zp;                    // of the lane's point: the largest |coordinate|; 0, or NaN if one is not finite
    const uint32_t* bound;           // the wave's best[] as words: [2 * lane + 1] holds the dist2 bits of lane's best
    uint32_t lane;
    static __device__ __forceinline__ WalkNearest make(const V3 p, const float r2, const unsigned long long* best, const uint32_t lane) {
        const float mp = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(p.x), __builtin_fabsf(p.y)), __builtin_fabsf(p.z));
        const float zp = __builtin_fmaf(0.0f, p.z, __builtin_fmaf(0.0f, p.y, 0.0f * p.x));
        return WalkNearest{ WalkPoint{ p, r2 }, mp, zp, reinterpret_cast<const uint32_t*>(best), lane };
    }
    __device__ __forceinline__ float best_of(const uint32_t owner) const {
        return __uint_as_float(__hip_atomic_load(bound + 2 * owner + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT));
    }
    __device__ __forceinline__ void init(float (*rows)[64], const uint32_t l) const { pt.init(rows, l); }
    __device__ __forceinline__ bool node(const float4 a, const float4 b) const {
        const V3 p = pt.p;
        const float dx = WalkPoint::axis(a.x, a.w, p.x), dy = WalkPoint::axis(a.y, b.x, p.y), dz = WalkPoint::axis(a.z, b.y, p.z);
        const float b2 = (dx * dx + dy * dy) + dz * dz;
        if (b2 > pt.r2) return false;
        // the header's low: the box grown by s = K half-ulps of the largest coordinate in play; a NaN or an infinity makes s a NaN and low 0
        float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(a.x), __builtin_fabsf(a.y)), __builtin_fabsf(a.z));
        m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(a.w)), __builtin_fmaxf(__builtin_fabsf(b.x), __builtin_fabsf(b.y)));
        m = __builtin_fmaxf(m, mp);
        float z = __builtin_fmaf(0.0f, a.x, zp);
        z = __builtin_fmaf(0.0f, a.y, z); z = __builtin_fmaf(0.0f, a.z, z); z = __builtin_fmaf(0.0f, a.w, z);
        z = __builtin_fmaf(0.0f, b.x, z); z = __builtin_fmaf(0.0f, b.y, z);
        const float s = __builtin_fmaf((float)SRT_NEAREST_K * 0x1p-24f, m, z);      // (one rounding, of K 2^-24 M: z is 0 or a NaN)
        float tx = dx - s, ty = dy - s, tz = dz - s;
        tx = tx > 0.0f ? tx : 0.0f; ty = ty > 0.0f ? ty : 0.0f; tz = tz > 0.0f ? tz : 0.0f;
        const float low = ((tx * tx + ty * ty) + tz * tz) * (1.0f - 0x1p-20f);
        return !(low > best_of(lane) && low < __builtin_inff());
    }
    // (a candidate above its owner's current best cannot win: the atomicMin is skipped; an equal one goes on, for the lowest id)
    template <typename Merge>
    __device__ __forceinline__ void leaf(float (*rows)[64], const uint32_t src, const V3 p1, const V3 e1, const V3 e2, const uint32_t tri, const Merge& mg) const {
        ClosestPoint c;
        closest_point(c, mk(rows[0][src], rows[1][src], rows[2][src]), p1, e1, e2);
        if (c.dist2 <= rows[3][src] && !(c.dist2 > best_of(src))) mg.offer(src, tri, c.dist2);
    }
};
template <> struct walk_shrinks<WalkNearest> : std::true_type {};
template <bool COUNT, bool MASK>
__global__ __launch_bounds__(256) void k_query_nearest(DevScene s, uint32_t n_points, const float* __restrict__ points, const float* __restrict__ radius,
                                                       srt_point_out out, unsigned long long* __restrict__ counters, QueryMask qm) {
    SRT_QUERY_POINTS_BODY(WalkNearest::make(p, r * r, best, lane))
}
#undef SRT_QUERY_POINTS_BODY

// =================================================================================================
// Signed distance and containment (srt_signed_points, include/srt_signed.h): k_query_nearest's distance, and a sign by winding along
// n_dirs rays from the point.
// Phase 1 (NEAR) is k_query_nearest's body, piece by piece: WalkNearest, MergeClosest, the winner recomputed from the key, the stores.  The
// host picks NEAR = false when neither a field of the point outputs nor sdist is wanted: containment for the price of the ray walks.
// Phase 2: the table (the caller's, or the header's default) goes into LDS once per workgroup; for every direction j the wave's 64 rays
// (p, dirs[j]) are ONE query_walk -- every live lane is busy, neighbouring points share a direction, nothing is compacted or dealt.  The
// walk is the ray's with another leaf: WalkCross keeps (o, d) in 6 rows as WalkRay does, tests a node with slab_pass<true> on the lane's
// own ray_rcp, and a leaf with ray_triangle on the OWNER's ray; a candidate that counts by the closest hit's rule offers the sign of its
// det.  MergeCross keeps two words a lane -- entries, exits -- in the 8 bytes that held phase 1's key, added to by whichever lane tested
// the pair.  A point whose radius walks nothing in phase 1 still gets its rays.
// LDS a workgroup: the queue 10,240 B, the keys / counts 2,048 B, 6 rows 6,144 B (phase 1 uses 4 of them, and 3 as its stage), the table
// 192 B: 18,624 B, eight workgroups a CU, which the registers do not reach.
// counters: [1] / [2] phase 1 as k_query_nearest counts it, [3] / [4] node / triangle tests of the sign rays, [8 + 8 * shard] the points
// that found a triangle.
// =================================================================================================
__constant__ float sign_default_dirs[9] = SRT_SIGN_DEFAULT_DIRS;
struct QuerySign { const float* dirs; uint32_t n_dirs, parity; };      // dirs NULL: sign_default_dirs (n_dirs is 3 then)
struct MergeCross {
    uint32_t* cnt;                // 2 x 64 words: [2 * lane] entries, [2 * lane + 1] exits of the lane's ray
    __device__ __forceinline__ void init(const uint32_t lane) const { cnt[2 * lane] = 0u; cnt[2 * lane + 1] = 0u; }
    __device__ __forceinline__ void offer(const uint32_t src, const uint32_t, const float det) const { atomicAdd(&cnt[2 * src + (det < 0.0f ? 1u : 0u)], 1u); }
};
struct WalkCross {
    V3 o, d;
    RayRcp rc;
    __device__ __forceinline__ void init(float (*rows)[64], const uint32_t lane) const {
        rows[0][lane] = o.x; rows[1][lane] = o.y; rows[2][lane] = o.z;
        rows[3][lane] = d.x; rows[4][lane] = d.y; rows[5][lane] = d.z;
    }
    __device__ __forceinline__ bool node(const float4 a, const float4 b) const { return slab_pass<true>(o, d, rc, a.x, a.y, a.z, a.w, b.x, b.y); }
    template <typename Merge>
    __device__ __forceinline__ void leaf(float (*rows)[64], const uint32_t src, const V3 p1, const V3 e1, const V3 e2, const uint32_t tri, const Merge& mg) const {
        const V3 os = mk(rows[0][src], rows[1][src], rows[2][src]), ds = mk(rows[3][src], rows[4][src], rows[5][src]);
        const float t = ray_triangle(os, ds, p1, e1, e2);
        // counts iff t != -inf && t < +inf (the closest hit's rule); then |det| >= 1e-12: an entry (det > 0) or an exit (det < 0)
        if (t != SRT_NEG_INF && t < __builtin_inff()) mg.offer(src, tri, dot3(e1, cross3(ds, e2)));
    }
};
template <bool COUNT, bool MASK, bool NEAR>
__global__ __launch_bounds__(256) void k_query_signed(DevScene s, uint32_t n_points, const float* __restrict__ points, const float* __restrict__ radius,
                                                      srt_point_out out, srt_sign_out sout, QuerySign sg, unsigned long long* __restrict__ counters, QueryMask qm) {
    __shared__ float dir_tab[SRT_SIGN_MAX_DIRS * 3];
    SRT_QUERY_POINTS_LDS(6)
    if (threadIdx.x < 3u * sg.n_dirs) dir_tab[threadIdx.x] = sg.dirs ? sg.dirs[threadIdx.x] : sign_default_dirs[threadIdx.x];
    __syncthreads();
    SRT_QUERY_POINTS_LOAD
    bool found = false;
    float dist2 = __builtin_inff();
    if constexpr (NEAR) {
        SRT_QUERY_POINTS_FIND(WalkNearest::make(p, r * r, best, lane))
        SRT_QUERY_POINTS_STORE
        found = h.is_hit; dist2 = c.dist2;
        __builtin_amdgcn_wave_barrier();              // every lane has read its key: the 8 bytes are the counts' now
    }
    unsigned long long n_node_s = 0, n_tri_s = 0;
    uint32_t* cnt = reinterpret_cast<uint32_t*>(best);
    uint32_t votes = 0;
    for (uint32_t j = 0; j < sg.n_dirs; j++) {        // wave-uniform
        const V3 d = mk(dir_tab[3 * j], dir_tab[3 * j + 1], dir_tab[3 * j + 2]);
        query_walk<COUNT, false, MergeCross, MASK>(s, live, p, d, lane, q_all[wave], MergeCross{ cnt }, rows, n_node_s, n_tri_s, 0.0f, 0.0f, qm.obj, m,
                                                   WalkCross{ p, d, ray_rcp(p, d) });
        const uint32_t entries = cnt[2 * lane], exits = cnt[2 * lane + 1];
        const int32_t winding = (int32_t)exits - (int32_t)entries;
        const uint32_t crossings = exits + entries;
        votes += sg.parity ? (crossings & 1u) : (winding > 0 ? 1u : 0u);
        if (live) {
            if (sout.winding) sout.winding[ri * sg.n_dirs + j] = winding;
            if (sout.crossings) sout.crossings[ri * sg.n_dirs + j] = crossings;
        }
        __builtin_amdgcn_wave_barrier();              // (the next direction clears the counts)
    }
    const bool inside = 2u * votes > sg.n_dirs;
    if (live) {
        if (sout.inside) sout.inside[ri] = inside ? 1 : 0;
        if (NEAR && sout.sdist) sout.sdist[ri] = inside ? -sqrtf(dist2) : sqrtf(dist2);
    }
    if (counters) count_hits(counters, found, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri, n_node_s, n_tri_s);
}
#undef SRT_QUERY_POINTS_LDS
#undef SRT_QUERY_POINTS_LOAD
#undef SRT_QUERY_POINTS_FIND
#undef SRT_QUERY_POINTS_STORE

// =================================================================================================
// The K nearest triangles of a point (srt_closest_points_multi, srt_nearest_points_multi; include/srt_points_multi.h): the two halves
// that existed, put together -- the point's policies (WalkPoint, WalkNearest) with srt_trace_rays_multi's merge (MergeMulti: k slots of 64
// keys a wave, a key carried down them by atomicMin).  hit_key(dist2, id) orders candidates by (dist2, id): dist2 is never -0.  Nothing of
// query_walk, the policies or the merge changes; cnt[] counts the offers, which in the closest form are ALL qualifying candidates.
// NEAR: WalkNearest as it stands with its `bound` on the wave's slot[k - 1] in the place of best[]: the high word of slot[k - 1][lane] is
// the k-th best dist2 offered so far for the lane's point.  An empty slot's ~0 reads as a NaN -- "no bound yet", as there.  The slot is
// written by atomicMin alone, so it only decreases, and MergeMulti's induction makes its FINAL value the k-th smallest key offered: any
// value read from it on the way is never below the final k-th dist2, so by (a) and (c) of include/srt_nearest.h no ancestor of any of the
// k winners is pruned, and the leaf filter !(dist2 > best_of(src)) drops only what cannot be among the k.  cnt[] counts the offers that
// passed that filter and means nothing to a caller: the kernel argument n_within is NULL in this form (the host refuses it).
// Phase 2: column by column the owning lane recomputes closest_point from the key's triangle and its own p -- the walk's function on the
// walk's operands, hence the walk's bits -- and stores that column's point, vw and region itself (rows of 12, 8 and 1 B at a stride of k
// rows: a per-column store_rows would need the stage k times for runs of 3 words; the bits do not depend on it).  tri and dist2 leave
// TRANSPOSED through the slots, as k_query_multi's hit_id and t do: 64 consecutive words per store.  n_within and n_found, one word a
// point, are coalesced as they stand; n_found is the number of filled slots, min(k, offers) in both forms.
// KB: the slots the build reserves (k <= KB; the host picks 4, 8 or 16).  LDS a workgroup: the queue 10,240 B, the slots KB x 2,048 B,
// the counts 1,024 B, 4 rows 4,096 B: 23,552 / 31,744 / 48,128 B -- six, five and three workgroups a CU of 160 KB.
// counters: [1] / [2] node / triangle tests (COUNT), [8 + 8 * shard] the points with n_found > 0.
// =================================================================================================
template <bool COUNT, bool MASK, bool NEAR, int KB>
__global__ __launch_bounds__(256) void k_query_points_multi(DevScene s, uint32_t n_points, const float* __restrict__ points, const float* __restrict__ radius,
                                                            uint32_t k, srt_point_multi_out out, unsigned long long* __restrict__ counters, QueryMask qm) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long slot_all[4][KB][64];
    __shared__ uint32_t cnt_all[256];
    __shared__ float row_all[4][4][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long (*slot)[64] = slot_all[wave];
    uint32_t* cnt = cnt_all + wave * 64;
    k = k < 1u ? 1u : k < (uint32_t)KB ? k : (uint32_t)KB;      // (the host picks KB >= k >= 1)
    const size_t base = wave_base(wave), ri = base + lane;
    const bool live = ri < (size_t)n_points;
    unsigned long long n_node = 0, n_tri = 0;
    V3 p = mk(0.0f, 0.0f, 0.0f);
    float r = __builtin_inff();
    uint32_t m = 0xFFFFFFFFu;
    if (live) {
        const float* pp = points + 3 * ri;
        p = mk(pp[0], pp[1], pp[2]);
        if (radius) r = radius[ri];
        if (MASK && qm.ray) m = qm.ray[ri];
    }
    const bool walks = live && r >= 0.0f;               // (a NaN radius fails the comparison)
    const MergeMulti mg{ slot, cnt, k };
    if constexpr (NEAR)
        query_walk<COUNT, false, MergeMulti, MASK>(s, walks, p, p, lane, q_all[wave], mg, row_all[wave], n_node, n_tri, 0.0f, 0.0f, qm.obj, m,
                                                   WalkNearest::make(p, r * r, slot[k - 1], lane));
    else
        query_walk<COUNT, false, MergeMulti, MASK>(s, walks, p, p, lane, q_all[wave], mg, row_all[wave], n_node, n_tri, 0.0f, 0.0f, qm.obj, m,
                                                   WalkPoint{ p, r * r });
    const float4* tris4 = reinterpret_cast<const float4*>(s.tris);
    const bool found = live && slot[0][lane] != ~0ull;
    if (live) {
        if (!NEAR && out.n_within) out.n_within[ri] = cnt[lane];
        if (out.n_found) {
            uint32_t nf = 0;
            for (uint32_t j = 0; j < k; j++) nf += slot[j][lane] != ~0ull ? 1u : 0u;
            out.n_found[ri] = nf;
        }
    }
    if (out.tri || out.dist2 || out.point || out.vw || out.region) {      // (wave-uniform: a kernel argument)
        for (uint32_t j = 0; j < k; j++) {
            const Winner h = winner_of(live ? slot[j][lane] : ~0ull);
            ClosestPoint c;
            c.v = 0.0f; c.w = 0.0f; c.dist2 = __builtin_inff(); c.point = mk(0.0f, 0.0f, 0.0f); c.region = 0u;
            if (h.is_hit) {
                V3 p1, e1, e2;
                load_tri_edges(tris4, (size_t)h.id, p1, e1, e2);
                closest_point(c, p, p1, e1, e2);          // (dist2, point, vw and region of THIS triangle)
            }
            if (live) {
                const size_t at = ri * k + j;
                if (out.region) out.region[at] = (uint8_t)c.region;
                if (out.point) { out.point[at * 3] = c.point.x; out.point[at * 3 + 1] = c.point.y; out.point[at * 3 + 2] = c.point.z; }
                if (out.vw) { out.vw[at * 2] = c.v; out.vw[at * 2 + 1] = c.w; }
            }
            slot[j][lane] = ((unsigned long long)__float_as_uint(c.dist2) << 32) | (uint32_t)h.id;
        }
        __builtin_amdgcn_wave_barrier();
        if (base < (size_t)n_points && (out.tri || out.dist2)) {      // wave-uniform
            const size_t left = (size_t)n_points - base;
            const uint32_t words = (uint32_t)(left < 64 ? left : 64) * k;      // the wave's rows are words [base * k, base * k + words)
            for (uint32_t w = lane; w < words; w += 64u) {
                const uint32_t row = w / k, j = w - row * k;
                const unsigned long long v = slot[j][row];
                if (out.tri) out.tri[base * k + w] = (int32_t)(uint32_t)v;
                if (out.dist2) out.dist2[base * k + w] = __uint_as_float((uint32_t)(v >> 32));
            }
        }
    }
    if (counters) count_hits(counters, found, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri);
}

// =================================================================================================
// Segment queries (srt_closest_segments, include/srt_segments.h): for a segment A-B with radius r, the triangle nearest to it within r.
// query_walk as it stands with a policy that carries a segment: WalkSegment keeps 7 rows a wave -- A, B and r2 (8 allocated); d = B - A
// is recomputed from the rows by whichever lane tests a pair, the owner's subtraction on the owner's operands, so every lane has the
// owner's d AND the owner's B with their own bits.  The reciprocals, r and the sloped flag of box test 2 are read by node() alone and
// stay in the owning lane's registers.  The radius never shrinks: candidates and counters are a function of the scene and the segment.
// =================================================================================================
// The header's triangle function.  The five candidates are a RUNNING minimum -- (dist2, s, v, w, feature), one candidate live at a time:
// the two ends through closest_point, the three edges through one loop that is not unrolled (origin and dir are selected by the edge's
// number), so the leaf holds one closest_point and one edge body in registers, not five results.  The crossing overrides them.
// FULL = false is the walk's leaf, which offers dist2 alone: a crossing is +0 without its closest_point, and everything but dist2 is dead.
struct SegmentHit { float dist2, s, v, w; uint32_t feature; };
__device__ __forceinline__ float clamp01(const float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }
template <bool FULL>
__device__ __forceinline__ void segment_triangle(SegmentHit& h, const V3 A, const V3 B, const V3 p1, const V3 e1, const V3 e2) {
    const V3 d = B - A;
    ClosestPoint c;
    closest_point(c, A, p1, e1, e2);
    h.dist2 = c.dist2; h.s = 0.0f; h.v = c.v; h.w = c.w; h.feature = 0u;
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return;      // a point: candidate 0 only
    const float t = ray_triangle(A, d, p1, e1, e2);
    if (t != SRT_NEG_INF && t >= 0.0f && t <= 1.0f) {
        h.dist2 = 0.0f; h.s = t; h.feature = 5u;
        if (FULL) { closest_point(c, A + d * t, p1, e1, e2); h.v = c.v; h.w = c.w; }
        return;
    }
    closest_point(c, B, p1, e1, e2);
    if (c.dist2 < h.dist2 || (h.dist2 != h.dist2 && c.dist2 == c.dist2)) { h.dist2 = c.dist2; h.s = 1.0f; h.v = c.v; h.w = c.w; h.feature = 1u; }
    const float a = dot3(d, d);
    #pragma nounroll
    for (uint32_t k = 0; k < 3u; k++) {
        const V3 origin = k == 1u ? p1 + e1 : p1;
        const V3 dir = k == 0u ? e1 : k == 1u ? e2 - e1 : e2;
        const V3 rr = A - origin;
        const float e = dot3(dir, dir), f = dot3(dir, rr), cc = dot3(d, rr), b = dot3(d, dir);
        float s = 0.0f, u = 0.0f, num = -cc;
        bool again = true;                              // s = clamp(num / a), the divide of whichever case asks for it
        if (e != 0.0f) {
            const float den = a * e - b * b;
            s = den > 0.0f ? clamp01((b * f - cc * e) / den) : 0.0f;
            u = (b * s + f) / e;
            again = false;
            if (u < 0.0f) { u = 0.0f; again = true; }
            else if (u > 1.0f) { u = 1.0f; num = b - cc; again = true; }
        }
        if (again) s = clamp01(num / a);
        const V3 x = (A + d * s) - (origin + dir * u);
        const float d2 = dot3(x, x);
        if (d2 < h.dist2 || (h.dist2 != h.dist2 && d2 == d2)) {
            h.dist2 = d2; h.s = s; h.feature = 2u + k;
            h.v = k == 0u ? u : k == 1u ? 1.0f - u : 0.0f;
            h.w = k == 0u ? 0.0f : u;
        }
    }
}

// The segment's tests (query_walk's TESTS).  node: the header's box test 1 -- for a point WalkPoint::axis, operation for operation -- and,
// for a sloped segment with a finite radius, box test 2.  leaf: the triangle qualifies iff its result's dist2 <= r2 (a NaN fails); dist2
// is a sum of squares or the crossing's +0 and never -0, so hit_key's order is (dist2, id) order.
struct WalkSegment {
    V3 A, B;
    float r, r2;
    V3 inv;                          // 1 / d per axis; read only when slab
    bool slab;                       // the segment is sloped and r < +inf: box test 2 applies
    static __device__ __forceinline__ bool finite(const float x) { return __builtin_fabsf(x) < __builtin_inff(); }
    static __device__ __forceinline__ WalkSegment make(const V3 A, const V3 B, const float r) {
        const V3 d = B - A;
        const V3 inv = mk(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
        const bool sloped = finite(d.x) && finite(d.y) && finite(d.z) && d.x != 0.0f && d.y != 0.0f && d.z != 0.0f && finite(inv.x) && finite(inv.y) && finite(inv.z);
        return WalkSegment{ A, B, r, r * r, inv, sloped && r < __builtin_inff() };
    }
    __device__ __forceinline__ void init(float (*rows)[64], const uint32_t lane) const {
        rows[0][lane] = A.x; rows[1][lane] = A.y; rows[2][lane] = A.z;
        rows[3][lane] = B.x; rows[4][lane] = B.y; rows[5][lane] = B.z; rows[6][lane] = r2;
    }
    static __device__ __forceinline__ float gap(const float mn, const float mx, const float a, const float b) {
        const float lo = a < b ? a : b, hi = a < b ? b : a;
        const float e = mn - hi, f = lo - mx;
        const float g = e > f ? e : f;
        return g > 0.0f ? g : 0.0f;
    }
    __device__ __forceinline__ bool node(const float4 a, const float4 b) const {
        const float gx = gap(a.x, a.w, A.x, B.x), gy = gap(a.y, b.x, A.y, B.y), gz = gap(a.z, b.y, A.z, B.z);
        const float b2 = (gx * gx + gy * gy) + gz * gz;
        if (b2 > r2) return false;
#ifdef SRT_SEGMENTS_NO_BOX_TEST_2
        return true;                                    // (a measurement build: what box test 2 buys, tools/ray_query_probe.py --segments)
#endif
        if (!slab) return true;
        const float x0 = ((a.x - r) - A.x) * inv.x, x1 = ((a.w + r) - A.x) * inv.x;
        const float y0 = ((a.y - r) - A.y) * inv.y, y1 = ((b.x + r) - A.y) * inv.y;
        const float z0 = ((a.z - r) - A.z) * inv.z, z1 = ((b.y + r) - A.z) * inv.z;
        const float xn = x0 < x1 ? x0 : x1, xf = x0 < x1 ? x1 : x0;
        const float yn = y0 < y1 ? y0 : y1, yf = y0 < y1 ? y1 : y0;
        const float zn = z0 < z1 ? z0 : z1, zf = z0 < z1 ? z1 : z0;
        float near = 0.0f, far = 1.0f;
        near = xn > near ? xn : near; near = yn > near ? yn : near; near = zn > near ? zn : near;
        far = xf < far ? xf : far; far = yf < far ? yf : far; far = zf < far ? zf : far;
        const bool nan = __builtin_isunordered(x0, x1) || __builtin_isunordered(y0, y1) || __builtin_isunordered(z0, z1);
        return !(near > far) || nan;
    }
    template <typename Merge>
    __device__ __forceinline__ void leaf(float (*rows)[64], const uint32_t src, const V3 p1, const V3 e1, const V3 e2, const uint32_t tri, const Merge& mg) const {
        SegmentHit h;
        segment_triangle<false>(h, mk(rows[0][src], rows[1][src], rows[2][src]), mk(rows[3][src], rows[4][src], rows[5][src]), p1, e1, e2);
        if (h.dist2 <= rows[6][src]) mg.offer(src, tri, h.dist2);
    }
};

// k_query_segments: one segment per lane, k_query_points' shape.  radius NULL: +inf; a segment whose radius is negative or NaN walks
// nothing.  MASK: segment i is walked with qm.ray[i] (NULL: all ones) against qm.obj; the build without MASK reads neither.
// Phase 2, as k_query_points': the owning lane recomputes the winner's (dist2, s, v, w, feature) from the key's triangle and its own A
// and B -- the walk's function on the walk's operands, hence the walk's bits -- and point = P1 + (e1 v + e2 w).  point and vw leave
// transposed through the wave's rows (store_rows), which are free once the walk is over.
// LDS a workgroup: the queue 10,240 B, the keys 2,048 B, 8 rows 8,192 B: 20,480 B.
// counters: [1] / [2] node / triangle tests (COUNT), [8 + 8 * shard] the segments that found a triangle.
template <bool COUNT, bool MASK>
__global__ __launch_bounds__(256) void k_query_segments(DevScene s, uint32_t n_segments, const float* __restrict__ segments, const float* __restrict__ radius,
                                                        srt_segment_out out, unsigned long long* __restrict__ counters, QueryMask qm) {
    __shared__ uint32_t q_all[4][QCAP];
    __shared__ unsigned long long best_all[256];
    __shared__ float row_all[4][8][64];
    const uint32_t lane = wave_lane(), wave = wave_index();
    unsigned long long* best = best_all + wave * 64;
    float (*rows)[64] = row_all[wave];
    const size_t base = wave_base(wave), ri = base + lane;
    const bool live = ri < (size_t)n_segments;
    unsigned long long n_node = 0, n_tri = 0;
    V3 A = mk(0.0f, 0.0f, 0.0f), B = A;
    float r = __builtin_inff();
    uint32_t m = 0xFFFFFFFFu;
    if (live) {
        const float* sp = segments + 6 * ri;
        A = mk(sp[0], sp[1], sp[2]); B = mk(sp[3], sp[4], sp[5]);
        if (radius) r = radius[ri];
        if (MASK && qm.ray) m = qm.ray[ri];
    }
    const bool walks = live && r >= 0.0f;               // (a NaN radius fails the comparison)
    query_walk<COUNT, false, MergeClosest, MASK>(s, walks, A, A, lane, q_all[wave], MergeClosest{ best }, rows, n_node, n_tri, 0.0f, 0.0f, qm.obj, m,
                                                 WalkSegment::make(A, B, r));
    const Winner h = winner_of(live ? best[lane] : ~0ull);
    SegmentHit c;
    c.dist2 = __builtin_inff(); c.s = 0.0f; c.v = 0.0f; c.w = 0.0f; c.feature = 0u;
    V3 pt = mk(0.0f, 0.0f, 0.0f);
    if (h.is_hit) {
        V3 p1, e1, e2;
        load_tri_edges(reinterpret_cast<const float4*>(s.tris), (size_t)h.id, p1, e1, e2);
        segment_triangle<true>(c, A, B, p1, e1, e2);
        pt = p1 + mk(e1.x * c.v + e2.x * c.w, e1.y * c.v + e2.y * c.w, e1.z * c.v + e2.z * c.w);
    }
    if (live) {
        if (out.tri) out.tri[ri] = h.id;
        if (out.dist2) out.dist2[ri] = c.dist2;
        if (out.s) out.s[ri] = c.s;
        if (out.feature) out.feature[ri] = (uint8_t)c.feature;
    }
    if (base < (size_t)n_segments) {                    // wave-uniform
        const size_t left = (size_t)n_segments - base;
        const uint32_t live_rows = (uint32_t)(left < 64 ? left : 64);
        __builtin_amdgcn_wave_barrier();
        if (out.point) { const float v[3] = { pt.x, pt.y, pt.z }; store_rows<3>(out.point, base, lane, live_rows, v, &rows[0][0]); }
        if (out.vw) { const float v[2] = { c.v, c.w }; store_rows<2>(out.vw, base, lane, live_rows, v, &rows[0][0]); }
    }
    if (counters) count_hits(counters, h.is_hit, blockIdx.x);
    count_walks<COUNT>(counters, n_node, n_tri);
}
