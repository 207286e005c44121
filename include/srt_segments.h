/* include/srt_segments.h -- segment queries: the nearest triangle to a SEGMENT within a radius, and where the two come closest.
 *
 * An extension header of include/srt.h, which includes it at its end, after include/srt_points_multi.h; it may be included on its own.
 * Same conventions: plain C, PODs, caller-owned buffers, int return codes; the handle, srt_stats, the flags and the error codes are srt.h's.
 * SRT_ABI_VERSION stays 3: nothing that existed changes.
 */
#ifndef SRT_SEGMENTS_H
#define SRT_SEGMENTS_H

#include "srt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The point calls (srt_points.h) answer "how far is this POINT from the geometry", the ray calls "what does this LINE hit".  A segment
 * with a radius -- a capsule -- lies between them: a particle of thickness r that moves from A to B in a step (a point query at B misses
 * a sheet the step jumped over, a ray from A to B misses a near miss), a cloth edge or a bone with a radius against a posed mesh, a line
 * of sight with a width.  Segment i is the six floats A, B; its result is the triangle nearest to it within r, the parameter s of the
 * segment's closest point A + (B - A) * s, the closest point ON THE TRIANGLE and which feature gave it.
 * Unless said here everything is as srt_points.h says for srt_closest_points: flags are 0 or SRT_FLAG_COUNT_WORK, the ordering on
 * `stream`, srt_scene_share, srt_scene_pose, srt_scene_refit_device, the private counter set, ONE launch with nothing allocated and
 * nothing copied, hipGraph capture of the _device form without SRT_FLAG_COUNT_WORK.
 * DEFINITION.  All arithmetic is f32 without contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; divides are IEEE divides; a vector
 * expression is evaluated per component; clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x) (a NaN stays a NaN).
 *   Operands    d = B - A.  r = radius[i], a NULL array means +inf; r2 = r * r.  A segment whose r is negative or NaN finds nothing and
 *               walks nothing (-0 is not negative).  The segment is a POINT iff d.x == 0 && d.y == 0 && d.z == 0.
 *   Box test 1  always: the gap between the segment's own box and the node's box (mn, mx).  Per axis, with a and b that component of A and B:
 *                   lo = a < b ? a : b    hi = a < b ? b : a    e = mn - hi    f = lo - mx    g = e > f ? e : f    g = g > 0 ? g : 0
 *               b2 = (gx*gx + gy*gy) + gz*gz, and the node FAILS iff b2 > r2.  For a point this is srt_points.h's box test, operation
 *               for operation.
 *   Box test 2  only for a SLOPED segment with r < +inf.  Sloped: for every axis d_k is finite and not 0 and inv_k = 1.0f / d_k is finite.
 *               The slab test of the segment over [0, 1] against the box grown by r.  Per axis:
 *                   t0 = ((mn - r) - a) * inv    t1 = ((mx + r) - a) * inv    tn = t0 < t1 ? t0 : t1    tf = t0 < t1 ? t1 : t0
 *               near = 0.0f, then for x, y, z in turn near = tn > near ? tn : near;  far = 1.0f, then far = tf < far ? tf : far.
 *               The node FAILS iff near > far and none of the six t0, t1 is a NaN.  A node passes iff it fails neither test.
 *               Why it may be applied: every point within r of the box lies in the box grown by r per axis, so a segment that comes
 *               within r of anything in the box meets the grown box; the test is conservative by the corners' r * (sqrt(3) - 1).
 *               Without it a long diagonal segment walks its whole bounding box.
 *   Candidates  the triangles of every leaf whose ancestors and itself all pass.  The radius NEVER SHRINKS: the candidate set, and under
 *               SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary, are a function of the scene and the segment alone (a leaf
 *               taken in slices counts once).
 *   Triangle    on the record's operands P1, e1, e2.  Five candidates, each (dist2, s, v, w), and the crossing:
 *               0  end A   srt_points.h's closest point of p = A: its v, w and dist2, with s = 0.
 *               1  end B   the same of p = B, with s = 1.
 *               2, 3, 4    the segment against the edge (origin, dir) = (P1, e1), (P1 + e1, e2 - e1), (P1, e2) -- edge 1-2, 2-3, 1-3 --
 *                          by Real-Time Collision Detection 5.1.9:
 *                              rr = A - origin   a = dot(d, d)   e = dot(dir, dir)   f = dot(dir, rr)   c = dot(d, rr)   b = dot(d, dir)
 *                              if e == 0:   u = 0, s = clamp((-c) / a)
 *                              otherwise    den = a*e - b*b
 *                                           s = den > 0 ? clamp((b*f - c*e) / den) : 0
 *                                           u = (b*s + f) / e
 *                                           if u < 0:        u = 0, s = clamp((-c) / a)
 *                                           else if u > 1:   u = 1, s = clamp((b - c) / a)
 *                          (v, w) = (u, 0), (1 - u, u), (0, u) for the three edges;
 *                          x = (A + d*s) - (origin + dir*u), dist2 = (x.x*x.x + x.y*x.y) + x.z*x.z.
 *               The result starts as candidate 0, whatever its dist2.  Candidates 1 .. 4 in turn replace it iff
 *                   dist2_k < dist2 || (dist2 != dist2 && dist2_k == dist2_k)
 *               -- the minimum, equal values to the lowest candidate number; a NaN never replaces anything and is replaced by any number.
 *               `feature` is the number of the candidate that gave the result.
 *               5  crossing   t = the ray queries' triangle test (srt.h) of the ray (A, d).  The segment crosses iff
 *                          t != -inf && t >= 0 && t <= 1.  Then the result is s = t, dist2 = +0, (v, w) = those of srt_points.h's closest
 *                          point of p = A + d*t, feature 5, whatever the candidates gave.
 *               A POINT segment has candidate 0 only: s = 0, feature 0, no crossing.
 *               In every case point = P1 + (e1*v + e2*w) -- for candidates 0, 1 and 5 that IS the closest point's `point`.
 *   Qualifies   the triangle qualifies iff the result's dist2 <= r2 (closed; a NaN fails).
 *   The winner  the minimum dist2 among the qualifying triangles, equal dist2 to the lowest triangle id (dist2 is never -0).  None:
 *               tri -1, dist2 +inf, s 0, point (0, 0, 0), vw (0, 0), feature 0.  Results never depend on the order of the segments in a call.
 * AT THE RADIUS.  The candidate set is OPERATIONAL: what the two box tests pass, in f32.  A triangle whose computed dist2 lies within a few
 * ulps of r2 may sit in a leaf whose box fails by as little (e1 and e2 are rounded differences; srt_points.h, WHY NO SHRINKING RADIUS), so
 * at the boundary "within r" means "found by this walk"; a triangle with dist2 <= r2 * (1 - 2^-10) was never lost on the scenes tested.
 * CONSEQUENCES.  A point segment returns srt_closest_points' tri, dist2, point, vw and both counters bit for bit.  A crossing's tri is
 * among srt_trace_rays_range's candidates of the ray (A, d) in (0, 1).
 * MASKS.  seg_mask: n words, or NULL = all ones, with the semantics of srt_points.h's point_mask; a NULL seg_mask launches the build that
 * never reads the scene's table.
 * Segments are n x 6 floats at any float alignment, read with 4-byte loads; nothing past the last segment is read.
 * Errors, before anything is touched: SRT_ERR_ARG for a NULL handle, a NULL `out`, NULL segments with n > 0, any flag bit but
 * SRT_FLAG_COUNT_WORK.  n == 0: SRT_OK with nothing done.  Every field of *out NULL in the _device form: SRT_OK, nothing launched.
 * The host form stages segments, radius, seg_mask and the outputs through the handle's pinned block, then waits.  *stats: primary_rays = n,
 * hit_rays = the segments that found a triangle, node_tests_primary / tri_tests_primary under SRT_FLAG_COUNT_WORK.
 * NOT HERE: a shrinking bound (the form srt_nearest.h is to srt_points.h); the K nearest triangles of a segment; a time of FIRST contact
 * of the swept sphere -- s is where the path comes closest, or where it crosses. */
typedef struct srt_segment_out {   /* device pointers in the _device form, host pointers in the host form; any may be NULL */
    int32_t* tri;      /* n      canonical triangle id, -1 = none within the radius */
    float*   dist2;    /* n      the winner's dist2, +0 for a crossing, +inf = none */
    float*   s;        /* n      where on the segment: closest point = A + (B - A) * s, 0 <= s <= 1 */
    float*   point;    /* n x 3  the closest point ON THE TRIANGLE */
    float*   vw;       /* n x 2  its (v, w) on the triangle */
    uint8_t* feature;  /* n      0 end A, 1 end B, 2 / 3 / 4 triangle edge 1-2 / 2-3 / 1-3, 5 the segment crosses the triangle */
} srt_segment_out;
int srt_closest_segments_device(srt_scene* s, uint32_t n, const float* d_segments /* n x 6: A, B */, const float* d_radius /* n or NULL = +inf */,
                                const uint32_t* d_seg_mask /* n or NULL */, uint32_t flags, void* stream, const srt_segment_out* out);
int srt_closest_segments(srt_scene* s, uint32_t n, const float* segments, const float* radius, const uint32_t* seg_mask, uint32_t flags,
                         const srt_segment_out* out, srt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SRT_SEGMENTS_H */
