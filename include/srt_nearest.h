/* include/srt_nearest.h -- the nearest triangle per point WITHOUT a radius to choose: srt_closest_points with a bound that shrinks.
 *
 * An extension header of include/srt.h, which includes it at its end, after include/srt_points.h; it may be included on its own.  Same
 * conventions; srt_point_out, the handle, srt_stats, the flags and the error codes are theirs.  SRT_ABI_VERSION stays 3.
 */
#ifndef SRT_NEAREST_H
#define SRT_NEAREST_H

#include "srt_points.h"

#ifdef __cplusplus
extern "C" {
#endif

/* srt_nearest_points is srt_closest_points (include/srt_points.h) -- its arguments, its radius (NULL = +inf), its masks, its srt_point_out, its
 * errors, n == 0, all-NULL `out`, stats fields, stream ordering, shared handles, ONE launch, hipGraph capture of the _device form without
 * SRT_FLAG_COUNT_WORK -- with one difference: during the walk a point also prunes by the best dist2 found so far for it.  A caller who does
 * not know the distance in advance passes no radius and pays for the neighbourhood of the answer, not for the scene.
 * CONTRACT.  Every output is bit for bit what srt_closest_points gives for the same scene, point, radius and mask, on every scene that
 * meets the two PRECONDITIONS below.
 * DEFINITION.  Box test, Triangle, Qualifies and The winner are srt_points.h's, operation by operation.  In addition:
 *   1. The caller's radius test is unchanged and has no margin: a node fails iff b2 > r2, a candidate qualifies iff dist2 <= r2.  The tested
 *      triangles are therefore a subset of srt_closest_points' candidates.
 *   2. A node that passes is pruned iff  low > best && low < +inf.  best: the minimum dist2 offered so far for that point as the walk
 *      sees it (+inf at the start; it may lag behind the offers, see COUNTERS).  low, with (dx, dy, dz) as the box test has them, f32
 *      without contraction:
 *          M   = the largest of |mn.x| |mn.y| |mn.z| |mx.x| |mx.y| |mx.z| |p.x| |p.y| |p.z|  (a maximum that passes a NaN operand over)
 *          z   = 0 if those nine values are all finite, else NaN
 *          s   = (SRT_NEAREST_K * 2^-24) * M + z
 *          tx  = dx - s;  tx = tx > 0 ? tx : 0          (ty, tz alike; a NaN becomes 0)
 *          low = ((tx*tx + ty*ty) + tz*tz) * (1 - 2^-20)
 *      In words: the box is grown by s on every side before the squared distance to it is taken.  s is SRT_NEAREST_K half-ulps of the
 *      largest coordinate in play, the scale of every rounding error between a triangle's vertices and its computed dist2.
 *   3. (a) MONOTONE: if box A contains box B then low(A, p) <= low(B, p) in these operations as written -- dx is no larger for A, M and
 *          s no smaller, and every later operation is monotone on non-negative operands.  So a bound that holds for a triangle's tight
 *          box holds for every box around it.
 *      (b) NAN-SAFE: a NaN or an infinity in the box or the point makes s NaN, so every t is 0 and low is 0; an overflowed low is +inf and
 *          is excluded; a NaN best (there is none: the initial bound compares as one) fails `low > best`.  None of them prunes.
 *      (c) SAFE: low(tight box of T, p) <= dist2(T, p) for every triangle T and point p whose dist2 is not NaN.  It follows from
 *          sqrt(b2) - sqrt(dist2) <= s, which is MEASURED, not proven: over the pairs of profiles/nearest_margin.txt the left side stays
 *          below 6.7 * 2^-24 M, and SRT_NEAREST_K is more than four times that.  DESIGN.md s5 "Nearest point" has the derivation.
 *      Hence the equality: every offered dist2 belongs to a candidate of srt_closest_points, so best is never below the final winner's
 *      dist2; by (a) and (c) no ancestor of the winner has low above that dist2; the winner is tested whatever the order of the tests, and
 *      ties go to the lowest id, as there.
 * PRECONDITIONS of the equality.
 *      - Boxes nest and contain their triangles' vertices: true of every scene built through the host mirror, and after srt_scene_pose
 *        and srt_scene_refit_device.  A hand-made hierarchy whose boxes do not nest does not meet it.
 *      - Property (c) holds for the winner.
 *   Where either fails, the call stays memory-safe and returns a QUALIFYING candidate with its own correct dist2, point, vw and region;
 *   that dist2 is never below the srt_closest_points winner's; but WHICH candidate comes back may then depend on the other points of the
 *   batch and their order.
 * COUNTERS.  Under SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary are of the walk as it ran.  They are NOT a function of the
 * point alone: triangle tests are queued per 64-point wave and run when 64 are queued or no point of the wave has a node left, and best
 * moves only then, so the count depends on the wave's other points.  They are at most srt_closest_points' counts at the same radius, and
 * at least the mandatory set's: the nodes all of whose ancestors pass the radius test with low <= the final dist2, and the triangles of
 * such leaves.  A node pruned by the bound counts as tested.
 * NOT HERE: a near-child-first order (the node layout has one order).  (The K nearest, pruned by the k-th best: see srt_points_multi.h.
 * A sign: see srt_signed.h.  The distance of a SEGMENT, within a radius that does not shrink: see srt_segments.h.) */
#define SRT_NEAREST_K 64     /* a power of two; at least four times the measured worst deficit (profiles/nearest_margin.txt) */
int srt_nearest_points_device(srt_scene* s, uint32_t n, const float* d_points /* n x 3 */, const float* d_radius /* n or NULL */,
                              const uint32_t* d_point_mask /* n or NULL */, uint32_t flags, void* stream, const srt_point_out* out);
int srt_nearest_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t flags,
                       const srt_point_out* out, srt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SRT_NEAREST_H */
