/* include/srt_points.h -- closest-point queries of the C ABI in include/srt.h: the nearest triangle within a radius, per point.
 *
 * An extension header of include/srt.h, which includes it at its end: a program that includes srt.h has these declarations, and this file
 * may be included on its own.  Same conventions: plain C, PODs, caller-owned buffers, int return codes; the handle, srt_stats, the flags and
 * the error codes are srt.h's.  SRT_ABI_VERSION stays 3: nothing that existed changes.
 */
#ifndef SRT_POINTS_H
#define SRT_POINTS_H

#include "srt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Closest point: for every point of a batch, the nearest triangle within a radius and the nearest point on it -- the other half of what a
 * bounding hierarchy is for: cloth and particle collision, snapping a point to a mesh, clearance around a sensor, a distance-field
 * slice, the loss of a mesh-fitting optimiser.  It reads the records the ray queries read (P1, e1, e2 of a triangle, the 32 B nodes), so
 * srt_scene_pose, srt_scene_refit_device, srt_scene_share and the object masks apply to it as they do to srt_trace_rays_masked.
 * Unless said here everything is as for srt_trace_rays_masked (include/srt.h): flags are 0 or SRT_FLAG_COUNT_WORK, the ordering on `stream`, the rules of
 * srt_scene_share, the private counter set, ONE launch with nothing allocated and nothing copied, hipGraph capture of the _device form
 * without SRT_FLAG_COUNT_WORK.
 * DEFINITION.  All arithmetic is f32 without contraction; dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z; divides are IEEE divides.
 *   The radius  point i has the radius r = radius[i]; a NULL array means +inf.  r2 = r * r.  A point whose r is negative or NaN finds
 *               nothing and walks nothing (-0 is not negative: r2 = 0).
 *   Box test    per axis, with (mn, mx) the node's box:  e = mn - p;  f = p - mx;  dx = e > f ? e : f;  dx = dx > 0 ? dx : 0.  Then
 *               b2 = (dx*dx + dy*dy) + dz*dz, and a node passes iff !(b2 > r2).
 *   Candidates  the triangles of every leaf whose ancestors and itself all pass.  The radius is the caller's and NEVER SHRINKS during the
 *               walk; nothing depends on what was found so far.  Under SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary are
 *               therefore a function of the scene and the point alone (a leaf taken in slices counts once).
 *   Triangle    Ericson's Voronoi-region closest point (Real-Time Collision Detection 5.1.5) on the record's operands P1, e1, e2:
 *                   ap = p - P1    d1 = dot(e1, ap)   d2 = dot(e2, ap)
 *                   bp = ap - e1   d3 = dot(e1, bp)   d4 = dot(e2, bp)
 *                   cp = ap - e2   d5 = dot(e1, cp)   d6 = dot(e2, cp)
 *                   vc = d1*d4 - d3*d2     vb = d5*d2 - d1*d6     va = d3*d6 - d5*d4     g = d4 - d3     h = d5 - d6
 *               The regions are tested in this order and the first true one wins:
 *                   region 4, vertex 1   d1 <= 0 && d2 <= 0               (v, w) = (0, 0)
 *                   region 5, vertex 2   d3 >= 0 && d4 <= d3              (v, w) = (1, 0)
 *                   region 1, edge 1-2   vc <= 0 && d1 >= 0 && d3 <= 0    (v, w) = (d1 / (d1 - d3), 0)
 *                   region 6, vertex 3   d6 >= 0 && d5 <= d6              (v, w) = (0, 1)
 *                   region 3, edge 1-3   vb <= 0 && d2 >= 0 && d6 <= 0    (v, w) = (0, d2 / (d2 - d6))
 *                   region 2, edge 2-3   va <= 0 && g >= 0 && h >= 0      w = g / (g + h), v = 1 - w
 *                   region 0, face       otherwise                        v = vb / ((va + vb) + vc), w = vc / ((va + vb) + vc)
 *               Then per component q = e1*v + e2*w, rr = ap - q, dist2 = (rr.x*rr.x + rr.y*rr.y) + rr.z*rr.z, point = P1 + q.
 *   Qualifies   a candidate qualifies iff dist2 <= r2 (closed; a NaN fails).  A zero-area triangle, a record with non-finite values and a
 *               NaN point give what this arithmetic gives, and a NaN dist2 qualifies for nothing; all of them are memory-safe.
 *   The winner  the minimum dist2 among the qualifying candidates, equal dist2 to the lowest triangle id (dist2 is never -0).  None:
 *               tri -1, dist2 +inf, point (0, 0, 0), vw (0, 0), region 0.  Results never depend on the order of the points in a call.
 * WHY NO SHRINKING RADIUS.  Pruning a box by the best distance so far is not bit-safe: e1 and e2 are ROUNDED differences, so the computed
 * dist2 of a triangle can lie below the computed b2 of that triangle's own tight box (about 0.6 % of random point / triangle pairs around
 * the origin in an f32 prototype), and a shrinking walk would change winners.  A caller who wants speed passes a radius.
 * MASKS.  point_mask: n words, or NULL = all ones.  Object k is walked for point i iff (obj_mask[k] & point_mask[i]) != 0, exactly as
 * srt_trace_rays_masked walks a ray ("distance to everything but my own object").  All ones gives the unmasked call's bits and counters;
 * a NULL point_mask launches the build that never reads the scene's table.
 * Points are n x 3 floats at any float alignment, read with 4-byte loads; nothing past the last point is read.
 * Errors, before anything is touched: SRT_ERR_ARG for a NULL handle, a NULL `out`, NULL points with n > 0, any other flag bit.  n == 0:
 * SRT_OK with nothing done.  Every field of *out NULL in the _device form: SRT_OK, nothing launched.
 * The host form stages points, radius, point_mask and the outputs through the handle's pinned block, then waits.  *stats: primary_rays = n,
 * hit_rays = the points that found a triangle, node_tests_primary / tri_tests_primary under SRT_FLAG_COUNT_WORK.
 * NOT HERE: a shrinking radius (above; see srt_nearest.h); a SIGN -- the distance is unsigned; see srt_signed.h, which counts the sign
 * along rays; `region` serves a caller who keeps pseudo-normals of their own (face, edge or vertex normal by region) --; the K nearest
 * triangles, and how many lie within the radius: see srt_points_multi.h (n_within > 0 is the any-within-radius answer, without the early
 * stop); the distance of a SEGMENT -- a particle's step, a capsule, a path with a width --: see srt_segments.h, whose point segments are
 * this call bit for bit. */
typedef struct srt_point_out {    /* device pointers in the _device form, host pointers in the host form */
    int32_t* tri;                /* n       canonical triangle id, -1 = none within the radius */
    float*   dist2;              /* n       the winner's dist2 with its own bits, +inf = none */
    float*   point;              /* n x 3   P1 + q of the winner */
    float*   vw;                 /* n x 2   (v, w) of the winner */
    uint8_t* region;             /* n       0 face, 1..3 edges, 4..6 vertices, as above */
} srt_point_out;                 /* any pointer may be NULL; all NULL in the _device form: SRT_OK, nothing launched */
int srt_closest_points_device(srt_scene* s, uint32_t n, const float* d_points /* n x 3 */, const float* d_radius /* n or NULL */,
                              const uint32_t* d_point_mask /* n or NULL */, uint32_t flags, void* stream, const srt_point_out* out);
int srt_closest_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t flags,
                       const srt_point_out* out, srt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SRT_POINTS_H */
