/* include/srt_points_multi.h -- the K nearest triangles per point: every contact within a radius, or the few nearest faces, in one walk.
 *
 * An extension header of include/srt.h, which includes it at its end, after include/srt_signed.h; it may be included on its own.  Same
 * conventions: plain C, PODs, caller-owned buffers, int return codes; the handle, srt_stats, the flags and the error codes are srt.h's.
 * SRT_ABI_VERSION stays 3: nothing that existed changes.
 */
#ifndef SRT_POINTS_MULTI_H
#define SRT_POINTS_MULTI_H

#include "srt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* srt_closest_points and srt_nearest_points return ONE triangle per point.  A particle near an edge or a fold touches several, and a solver
 * wants all contacts within its thickness; a fitting loss wants the few nearest faces; a clearance check wants to know HOW MANY triangles
 * lie within r.  The two calls here keep the k best candidates of a point, k = 1 .. SRT_POINT_MULTI_MAX, in the walk those calls run.
 * Row i of an n x k output is words i*k .. i*k+k-1, as in srt_trace_rays_multi.
 *
 * THE CLOSEST FORM, srt_closest_points_multi, is srt_closest_points (include/srt_points.h) except for what is kept of the qualifying
 * candidates.  The radius (NULL = +inf, never shrinking), the box test, the candidates, the triangle arithmetic and the "qualifies" rule
 * are that header's, operation by operation; so are the masks, the stream ordering, the rules of shared handles, ONE launch with nothing
 * allocated and nothing copied, and hipGraph capture of the _device form without SRT_FLAG_COUNT_WORK.
 *   n_within    ALL qualifying candidates of the point; it may exceed k.  A function of the scene and the point alone.
 *   n_found     the filled columns, min(k, n_within).
 *   column j    the (j+1)-th qualifying candidate in (dist2, id) order -- dist2 is never -0, so that is the order of (dist2 bits, id) --
 *               with that triangle's OWN dist2, point, vw and region.  Column 0 is srt_closest_points' winner bit for bit.  Coplanar
 *               duplicates, and triangles that share the nearest vertex or edge, have equal dist2 and are all reported, lowest id first.
 *               An empty column: tri -1, dist2 +inf, point (0, 0, 0), vw (0, 0), region 0.
 *   Counters    under SRT_FLAG_COUNT_WORK node_tests_primary / tri_tests_primary are exactly srt_closest_points' for the same call.
 *   Results never depend on the order of the points in a call.
 *
 * THE NEAREST FORM, srt_nearest_points_multi, gives the same columns and the same n_found, bit for bit, on every scene that meets the
 * PRECONDITIONS of include/srt_nearest.h, with precondition (c) read for EACH of the k winners.  It is srt_nearest_points' walk with one
 * difference: the bound a node is pruned by (rule 2 there) and a candidate is filtered by is the K-TH BEST dist2 offered so far for the
 * point, not the best; while fewer than k candidates were kept there is no bound.  A caller who wants the few nearest faces passes no
 * radius and pays for the neighbourhood of the answer.
 *   Why the k winners are found.  The k best keys of a point live in k slots; slot j is only ever written by an atomic minimum, so it only
 *   decreases, and it ends as the (j+1)-th smallest key offered.  Any value the walk reads from slot k-1 is therefore never below the FINAL
 *   k-th dist2.  Every offered dist2 belongs to a candidate of the closest form, so that final value is never below the closest form's
 *   k-th dist2.  By (a) and (c) of srt_nearest.h no ancestor of any of the k winners has `low` above its winner's dist2, hence none above
 *   the bound; each winner is tested whatever the order of the tests, passes the filter !(dist2 > bound), and equal dist2 go by lowest id.
 *   n_within    is NOT DEFINED under pruning: a non-NULL n_within returns SRT_ERR_ARG, before anything is touched.
 *   Counters    of the walk as it ran (srt_nearest.h, COUNTERS): at most the closest form's at the same radius, at least the mandatory
 *               set's evaluated at the k-th winner's dist2 -- at the radius where fewer than k are found.
 *   Where a precondition fails the call stays memory-safe; every returned column is a QUALIFYING candidate with its own correct dist2,
 *   point, vw and region; the columns are sorted by (dist2, id) and distinct; n_found is still min(k, n_within) -- nothing is pruned
 *   before k candidates were kept -- and column j's dist2 is never below the closest form's.  WHICH candidates come back may then depend on
 *   the other points of the batch.
 *
 * Errors, before anything is touched: SRT_ERR_ARG for a NULL handle, a NULL `out`, NULL points with n > 0, any flag bit but
 * SRT_FLAG_COUNT_WORK, k outside 1 .. SRT_POINT_MULTI_MAX, n_within in the nearest form.  n == 0: SRT_OK with nothing done.  Every field
 * of *out NULL in the _device form: SRT_OK, nothing launched.
 * The host forms stage points, radius, point_mask and the outputs through the handle's pinned block, then wait.  *stats: primary_rays = n,
 * hit_rays = the points with n_found > 0, node_tests_primary / tri_tests_primary under SRT_FLAG_COUNT_WORK.
 * NOT HERE: k > 16; a near-child-first order; the object of a candidate (tri_obj is the caller's); a sign per column (srt_signed.h has the
 * point's). */
#define SRT_POINT_MULTI_MAX 16
typedef struct srt_point_multi_out {   /* device pointers in the _device form, host pointers in the host form; any may be NULL */
    uint32_t* n_within;   /* n          ALL qualifying candidates of the point (closest form only) */
    uint32_t* n_found;    /* n          filled columns = min(k, n_within) */
    int32_t*  tri;        /* n x k      nearest first, equal dist2 by lowest id; -1 = empty column */
    float*    dist2;      /* n x k      +inf = empty */
    float*    point;      /* n x k x 3  zeros = empty */
    float*    vw;         /* n x k x 2 */
    uint8_t*  region;     /* n x k */
} srt_point_multi_out;
int srt_closest_points_multi_device(srt_scene* s, uint32_t n, const float* d_points /* n x 3 */, const float* d_radius /* n or NULL */,
                                    const uint32_t* d_point_mask /* n or NULL */, uint32_t k, uint32_t flags, void* stream,
                                    const srt_point_multi_out* out);
int srt_closest_points_multi(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t k,
                             uint32_t flags, const srt_point_multi_out* out, srt_stats* stats);
int srt_nearest_points_multi_device(srt_scene* s, uint32_t n, const float* d_points /* n x 3 */, const float* d_radius /* n or NULL */,
                                    const uint32_t* d_point_mask /* n or NULL */, uint32_t k, uint32_t flags, void* stream,
                                    const srt_point_multi_out* out);
int srt_nearest_points_multi(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, uint32_t k,
                             uint32_t flags, const srt_point_multi_out* out, srt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SRT_POINTS_MULTI_H */
