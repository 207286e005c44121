/* include/srt_signed.h -- signed distance and containment per point: srt_nearest_points' distance with a sign counted along a few rays.
 *
 * An extension header of include/srt.h, which includes it at its end, after include/srt_nearest.h; it may be included on its own.  Same
 * conventions; srt_point_out, the handle, srt_stats, the flags and the error codes are theirs.  SRT_ABI_VERSION stays 3.
 */
#ifndef SRT_SIGNED_H
#define SRT_SIGNED_H

#include "srt_nearest.h"

#ifdef __cplusplus
extern "C" {
#endif

/* srt_signed_points answers "on which side": collision (is the particle already inside?), a signed distance-field slice, a fitting loss,
 * clearance, voxelisation, point-in-mesh tests.  The sign of a point is the WINDING of the surface around it, counted along n_dirs rays
 * from the point on the records every other query reads: srt_scene_pose, srt_scene_refit_device, srt_scene_share and the object masks
 * apply with no scene state of its own.  It is meant for CLOSED meshes whose normals e1 x e2 point out of the solid, the convention
 * srt_shade_paths_refract requires; on an open mesh it gives what the definition gives (a ray through a hole loses a crossing).
 * DEFINITION.  All arithmetic is f32 without contraction; dot and cross as ray_triangle (srt_device.h) writes them.
 *   1. Point outputs.  *out is srt_nearest_points' (include/srt_nearest.h) for the same scene, points, radius and mask, bit for bit.
 *      PRECONDITIONS of that equality, taken over from there:
 *        - Boxes nest and contain their triangles' vertices: true of every scene built through the host mirror, and after srt_scene_pose
 *          and srt_scene_refit_device.  A hand-made hierarchy whose boxes do not nest does not meet it.
 *        - Property (c) holds for the winner.
 *      Where either fails, the call stays memory-safe and returns a QUALIFYING candidate with its own correct dist2, point, vw and region;
 *      that dist2 is never below the srt_closest_points winner's; but WHICH candidate comes back may then depend on the other points of the
 *      batch and their order.
 *   2. Sign rays.  Ray j of point i is (o, d) = (p_i, dirs[j]), unbounded.  It is walked over the objects k with
 *      (obj_mask[k] & point_mask[i]) != 0 exactly as srt_trace_rays_masked walks a ray: the same slab test on the same nodes, the same
 *      candidate set.  A candidate COUNTS iff t != -inf && t < +inf, the closest hit's rule: a NaN t does not count, t = +-0 does.  With
 *      det = dot(e1, cross(d, e2)) as ray_triangle computes it on the record's e1, e2, a counted candidate is an ENTRY iff det > 0 and an
 *      EXIT iff det < 0 (a counted candidate has |det| >= 1e-12 and no NaN, so it is one or the other; with outward normals det = -d.n).
 *          winding[i][j] = exits - entries          crossings[i][j] = exits + entries
 *   3. The vote.  vote_j = (sign->flags & SRT_SIGN_PARITY) ? (crossings_j & 1) : (winding_j > 0);  inside = 2 * (sum of vote_j) > n_dirs.
 *      Winding is the default because it is right for overlapping closed objects, where parity gives XOR; parity is for meshes whose
 *      orientation is not consistent.
 *   4. The signed distance.  sdist = inside ? -sqrt(dist2) : sqrt(dist2), dist2 of item 1, an IEEE correctly rounded sqrt.  A point with
 *      no triangle within its radius gets -inf or +inf.
 *   5. The sign does not depend on the radius.  EVERY live point gets its rays, also one whose radius is negative or NaN, which walks
 *      nothing in the nearest phase.  A caller who wants containment only leaves `out` NULL and asks for no sdist: the nearest phase then
 *      does not run at all -- point-in-mesh for the price of n_dirs ray walks.  A caller who wants a narrow band filters the points with
 *      srt_closest_points (a radius) first and passes on the ones it found: this call has no skip of its own.
 *   6. The default table (sign NULL, or sign->dirs NULL with n_dirs 0): SRT_SIGN_DEFAULT_DIRS below, three directions that are not unit
 *      length -- nothing reads t's scale -- and parallel to no axis, face diagonal or body diagonal.  A zero, non-finite or axis-parallel
 *      direction of a caller's table gives what the arithmetic gives.
 *   7. sout NULL, or every field of it NULL: the call is srt_nearest_points with that call's kernels, and `sign` is not read.  Everything
 *      NULL in the _device form: SRT_OK, nothing launched.  n == 0: SRT_OK.
 * Errors, before anything is touched: srt_closest_points' (a NULL handle, NULL points with n > 0, any flag bit but SRT_FLAG_COUNT_WORK), and
 * SRT_ERR_ARG for n_dirs > SRT_SIGN_MAX_DIRS, n_dirs == 0 with dirs != NULL or the reverse, an unknown bit in sign->flags, `out` and `sout`
 * both NULL.
 * Everything else is srt_nearest_points': `flags` is 0 or SRT_FLAG_COUNT_WORK, stream ordering, shared handles, ONE launch with nothing
 * allocated, hipGraph capture of the _device form without counting.  The host form stages through the handle's pinned block and stages
 * dirs as well.  *stats: primary_rays = n, hit_rays = the points that found a triangle (0 when the nearest phase did not run),
 * shadow_rays = n x n_dirs.  Under SRT_FLAG_COUNT_WORK the nearest phase goes into node_tests_primary / tri_tests_primary as
 * srt_nearest_points counts them (they depend on the batch); the sign rays go into node_tests_shadow / tri_tests_shadow, which ARE a
 * function of scene, point, mask and table alone: a ray's count is srt_trace_rays_masked's.
 * NOT HERE: a sign for open meshes; per-direction weights; a narrow-band skip inside the call; the K nearest; an any-within-radius form.
 * `region` of srt_point_out stays what it is, for callers who keep pseudo-normals of their own. */
#define SRT_SIGN_MAX_DIRS 16
#define SRT_SIGN_PARITY   1u          /* vote by crossings & 1 instead of winding > 0 */
#define SRT_SIGN_DEFAULT_DIRS { 0.57f, 0.31f, 0.76f,  -0.43f, 0.81f, -0.39f,  0.29f, -0.66f, -0.69f }
typedef struct srt_sign {
    const float* dirs;            /* n_dirs x 3; device memory in the _device form, host memory in the host form; NULL: the default table */
    uint32_t     n_dirs;          /* 1 .. SRT_SIGN_MAX_DIRS; 0 iff dirs is NULL */
    uint32_t     flags;           /* 0 or SRT_SIGN_PARITY */
} srt_sign;
typedef struct srt_sign_out {     /* device pointers in the _device form, host pointers in the host form; any pointer may be NULL */
    float*    sdist;              /* n            inside ? -sqrt(dist2) : +sqrt(dist2) */
    uint8_t*  inside;             /* n            1 / 0 */
    int32_t*  winding;            /* n x n_dirs   exits - entries along direction j */
    uint32_t* crossings;          /* n x n_dirs   exits + entries */
} srt_sign_out;
int srt_signed_points_device(srt_scene* s, uint32_t n, const float* d_points /* n x 3 */, const float* d_radius /* n or NULL */,
                             const uint32_t* d_point_mask /* n or NULL */, const srt_sign* sign /* NULL = defaults */, uint32_t flags, void* stream,
                             const srt_point_out* out /* may be NULL */, const srt_sign_out* sout);
int srt_signed_points(srt_scene* s, uint32_t n, const float* points, const float* radius, const uint32_t* point_mask, const srt_sign* sign,
                      uint32_t flags, const srt_point_out* out, const srt_sign_out* sout, srt_stats* stats);

#ifdef __cplusplus
}
#endif
#endif /* SRT_SIGNED_H */
