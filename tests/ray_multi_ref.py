"""The yardstick of srt_trace_rays_multi (include/srt.h, RAY QUERIES, "The K nearest hits of a ray in one walk"): plain numpy on the
candidate set of tests/ray_range_ref.py -- the oracle's slab test on every node, its triangle test on every triangle of the reached
leaves.  Q of a ray = its candidates with t != -inf && t < +inf that are in range; sorted by (t with -0 keyed as +0, id), as
ray_range_ref.closest sorts them; the first k are the row, the count is n_hits.

Below it: the `stack` scene and batch of the overflow cases (40 parallel triangles behind each other, every ray through all of them)."""
import functools

import numpy as np

import ray_range_ref as rr
import tree_shapes as ts

INF = np.float32(np.inf)


def multi(c, k, t_range=None):
    """(n_hits uint32 n, hit_id int32 n x k, t float32 n x k): the full count, and the k first of Q with their own t bits; the rest of a
    row is -1 and +inf."""
    with np.errstate(invalid="ignore"):
        ok = (c.t != -np.inf) & (c.t < np.inf) & rr.in_range(c, t_range)
    ray, tri, t = c.ray[ok], c.tri[ok], c.t[ok]
    order = np.lexsort((tri, t + np.float32(0.0), ray))      # -0 + 0 = +0: the two zeros tie, the lowest id first
    ray, tri, t = ray[order], tri[order], t[order]
    n_hits = np.bincount(ray, minlength=c.n_rays)
    rank = np.arange(ray.size, dtype=np.int64) - (np.cumsum(n_hits) - n_hits)[ray]
    keep = rank < k
    hit = np.full((c.n_rays, k), -1, np.int32); tt = np.full((c.n_rays, k), INF, np.float32)
    hit[ray[keep], rank[keep]] = tri[keep]; tt[ray[keep], rank[keep]] = t[keep]
    return n_hits.astype(np.uint32), hit, tt


def multi_bary(oracle, flat, rays, hit, t):
    """n x k x 3: ray_range_ref.want_bary column by column -- every hit at its own o + d * t, (0, 0, 0) in an unused slot."""
    return np.stack([rr.want_bary(oracle, flat, rays, hit[:, j], t[:, j]) for j in range(hit.shape[1])], axis=1)


def equal_t_groups(c, t_range=None):
    """(groups of two or more members of Q with the same t key on one ray, the deepest such group)."""
    with np.errstate(invalid="ignore"):
        ok = (c.t != -np.inf) & (c.t < np.inf) & rr.in_range(c, t_range)
    key = np.stack([c.ray[ok], (c.t[ok] + np.float32(0.0)).view(np.uint32).astype(np.int64)], axis=1)
    if not key.shape[0]:
        return 0, 0
    _, counts = np.unique(key, axis=0, return_counts=True)
    return int((counts >= 2).sum()), int(counts.max())


def zero_pairs(c):
    """bool per ray: Q (unbounded) is exactly one +0 and one -0."""
    n_hits, hit, t = multi(c, 3)
    b = t.view(np.uint32)
    return (n_hits == 2) & (np.sort(b[:, :2], axis=1) == np.array([0, 0x80000000], np.uint32)).all(1)


# ---- the overflow scene ------------------------------------------------------------------------------------------------------------
STACK_LAYERS, STACK_Z0, STACK_DZ, STACK_RAYS = 40, 100.0, 3.0, 65


@functools.lru_cache(maxsize=None)
def stack_scene():
    """One object of 40 parallel triangles z = 100 + 3 j, leaves (31, 9): the big leaf is pushed in slices."""
    tris = np.ones((STACK_LAYERS, 3, 4), np.float32)
    for j in range(STACK_LAYERS):
        z = STACK_Z0 + STACK_DZ * j
        tris[j, :, :3] = [[-30.0, -30.0, z], [30.0, -30.0, z], [0.0, 40.0, z]]
    return ts.flat_scene([dict(tris=tris, leaves=(31, 9), shape="left_comb")])


@functools.lru_cache(maxsize=None)
def stack_rays():
    """65 rays from near the origin along +z with a small tilt: each crosses all 40 layers, at t = z of the layer (d.z = 1, o.z = 0)."""
    rng = np.random.default_rng(40)
    r = np.zeros((STACK_RAYS, 6), np.float32)
    r[:, 0:2] = rng.uniform(-2.0, 2.0, (STACK_RAYS, 2))
    r[:, 3:5] = rng.uniform(-0.02, 0.02, (STACK_RAYS, 2))
    r[:, 5] = 1.0
    r.setflags(write=False)
    return r


def stack_segment(layers):
    """The interval that admits exactly the layers 5 .. 5 + layers - 1 of every ray of stack_rays (bounds midway between two layers)."""
    lo = STACK_Z0 + STACK_DZ * 5 - 1.5
    return np.tile(np.float32([lo, lo + STACK_DZ * layers]), (STACK_RAYS, 1))
