"""The yardstick of the ray queries with a per-ray t interval (include/srt.h, RAY QUERIES, "A t interval per ray"), built from the
oracle's leaf functions as they stand:

  * oracle.ray_aabb on every (ray, node) pair: the literal slab test;
  * reachability pushed down each object's tree from obj_root through node_left / node_right: a node is reached iff it and all its
    ancestors pass -- the nodes closest_in_tree and anyhit_in_tree descend into, no pruning by t;
  * oracle.ray_triangle on every (ray, triangle) pair of the reached leaves: the candidate set of the ray and each candidate's t;
  * the header's definition in numpy, on that set: in range iff !(t < t_min) && !(t > t_max); the closest hit is the first minimum of t
    (lowest id among equal t, -0 keyed as +0) among the in-range candidates with t != -inf && t < +inf; occluded iff a candidate outside
    the skipped object has t != -inf and is in range.

At (0, +inf) it is the oracle's own closest hit and shadow rule (tests/test_ray_range_ref.py pins that against ray_query_ref)."""
from dataclasses import dataclass

import numpy as np

PAIRS_A_CHUNK = 1 << 21           # (ray, node) pairs handed to oracle.ray_aabb at once


@dataclass
class Candidates:
    """One entry per (ray, candidate triangle), sorted by ray, then by triangle id."""
    n_rays: int
    ray: np.ndarray               # int64
    tri: np.ndarray               # int64, canonical triangle id
    t: np.ndarray                 # float32, oracle.ray_triangle's result with its own bits

    def finite(self):
        """Per ray: how many candidates the closest hit may take when nothing bounds t (t != -inf && t < +inf)."""
        with np.errstate(invalid="ignore"):
            ok = (self.t != -np.inf) & (self.t < np.inf)
        return np.bincount(self.ray[ok], minlength=self.n_rays)

    def nan(self):
        return np.bincount(self.ray[np.isnan(self.t)], minlength=self.n_rays)


def reached_nodes(oracle, flat, rays):
    """n_rays x n_nodes bool: the node and all its ancestors pass the literal slab test."""
    n, N = rays.shape[0], flat.n_nodes
    box = np.concatenate([flat.node_min.reshape(-1, 3), flat.node_max.reshape(-1, 3)], axis=1).astype(np.float32)
    passed = np.empty((n, N), bool)
    step = max(1, PAIRS_A_CHUNK // max(N, 1))
    for a in range(0, n, step):
        r = rays[a:a + step]
        passed[a:a + step] = oracle.ray_aabb(np.repeat(r, N, axis=0), np.tile(box, (r.shape[0], 1))).reshape(-1, N).astype(bool)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    reach = np.zeros((n, N), bool)
    cur = flat.obj_root.astype(np.int64)
    reach[:, cur] = passed[:, cur]
    while cur.size:
        inner = cur[(left[cur] >= 0) | (right[cur] >= 0)]
        assert (left[inner] >= 0).all() and (right[inner] >= 0).all(), "a node has two children or none"
        for child in (left[inner], right[inner]):
            reach[:, child] = reach[:, inner] & passed[:, child]
        cur = np.concatenate([left[inner], right[inner]])
    return reach


def candidates(oracle, flat, rays):
    """The candidate set of every ray of `rays` (n x 6) on `flat`, with the oracle's t of every candidate."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    reach = reached_nodes(oracle, flat, rays)
    leaf = (flat.node_left < 0) & (flat.node_right < 0)
    ri, ni = np.nonzero(reach[:, leaf])
    ni = np.flatnonzero(leaf)[ni]
    cnt = flat.node_count[ni].astype(np.int64)
    start = np.cumsum(cnt) - cnt
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(start, cnt)
    ray = np.repeat(ri.astype(np.int64), cnt)
    tri = np.repeat(flat.node_first[ni].astype(np.int64), cnt) + within
    order = np.lexsort((tri, ray))
    ray, tri = ray[order], tri[order]
    pts = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 12)
    t = oracle.ray_triangle(rays[ray], pts[tri]) if ray.size else np.empty(0, np.float32)
    return Candidates(rays.shape[0], ray, tri, t)


def full_range(n, t_range):
    """t_range (n x 2, or None: nothing bounds t) as two float32 columns."""
    if t_range is None:
        return np.full(n, -np.inf, np.float32), np.full(n, np.inf, np.float32)
    tr = np.ascontiguousarray(t_range, np.float32).reshape(n, 2)
    return tr[:, 0], tr[:, 1]


def in_range(c, t_range):
    lo, hi = full_range(c.n_rays, t_range)
    with np.errstate(invalid="ignore"):
        return ~(c.t < lo[c.ray]) & ~(c.t > hi[c.ray])        # closed; a NaN bound bounds nothing; a NaN t is in range


def closest(c, t_range=None):
    """(hit_id, t): -1 and +inf on a miss, else the winner's id and its t with its own bits."""
    with np.errstate(invalid="ignore"):
        ok = (c.t != -np.inf) & (c.t < np.inf) & in_range(c, t_range)
    ray, tri, t = c.ray[ok], c.tri[ok], c.t[ok]
    order = np.lexsort((tri, t + np.float32(0.0), ray))      # -0 + 0 = +0: the two zeros tie, the lowest id first
    ray, tri, t = ray[order], tri[order], t[order]
    first = np.ones(ray.size, bool)
    first[1:] = ray[1:] != ray[:-1]
    hit = np.full(c.n_rays, -1, np.int32); tt = np.full(c.n_rays, np.inf, np.float32)
    hit[ray[first]] = tri[first]; tt[ray[first]] = t[first]
    return hit, tt


def occluded(c, flat, t_range=None, skip_obj=None):
    """uint8 per ray: a candidate outside object skip_obj[i] has t != -inf (NaN included) and is in range."""
    blocks = (c.t != -np.inf) & in_range(c, t_range)
    if skip_obj is not None:
        blocks &= flat.tri_obj[c.tri].astype(np.int64) != np.asarray(skip_obj, np.int64).reshape(-1)[c.ray]
    return (np.bincount(c.ray[blocks], minlength=c.n_rays) > 0).astype(np.uint8)


def next_up(t):
    return np.nextafter(np.asarray(t, np.float32), np.float32(np.inf))


def next_down(t):
    return np.nextafter(np.asarray(t, np.float32), np.float32(-np.inf))


def mixed_intervals(c, seed):
    """One interval per ray, the kinds dealt round robin so that neighbours differ.  t1 = the ray's closest hit without bounds (a miss
    takes the batch's median instead): 0 (next_up(t1), inf) -- the second hit; 1 (0, next_down(t1)) -- a miss; 2 (t1, t1) -- closed, the
    same id; 3 t_min > t_max; 4 and 5 random intervals around t1; 6 one bound NaN."""
    rng = np.random.default_rng(seed)
    n = c.n_rays
    hit, t1 = closest(c)
    mid = np.float32(np.median(t1[hit >= 0])) if (hit >= 0).any() else np.float32(1.0)
    base = np.where(hit >= 0, t1, mid).astype(np.float32)
    a = (base * rng.uniform(0.0, 2.0, n)).astype(np.float32)
    b = (a + base * rng.uniform(0.0, 2.0, n)).astype(np.float32)
    kind = np.arange(n) % 7
    tr = np.empty((n, 2), np.float32)
    tr[:, 0] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 6], [next_up(base), 0.0, base, next_up(b), np.float32(np.nan)], a)
    tr[:, 1] = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 6], [np.float32(np.inf), next_down(base), base, a, a], b)
    swap = (kind == 6) & (np.arange(n) % 2 == 1)
    tr[swap] = tr[swap][:, ::-1]
    return tr, kind, hit


def want_bary(oracle, flat, rays, hit, t):
    """calculateBarycentricCoords of every hit at o + d * t (three float32 operations), (0, 0, 0) on a miss."""
    out = np.zeros((rays.shape[0], 3), np.float32)
    sel = hit >= 0
    dt = rays[sel, 3:6] * t[sel, None]
    P = rays[sel, 0:3] + dt
    pts = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 12)[hit[sel]]
    out[sel] = oracle.barycentric(np.concatenate([pts, P], axis=1))
    return out
