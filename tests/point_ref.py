"""The yardstick of the closest-point query (include/srt_points.h): plain numpy float32, one array statement per operation, in
the header's association.

  * the records are tests/refit_edges.derive_ref's (P1, e1, e2 per triangle, as the device derives them), or DeviceScene.records();
  * the box test on every (point, node) pair, and reachability pushed down each object's tree from obj_root through node_left /
    node_right, as ray_range_ref.reached_nodes does it: a node is reached iff it and all its ancestors pass.  The radius never shrinks;
  * Ericson's closest point on every (point, triangle) pair of the reached leaves: the candidate set and each candidate's
    (v, w, region, dist2, point);
  * the winner by lexsort((tri, dist2, point)) among the candidates with dist2 <= r2;
  * both work counts: a node is TESTED iff it is the root of a walked object or its parent is reached (a leaf in slices counts once);
    a triangle is tested iff its leaf is reached.

Masks: object k is walked for point i iff (obj_mask[k] & point_mask[i]) != 0.  A point whose radius is negative or NaN walks nothing."""
import numpy as np

import refit_edges as re_

F = np.float32
INF = F(np.inf)
PAIRS_A_CHUNK = 1 << 20           # (point, triangle) pairs evaluated at once


def records_of(flat):
    """The triangle records the device derives from the flat scene's points: n_tris x 12 float32 (P1, e1, e2, normal)."""
    return re_.derive_ref(flat.tri_points)[0]


def dot(ax, ay, az, bx, by, bz):
    m0 = ax * bx; m1 = ay * by; m2 = az * bz
    s0 = m0 + m1
    return s0 + m2


def closest_on_triangles(p, rec):
    """Point p[k] against record rec[k] (m x 3, m x 12 float32): dict of v, w, dist2 (m float32), point (m x 3), region (m uint8)."""
    p = np.ascontiguousarray(p, F).reshape(-1, 3); rec = np.ascontiguousarray(rec, F).reshape(-1, 12)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    p1x, p1y, p1z, e1x, e1y, e1z, e2x, e2y, e2z = [rec[:, k] for k in range(9)]
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        apx = px - p1x; apy = py - p1y; apz = pz - p1z
        d1 = dot(e1x, e1y, e1z, apx, apy, apz); d2 = dot(e2x, e2y, e2z, apx, apy, apz)
        bpx = apx - e1x; bpy = apy - e1y; bpz = apz - e1z
        d3 = dot(e1x, e1y, e1z, bpx, bpy, bpz); d4 = dot(e2x, e2y, e2z, bpx, bpy, bpz)
        cpx = apx - e2x; cpy = apy - e2y; cpz = apz - e2z
        d5 = dot(e1x, e1y, e1z, cpx, cpy, cpz); d6 = dot(e2x, e2y, e2z, cpx, cpy, cpz)
        a0 = d1 * d4; a1 = d3 * d2; vc = a0 - a1
        b0 = d5 * d2; b1 = d1 * d6; vb = b0 - b1
        c0 = d3 * d6; c1 = d5 * d4; va = c0 - c1
        g = d4 - d3; h = d5 - d6
        r4 = (d1 <= zero) & (d2 <= zero)
        r5 = (d3 >= zero) & (d4 <= d3)
        r1 = (vc <= zero) & (d1 >= zero) & (d3 <= zero)
        r6 = (d6 >= zero) & (d5 <= d6)
        r3 = (vb <= zero) & (d2 >= zero) & (d6 <= zero)
        r2 = (va <= zero) & (g >= zero) & (h >= zero)
        region = np.select([r4, r5, r1, r6, r3, r2], [4, 5, 1, 6, 3, 2], 0).astype(np.uint8)
        d13 = d1 - d3; v1 = d1 / d13
        d26 = d2 - d6; w3 = d2 / d26
        gh = g + h; w2 = g / gh; v2 = one - w2
        s0 = va + vb; den = s0 + vc; v0 = vb / den; w0 = vc / den
        zeros, ones = np.zeros_like(d1), np.ones_like(d1)
        v = np.select([region == 4, region == 5, region == 1, region == 6, region == 3, region == 2], [zeros, ones, v1, zeros, zeros, v2], v0).astype(F)
        w = np.select([region == 4, region == 5, region == 1, region == 6, region == 3, region == 2], [zeros, zeros, zeros, ones, w3, w2], w0).astype(F)
        qx0 = e1x * v; qx1 = e2x * w; qx = qx0 + qx1
        qy0 = e1y * v; qy1 = e2y * w; qy = qy0 + qy1
        qz0 = e1z * v; qz1 = e2z * w; qz = qz0 + qz1
        rx = apx - qx; ry = apy - qy; rz = apz - qz
        dist2 = dot(rx, ry, rz, rx, ry, rz)
        ox = p1x + qx; oy = p1y + qy; oz = p1z + qz
    assert dist2.dtype == F and v.dtype == F and ox.dtype == F
    return dict(v=v, w=w, dist2=dist2, point=np.stack([ox, oy, oz], 1), region=region)


def radius2(n, radius):
    """(r, r2) of n points: radius None = +inf, one float for all, or n floats."""
    r = np.full(n, INF, F) if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, F).reshape(-1), (n,)), F)
    with np.errstate(all="ignore"):
        return r, r * r


def box_pass(p, r2, mn, mx):
    """n x N bool: node j passes for point i -- per axis e = mn - p, f = p - mx, dx = e > f ? e : f, dx = dx > 0 ? dx : 0."""
    zero = F(0.0)
    sq = []
    with np.errstate(all="ignore"):
        for a in range(3):
            e = mn[None, :, a] - p[:, None, a]
            f = p[:, None, a] - mx[None, :, a]
            dx = np.where(e > f, e, f)
            dx = np.where(dx > zero, dx, zero)
            sq.append(dx * dx)
        s0 = sq[0] + sq[1]
        b2 = s0 + sq[2]
        return ~(b2 > r2[:, None])


def walked_objects(flat, n, point_mask=None, obj_mask=None):
    """n x n_objects bool: object k is walked for point i."""
    pm = np.full(n, 0xFFFFFFFF, np.uint32) if point_mask is None else np.ascontiguousarray(point_mask, np.uint32).reshape(-1)
    om = np.full(flat.n_objects, 0xFFFFFFFF, np.uint32) if obj_mask is None else np.ascontiguousarray(obj_mask, np.uint32).reshape(-1)
    return (pm[:, None] & om[None, :]) != 0


def reached_nodes(flat, p, r, r2, walked):
    """(reach, tested), n x n_nodes bool each: reach -- the node and all its ancestors pass; tested -- the walk meets the node."""
    n, N = p.shape[0], flat.n_nodes
    passed = box_pass(p, r2, flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F))
    with np.errstate(invalid="ignore"):
        walks = r >= F(0.0)                       # (a NaN radius fails the comparison)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    reach, tested = np.zeros((n, N), bool), np.zeros((n, N), bool)
    cur = flat.obj_root.astype(np.int64)              # (every object has a root)
    tested[:, cur] = walked & walks[:, None]
    reach[:, cur] = tested[:, cur] & passed[:, cur]
    while cur.size:
        inner = cur[(left[cur] >= 0) | (right[cur] >= 0)]
        assert (left[inner] >= 0).all() and (right[inner] >= 0).all(), "a node has two children or none"
        for child in (left[inner], right[inner]):
            tested[:, child] = reach[:, inner]
            reach[:, child] = reach[:, inner] & passed[:, child]
        cur = np.concatenate([left[inner], right[inner]])
    return reach, tested


def candidate_pairs(flat, reach):
    """(point, triangle) of every candidate, sorted by point, then by triangle id (int64 each)."""
    leaf = (flat.node_left < 0) & (flat.node_right < 0)
    ri, ni = np.nonzero(reach[:, leaf])
    ni = np.flatnonzero(leaf)[ni]
    cnt = flat.node_count[ni].astype(np.int64)
    start = np.cumsum(cnt) - cnt
    within = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(start, cnt)
    pt = np.repeat(ri.astype(np.int64), cnt)
    tri = np.repeat(flat.node_first[ni].astype(np.int64), cnt) + within
    order = np.lexsort((tri, pt))
    return pt[order], tri[order]


def closest_points(flat, points, radius=None, point_mask=None, obj_mask=None, rec=None):
    """The query on `flat` for `points` (n x 3): dict of tri (n int32), dist2 (n), point (n x 3), vw (n x 2), region (n uint8), node_tests,
    tri_tests (ints; node_tests_each, tri_tests_each: per point), hits."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    rec = records_of(flat) if rec is None else np.ascontiguousarray(rec).view(F).reshape(-1, 12)
    r, r2 = radius2(n, radius)
    reach, tested = reached_nodes(flat, p, r, r2, walked_objects(flat, n, point_mask, obj_mask))
    pt, tri = candidate_pairs(flat, reach)
    out = dict(tri=np.full(n, -1, np.int32), dist2=np.full(n, INF, F), point=np.zeros((n, 3), F), vw=np.zeros((n, 2), F), region=np.zeros(n, np.uint8),
               node_tests=int(tested.sum()), tri_tests=int(pt.size), node_tests_each=tested.sum(1).astype(np.int64),
               tri_tests_each=np.bincount(pt, minlength=n).astype(np.int64))
    best = {}                                         # per chunk: the winners' rows
    for a in range(0, pt.size, PAIRS_A_CHUNK):
        ci, ct = pt[a:a + PAIRS_A_CHUNK], tri[a:a + PAIRS_A_CHUNK]
        c = closest_on_triangles(p[ci], rec[ct])
        with np.errstate(invalid="ignore"):
            ok = c["dist2"] <= r2[ci]                 # closed; a NaN fails
        ci, ct, c = ci[ok], ct[ok], {k: v[ok] for k, v in c.items()}
        best.setdefault("pt", []).append(ci); best.setdefault("tri", []).append(ct)
        for k, v in c.items():
            best.setdefault(k, []).append(v)
    if best:
        b = {k: np.concatenate(v) for k, v in best.items()}
        order = np.lexsort((b["tri"], b["dist2"], b["pt"]))
        first = order[np.r_[True, b["pt"][order][1:] != b["pt"][order][:-1]]] if order.size else order
        i = b["pt"][first]
        out["tri"][i] = b["tri"][first]; out["dist2"][i] = b["dist2"][first]; out["point"][i] = b["point"][first]
        out["vw"][i, 0] = b["v"][first]; out["vw"][i, 1] = b["w"][first]; out["region"][i] = b["region"][first]
    out["hits"] = int((out["tri"] >= 0).sum())
    return out


def brute_force(flat, points, rec=None):
    """Every triangle as a candidate of every point, radius +inf: (tri, dist2) of the winner by (dist2, id), -1 / +inf where every dist2 is NaN."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    rec = records_of(flat) if rec is None else rec
    T = rec.shape[0]
    tri, d2 = np.full(p.shape[0], -1, np.int32), np.full(p.shape[0], INF, F)
    for i in range(p.shape[0]):
        c = closest_on_triangles(np.repeat(p[i:i + 1], T, 0), rec)["dist2"]
        ok = np.flatnonzero(~np.isnan(c))
        if ok.size:
            k = ok[np.lexsort((ok, c[ok]))[0]]
            tri[i], d2[i] = k, c[k]
    return tri, d2


SAME_KEYS = ("tri", "dist2", "point", "vw", "region")


def first(want, n):
    """The yardstick's result for the first n points of its batch (a point's result and counts do not depend on the others)."""
    out = {k: want[k][:n] for k in SAME_KEYS}
    out.update(node_tests=int(want["node_tests_each"][:n].sum()), tri_tests=int(want["tri_tests_each"][:n].sum()), hits=int((want["tri"][:n] >= 0).sum()))
    return out


def same_counts(stats, want, n, what=""):
    got = (stats["primary_rays"], stats["hit_rays"], stats["node_tests_primary"], stats["tri_tests_primary"])
    assert got == (n, want["hits"], want["node_tests"], want["tri_tests"]), (what, got, (n, want["hits"], want["node_tests"], want["tri_tests"]))


def same(got, want, what=""):
    """Every output of `got` (a DeviceScene.closest_points result, or tensors brought back) against the yardstick, bit for bit."""
    for k in SAME_KEYS:
        if k not in got:
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if w.dtype == F:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} points, first {int(bad[0])}: got {got[k][bad[0]]}, want {want[k][bad[0]]}"
