"""The yardstick of the segment query (include/srt_segments.h): plain numpy float32, one array statement per operation, in the header's
association.

  * the records, the closest point on a triangle, the walk order (reachability pushed down each object's tree) and the candidate pairs are
    tests/point_ref.py's, with the segment's node test -- box test 1, and box test 2 for sloped segments with a finite radius -- in the
    place of the point's;
  * the crossing's t is the ray yardstick's triangle test, oracle.ray_triangle, as tests/ray_range_ref.py uses it, on the ray (A, B - A);
  * the triangle function: candidates 0 .. 4 as a running minimum in the header's order and with the header's replacement rule, then the
    crossing; the winner by lexsort((tri, dist2, segment)) among the triangles with dist2 <= r2;
  * both work counts as point_ref counts them.

STAGE2 = False (or stage2=False) leaves box test 2 out: tests/test_segment_ref.py shows that the walk loses nothing either way."""
import numpy as np

import point_ref as pr
from oracle import pyoracle

F = np.float32
INF = F(np.inf)
PAIRS_A_CHUNK = 1 << 19
STAGE2 = True
SAME_KEYS = ("tri", "dist2", "s", "point", "vw", "feature")


def split(segments):
    """(A, B, d) of n x 6 segments, float32; d = B - A."""
    seg = np.ascontiguousarray(segments, F).reshape(-1, 6)
    A = np.ascontiguousarray(seg[:, :3]); B = np.ascontiguousarray(seg[:, 3:])
    with np.errstate(all="ignore"):
        d = B - A
    return A, B, d


def is_point(d):
    return (d[:, 0] == 0) & (d[:, 1] == 0) & (d[:, 2] == 0)


def clamp(x):
    zero, one = F(0.0), F(1.0)
    return np.where(x < zero, zero, np.where(x > one, one, x)).astype(F)


def edge_candidate(A, d, a, origin, dr):
    """The segment (A, d) against the edge (origin, dr), Ericson 5.1.9: (s, u, dist2), float32 each."""
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        rx = A[:, 0] - origin[:, 0]; ry = A[:, 1] - origin[:, 1]; rz = A[:, 2] - origin[:, 2]
        e = pr.dot(dr[:, 0], dr[:, 1], dr[:, 2], dr[:, 0], dr[:, 1], dr[:, 2])
        f = pr.dot(dr[:, 0], dr[:, 1], dr[:, 2], rx, ry, rz)
        c = pr.dot(d[:, 0], d[:, 1], d[:, 2], rx, ry, rz)
        b = pr.dot(d[:, 0], d[:, 1], d[:, 2], dr[:, 0], dr[:, 1], dr[:, 2])
        nc = -c
        s_a = clamp(nc / a)                       # clamp((-c) / a)
        bc = b - c
        s_b = clamp(bc / a)                       # clamp((b - c) / a)
        ae = a * e; bb = b * b; den = ae - bb
        bf = b * f; ce = c * e; num = bf - ce
        s0 = np.where(den > zero, clamp(num / den), zero).astype(F)
        bs = b * s0; bsf = bs + f; u0 = bsf / e
        low = u0 < zero
        high = ~low & (u0 > one)
        u1 = np.where(low, zero, np.where(high, one, u0)).astype(F)
        s1 = np.where(low, s_a, np.where(high, s_b, s0)).astype(F)
        flat = e == zero
        u = np.where(flat, zero, u1).astype(F)
        s = np.where(flat, s_a, s1).astype(F)
        comp = []
        for k in range(3):
            ds = d[:, k] * s; on_seg = A[:, k] + ds
            du = dr[:, k] * u; on_edge = origin[:, k] + du
            comp.append(on_seg - on_edge)
        dist2 = pr.dot(comp[0], comp[1], comp[2], comp[0], comp[1], comp[2])
    assert s.dtype == F and u.dtype == F and dist2.dtype == F
    return s, u, dist2


def replaces(new, old):
    """The header's rule: dist2_k < dist2 || (dist2 != dist2 && dist2_k == dist2_k)."""
    with np.errstate(invalid="ignore"):
        return (new < old) | ((old != old) & (new == new))


def segment_on_triangles(A, B, rec, tri_pts):
    """Segment k against record rec[k] (m x 12 float32; tri_pts: the same triangles' points, m x 12, for the ray test): dict of dist2, s,
    v, w (m float32), point (m x 3), feature (m uint8), t (the ray test's result)."""
    A = np.ascontiguousarray(A, F).reshape(-1, 3); B = np.ascontiguousarray(B, F).reshape(-1, 3)
    rec = np.ascontiguousarray(rec, F).reshape(-1, 12)
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        d = B - A
        point_seg = is_point(d)
        c0 = pr.closest_on_triangles(A, rec)
        dist2, s, v, w = c0["dist2"].copy(), np.zeros(len(A), F), c0["v"].copy(), c0["w"].copy()
        feature = np.zeros(len(A), np.uint8)
        c1 = pr.closest_on_triangles(B, rec)
        take = replaces(c1["dist2"], dist2) & ~point_seg
        dist2 = np.where(take, c1["dist2"], dist2); s = np.where(take, one, s).astype(F); v = np.where(take, c1["v"], v); w = np.where(take, c1["w"], w)
        feature = np.where(take, 1, feature).astype(np.uint8)
        P1, e1, e2 = rec[:, 0:3], rec[:, 3:6], rec[:, 6:9]
        a = pr.dot(d[:, 0], d[:, 1], d[:, 2], d[:, 0], d[:, 1], d[:, 2])
        p2 = P1 + e1
        e21 = e2 - e1
        for k, (origin, dr) in enumerate(((P1, e1), (p2, e21), (P1, e2))):
            sk, u, dk = edge_candidate(A, d, a, origin, dr)
            zeros = np.zeros_like(u)
            vk, wk = ((u, zeros), (one - u, u), (zeros, u))[k]
            take = replaces(dk, dist2) & ~point_seg
            dist2 = np.where(take, dk, dist2); s = np.where(take, sk, s); v = np.where(take, vk, v).astype(F); w = np.where(take, wk, w).astype(F)
            feature = np.where(take, 2 + k, feature).astype(np.uint8)
        t = pyoracle.ray_triangle(np.concatenate([A, d], 1), np.ascontiguousarray(tri_pts, F).reshape(-1, 12)) if len(A) else np.empty(0, F)
        cross = (t != -INF) & (t >= zero) & (t <= one) & ~point_seg
        if cross.any():
            tc = t[cross]
            px = A[cross, 0] + d[cross, 0] * tc; py = A[cross, 1] + d[cross, 1] * tc; pz = A[cross, 2] + d[cross, 2] * tc
            c5 = pr.closest_on_triangles(np.stack([px, py, pz], 1), rec[cross])
            dist2[cross] = zero; s[cross] = tc; v[cross] = c5["v"]; w[cross] = c5["w"]; feature[cross] = 5
        comp = []
        for k in range(3):
            q0 = e1[:, k] * v; q1 = e2[:, k] * w; q = q0 + q1
            comp.append(P1[:, k] + q)
    out = dict(dist2=dist2.astype(F), s=s.astype(F), v=v.astype(F), w=w.astype(F), point=np.stack(comp, 1).astype(F), feature=feature, t=t)
    assert all(out[k].dtype == F for k in ("dist2", "s", "v", "w", "point"))
    return out


def sloped(d):
    """(sloped, inv): every d_k finite and not 0, and inv_k = 1 / d_k finite."""
    with np.errstate(all="ignore"):
        inv = F(1.0) / d
        return (np.isfinite(d) & (d != 0) & np.isfinite(inv)).all(1), inv


def node_pass(A, B, r, r2, mn, mx, stage2=None):
    """n x N bool: node j passes both box tests for segment i."""
    stage2 = STAGE2 if stage2 is None else stage2
    zero, one = F(0.0), F(1.0)
    with np.errstate(all="ignore"):
        d = B - A
        sq = []
        for k in range(3):
            a, b = A[:, None, k], B[:, None, k]
            lo = np.where(a < b, a, b); hi = np.where(a < b, b, a)
            e = mn[None, :, k] - hi
            f = lo - mx[None, :, k]
            g = np.where(e > f, e, f)
            g = np.where(g > zero, g, zero)
            sq.append(g * g)
        s0 = sq[0] + sq[1]
        b2 = s0 + sq[2]
        ok = ~(b2 > r2[:, None])
        if not stage2:
            return ok
        slab, inv = sloped(d)
        slab &= r < INF
        near = np.zeros(ok.shape, F); far = np.ones(ok.shape, F); nan = np.zeros(ok.shape, bool)
        for k in range(3):
            lo_box = mn[None, :, k] - r[:, None]; t0 = (lo_box - A[:, None, k]) * inv[:, None, k]
            hi_box = mx[None, :, k] + r[:, None]; t1 = (hi_box - A[:, None, k]) * inv[:, None, k]
            tn = np.where(t0 < t1, t0, t1); tf = np.where(t0 < t1, t1, t0)
            near = np.where(tn > near, tn, near); far = np.where(tf < far, tf, far)
            nan |= np.isnan(t0) | np.isnan(t1)
        fails2 = (near > far) & ~nan & slab[:, None]
        return ok & ~fails2


def reached_nodes(flat, A, B, r, r2, walked, stage2=None):
    """(reach, tested), n x n_nodes bool each, as point_ref.reached_nodes with the segment's node test."""
    n, N = A.shape[0], flat.n_nodes
    passed = node_pass(A, B, r, r2, flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F), stage2)
    with np.errstate(invalid="ignore"):
        walks = r >= F(0.0)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    reach, tested = np.zeros((n, N), bool), np.zeros((n, N), bool)
    cur = flat.obj_root.astype(np.int64)
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


def tri_points_of(flat):
    return np.ascontiguousarray(flat.tri_points, F).reshape(-1, 12)


def evaluate(flat, A, B, r2, sg, tri, rec=None):
    """The qualifying (segment, triangle) pairs among (sg, tri) with their results: dict of sg, tri, dist2, s, v, w, point, feature."""
    rec = pr.records_of(flat) if rec is None else rec
    pts = tri_points_of(flat)
    keep = {}
    for a in range(0, sg.size, PAIRS_A_CHUNK):
        ci, ct = sg[a:a + PAIRS_A_CHUNK], tri[a:a + PAIRS_A_CHUNK]
        c = segment_on_triangles(A[ci], B[ci], rec[ct], pts[ct])
        with np.errstate(invalid="ignore"):
            ok = c["dist2"] <= r2[ci]                 # closed; a NaN fails
        keep.setdefault("sg", []).append(ci[ok]); keep.setdefault("tri", []).append(ct[ok])
        for k, val in c.items():
            keep.setdefault(k, []).append(val[ok])
    return {k: np.concatenate(val) for k, val in keep.items()} if keep else None


def winners(n, b):
    """The winner per segment among the qualifying pairs `b` (evaluate): the header's outputs."""
    out = dict(tri=np.full(n, -1, np.int32), dist2=np.full(n, INF, F), s=np.zeros(n, F), point=np.zeros((n, 3), F), vw=np.zeros((n, 2), F),
               feature=np.zeros(n, np.uint8))
    if b is not None and b["sg"].size:
        order = np.lexsort((b["tri"], b["dist2"], b["sg"]))
        first = order[np.r_[True, b["sg"][order][1:] != b["sg"][order][:-1]]]
        i = b["sg"][first]
        out["tri"][i] = b["tri"][first]; out["dist2"][i] = b["dist2"][first]; out["s"][i] = b["s"][first]; out["point"][i] = b["point"][first]
        out["vw"][i, 0] = b["v"][first]; out["vw"][i, 1] = b["w"][first]; out["feature"][i] = b["feature"][first]
    out["hits"] = int((out["tri"] >= 0).sum())
    return out


def walk(flat, segments, radius=None, seg_mask=None, obj_mask=None, stage2=None):
    """The walk alone: (A, B, r2, the candidates as (segment, triangle), tested: n x n_nodes bool)."""
    A, B, _ = split(segments)
    n = A.shape[0]
    r, r2 = pr.radius2(n, radius)
    reach, tested = reached_nodes(flat, A, B, r, r2, pr.walked_objects(flat, n, seg_mask, obj_mask), stage2)
    sg, tri = pr.candidate_pairs(flat, reach)
    return A, B, r2, sg, tri, tested


def closest_segments(flat, segments, radius=None, seg_mask=None, obj_mask=None, stage2=None, rec=None):
    """The query on `flat` for `segments` (n x 6): dict of tri (n int32), dist2, s (n), point (n x 3), vw (n x 2), feature (n uint8),
    node_tests, tri_tests (ints; node_tests_each, tri_tests_each: per segment), hits, `pairs`: the candidates as (segment, triangle), and
    `qualifying`: those with dist2 <= r2, with their results (evaluate)."""
    A, B, r2, sg, tri, tested = walk(flat, segments, radius, seg_mask, obj_mask, stage2)
    n = A.shape[0]
    b = evaluate(flat, A, B, r2, sg, tri, rec)
    out = winners(n, b)
    out.update(qualifying=b, node_tests=int(tested.sum()), tri_tests=int(sg.size), node_tests_each=tested.sum(1).astype(np.int64),
               tri_tests_each=np.bincount(sg, minlength=n).astype(np.int64), pairs=(sg, tri))
    return out


def brute_force(flat, segments, radius=None):
    """Every triangle as a candidate of every segment, no walk: (the winners, the qualifying pairs with their results)."""
    A, B, _ = split(segments)
    n, T = A.shape[0], flat.n_tris
    _, r2 = pr.radius2(n, radius)
    sg = np.repeat(np.arange(n, dtype=np.int64), T); tri = np.tile(np.arange(T, dtype=np.int64), n)
    b = evaluate(flat, A, B, r2, sg, tri)
    return winners(n, b), b


def first(want, n):
    """The yardstick's result for the first n segments of its batch (a segment's result and counts do not depend on the others)."""
    out = {k: want[k][:n] for k in SAME_KEYS}
    out.update(node_tests=int(want["node_tests_each"][:n].sum()), tri_tests=int(want["tri_tests_each"][:n].sum()), hits=int((want["tri"][:n] >= 0).sum()))
    return out


same_counts = pr.same_counts


def same(got, want, what="", keys=SAME_KEYS, nan_equal=False):
    """Every output of `got` (a DeviceScene.closest_segments result, or tensors brought back) against the yardstick, bit for bit.
    nan_equal: a NaN on both sides counts as equal whatever its payload (tests/refit_edges.py's rule)."""
    for k in keys:
        if k not in got:
            continue
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        if w.dtype == F:
            both_nan = np.isnan(g) & np.isnan(w) if nan_equal else np.zeros(g.shape, bool)
            diff = (g.view(np.uint32) != w.view(np.uint32)) & ~both_nan
        else:
            diff = g != w
        bad = np.flatnonzero(diff.reshape(g.shape[0], -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} segments, first {int(bad[0])}: got {got[k][bad[0]]}, want {want[k][bad[0]]}"
