"""The yardstick of the nearest-point query (include/srt_nearest.h): plain numpy float32, one array statement per operation.

  * low(p, mn, mx): item 2 of the header's definition -- the squared distance from p to the box grown by s = K 2^-24 M on every side,
    times (1 - 2^-20) -- and prunes(low, best): `low > best && low < +inf`;
  * deficit(...): (sqrt(b2 of a triangle's tight box) - sqrt(dist2)) / (2^-24 M), the quantity K is fixed from;
  * margin_holds(flat, points): property (c), low(tight box of T, p) <= dist2(T, p), on every (point, triangle) pair of a scene, and the
    scene's boxes nest;
  * shrinking_walk(...): the walk simulated point by point in the device's node order (pre-order, object by object), the bound moving at
    once or a number of triangle tests late -- the device's moves when the wave's queue flushes; whatever the delay, the outputs are
    tests/point_ref.closest_points';
  * mandatory(...): the least any such walk tests -- the nodes all of whose ancestors pass the radius test with low <= the final dist2,
    and the triangles of such leaves."""
import numpy as np

import point_ref as pr
from simple_raytracer_amd import abi

F = np.float32
INF = F(np.inf)
K = abi.NEAREST_K
U = 2.0 ** -24
REL = F(1.0) - F(2.0 ** -20)


def box_axes(p, mn, mx):
    """(dx, dy, dz) of the box test, for p (..., 3) against mn, mx (..., 3), broadcast."""
    zero = F(0.0)
    out = []
    with np.errstate(all="ignore"):
        for a in range(3):
            e = mn[..., a] - p[..., a]
            f = p[..., a] - mx[..., a]
            dx = np.where(e > f, e, f)
            dx = np.where(dx > zero, dx, zero)
            out.append(dx.astype(F))
    return out


def scale(p, mn, mx):
    """M and z of the header: the largest of the nine |coordinates| (a NaN is passed over), and 0 or NaN."""
    nine = np.broadcast_arrays(*([np.abs(mn[..., a]) for a in range(3)] + [np.abs(mx[..., a]) for a in range(3)] + [np.abs(p[..., a]) for a in range(3)]))
    M = nine[0]
    finite = np.isfinite(nine[0])
    for v in nine[1:]:
        M = np.fmax(M, v)
        finite = finite & np.isfinite(v)
    return M.astype(F), np.where(finite, F(0.0), F(np.nan)).astype(F)


def low(p, mn, mx, k=K, rel=True):
    """(b2, low) float32.  k = 0 and rel = False is the mutant: low = b2."""
    p, mn, mx = (np.asarray(a, F) for a in (p, mn, mx))
    zero = F(0.0)
    dx, dy, dz = box_axes(p, mn, mx)
    with np.errstate(all="ignore"):
        sx = dx * dx; sy = dy * dy; sz = dz * dz
        b0 = sx + sy
        b2 = b0 + sz
        M, z = scale(p, mn, mx)
        c = F(k * U)                                  # exact: k is a power of two (or 0)
        s0 = c * M
        s = s0 + z
        tx = dx - s; ty = dy - s; tz = dz - s
        tx = np.where(tx > zero, tx, zero); ty = np.where(ty > zero, ty, zero); tz = np.where(tz > zero, tz, zero)
        qx = tx * tx; qy = ty * ty; qz = tz * tz
        l0 = qx + qy
        l1 = l0 + qz
        lo = l1 * REL if rel else l1
    assert b2.dtype == F and lo.dtype == F
    return b2, lo


def prunes(lo, best):
    with np.errstate(invalid="ignore"):
        return (lo > best) & (lo < INF)


def tight_boxes(tri_points):
    """(mn, mx), n x 3 each: the box of each triangle's three vertices (raw xyz)."""
    P = np.ascontiguousarray(tri_points, F).reshape(-1, 3, 4)[..., :3]
    with np.errstate(invalid="ignore"):
        return P.min(1), P.max(1)


def deficit(p, rec, mn, mx, k=K):
    """(sqrt(b2) - sqrt(dist2)) / (2^-24 M) per pair in float64 (NaN where dist2 or b2 is not finite), dist2, and low at k."""
    d2 = pr.closest_on_triangles(p, rec)["dist2"]
    b2, lo = low(p, mn, mx, k)
    M, _ = scale(p, mn, mx)
    with np.errstate(all="ignore"):
        d = (np.sqrt(b2.astype(np.float64)) - np.sqrt(d2.astype(np.float64))) / (U * M.astype(np.float64))
    return np.where(np.isfinite(d2) & np.isfinite(b2), d, np.nan), d2, lo


def contains(amn, amx, bmn, bmx):
    """Box a contains box b (an empty b, mn > mx on an axis, is contained in anything)."""
    with np.errstate(invalid="ignore"):
        return ((amn <= bmn) & (amx >= bmx)).all(-1) | (bmn > bmx).any(-1)


def nests(flat):
    """Every inner node's box contains its children's, every leaf's box the vertices of its triangles (a triangle with a NaN is exempt:
    its dist2 is a NaN and it never wins)."""
    mn, mx = flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    inner = np.flatnonzero(left >= 0)
    ok = contains(mn[inner], mx[inner], mn[left[inner]], mx[left[inner]]).all() and contains(mn[inner], mx[inner], mn[right[inner]], mx[right[inner]]).all()
    tmn, tmx = tight_boxes(flat.tri_points)
    for i in np.flatnonzero((left < 0) & (flat.node_count > 0)):
        f, c = int(flat.node_first[i]), int(flat.node_count[i])
        clean = ~(np.isnan(tmn[f:f + c]).any(1) | np.isnan(tmx[f:f + c]).any(1))
        ok = ok and bool(contains(mn[i], mx[i], tmn[f:f + c][clean], tmx[f:f + c][clean]).all())
    return bool(ok)


def margin_holds(flat, points, k=K, rec=None, chunk=1 << 20):
    """(holds, pairs that fail property (c), worst deficit in 2^-24 M): every (point, triangle) pair of the scene against the triangle's
    tight box; holds also needs nests(flat)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    rec = pr.records_of(flat) if rec is None else rec
    tmn, tmx = tight_boxes(flat.tri_points)
    T = rec.shape[0]
    bad, worst = 0, -np.inf
    per = max(1, chunk // max(T, 1))
    for a in range(0, p.shape[0], per):
        q = np.repeat(p[a:a + per], T, 0)
        t = np.tile(np.arange(T), p[a:a + per].shape[0])
        d, d2, lo = deficit(q, rec[t], tmn[t], tmx[t], k)
        with np.errstate(invalid="ignore"):
            bad += int((~np.isnan(d2) & ~(lo <= d2)).sum())
        if np.isfinite(d).any():
            worst = max(worst, float(np.nanmax(d)))
    return nests(flat) and bad == 0, bad, worst


def low_on_the_way_down(flat, p, k=K):
    """points x nodes: the largest low(box, p) over a node and its ancestors."""
    mn, mx = flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F)
    _, lo = low(p[:, None, :], mn[None], mx[None], k)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    cur = flat.obj_root.astype(np.int64)
    while cur.size:
        inner = cur[left[cur] >= 0]
        for child in (left[inner], right[inner]):
            lo[:, child] = np.maximum(lo[:, child], lo[:, inner])
        cur = np.concatenate([left[inner], right[inner]])
    return lo


def ancestors_hold(flat, points, k=K, rec=None):
    """What (a) and (c) are there to give, checked directly and without assuming that boxes nest: for every point and every triangle T
    whose dist2 is not NaN, low(box, p) <= dist2(T, p) for the box of T's leaf and of every ancestor.  Returns the pairs that fail."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    rec = pr.records_of(flat) if rec is None else rec
    lo = low_on_the_way_down(flat, p, k)
    bad = 0
    for i in np.flatnonzero((flat.node_left < 0) & (flat.node_count > 0)):
        f, c = int(flat.node_first[i]), int(flat.node_count[i])
        d2 = pr.closest_on_triangles(np.repeat(p, c, 0), np.tile(rec[f:f + c], (p.shape[0], 1)))["dist2"].reshape(p.shape[0], c)
        with np.errstate(invalid="ignore"):
            bad += int((~np.isnan(d2) & ~(lo[:, i][:, None] <= d2)).sum())
    return bad


def winners_hold(flat, points, want, k=K):
    """The second precondition alone, on any tree: the points whose winner W (want["tri"], want["dist2"]) has a leaf or an ancestor with
    low(box, p) > dist2(W, p).  For every other point the shrinking walk cannot lose W, whatever else the scene holds."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    lo = low_on_the_way_down(flat, p, k)
    leaf_of = np.full(flat.n_tris, -1, np.int64)
    for i in np.flatnonzero((flat.node_left < 0) & (flat.node_count > 0)):
        leaf_of[int(flat.node_first[i]):int(flat.node_first[i]) + int(flat.node_count[i])] = i
    hit = np.flatnonzero(want["tri"] >= 0)
    over = lo[hit, leaf_of[want["tri"][hit]]] > want["dist2"][hit]
    return hit[over]


def preorder(flat, walked_objects):
    """The device's node order for one point: the objects it walks in their order, each root, left subtree, right subtree.  Yields lists
    (node, end) where `end` is the position after the node's subtree (its skip link)."""
    order, end = [], []
    for k in walked_objects:
        stack = [int(flat.obj_root[k])]
        opened = []
        while stack:
            i = stack.pop()
            if i < 0:                                 # the marker after a subtree: its root's skip link is here
                end[opened.pop()] = len(order)
                continue
            opened.append(len(order)); order.append(i); end.append(-1)
            stack.append(-1)
            if flat.node_left[i] >= 0:
                stack.append(int(flat.node_right[i])); stack.append(int(flat.node_left[i]))
    return order, end


def shrinking_walk(flat, points, radius=None, point_mask=None, obj_mask=None, max_delay=0, seed=0, order=None, k=K, rel=True, rec=None):
    """The shrinking walk, point by point (in `order`, which only moves the random delays): the result dict of point_ref.closest_points
    with the walk's own node_tests / tri_tests (+ _each).  max_delay: every offer reaches the bound a random number of this point's
    triangle tests later, 0 .. max_delay (0: at once)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    rec = pr.records_of(flat) if rec is None else rec
    r, r2 = pr.radius2(n, radius)
    walked = pr.walked_objects(flat, n, point_mask, obj_mask)
    mn, mx = flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F)
    is_leaf = flat.node_left < 0
    rng = np.random.default_rng(seed)
    out = dict(tri=np.full(n, -1, np.int32), dist2=np.full(n, INF, F), point=np.zeros((n, 3), F), vw=np.zeros((n, 2), F), region=np.zeros(n, np.uint8),
               node_tests_each=np.zeros(n, np.int64), tri_tests_each=np.zeros(n, np.int64))
    plans = {}
    for i in (range(n) if order is None else order):
        with np.errstate(invalid="ignore"):
            if not r[i] >= F(0.0):
                continue
        key = walked[i].tobytes()
        if key not in plans:
            plans[key] = preorder(flat, np.flatnonzero(walked[i]))
        nodes, end = plans[key]
        b2, lo = low(p[i][None, :], mn, mx, k, rel)
        with np.errstate(invalid="ignore"):
            fails = (b2 > r2[i]).tolist()
        lo = lo.tolist()
        best_seen, pending, tests = float("nan"), [], 0          # (NaN: no bound yet -- `low > NaN` is false)
        win = (float("inf"), -1)
        at = 0
        while at < len(nodes):
            while pending and pending[0][0] <= tests:
                d = pending.pop(0)[1]
                if not best_seen <= d:
                    best_seen = d
            j = nodes[at]
            out["node_tests_each"][i] += 1
            if fails[j] or (lo[j] > best_seen and lo[j] < float("inf")):
                at = end[at]
                continue
            if is_leaf[j] and flat.node_count[j] > 0:
                f, c = int(flat.node_first[j]), int(flat.node_count[j])
                d2 = pr.closest_on_triangles(np.repeat(p[i][None, :], c, 0), rec[f:f + c])["dist2"]
                tests += c
                out["tri_tests_each"][i] += c
                with np.errstate(invalid="ignore"):
                    ok = np.flatnonzero(d2 <= r2[i])
                for t in ok:
                    cand = (float(d2[t]), f + int(t))
                    if cand < win or win[1] < 0:
                        win = cand
                    pending.append((tests + (int(rng.integers(0, max_delay + 1)) if max_delay else 0), cand[0]))
                pending.sort(key=lambda e: e[0])
            at += 1
        if win[1] >= 0:
            c = pr.closest_on_triangles(p[i][None, :], rec[win[1]][None, :])
            out["tri"][i] = win[1]; out["dist2"][i] = c["dist2"][0]; out["point"][i] = c["point"][0]
            out["vw"][i] = (c["v"][0], c["w"][0]); out["region"][i] = c["region"][0]
    out["node_tests"], out["tri_tests"] = int(out["node_tests_each"].sum()), int(out["tri_tests_each"].sum())
    out["hits"] = int((out["tri"] >= 0).sum())
    return out


def mandatory(flat, points, final_d2, radius=None, point_mask=None, obj_mask=None, k=K):
    """(node tests, triangle tests) per point that no shrinking walk can avoid, given the final dist2 of each point (+inf: none found)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    r, r2 = pr.radius2(n, radius)
    mn, mx = flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F)
    b2, lo = low(p[:, None, :], mn[None], mx[None], k)
    with np.errstate(invalid="ignore"):
        opened = ~(b2 > r2[:, None]) & ~prunes(lo, np.asarray(final_d2, F)[:, None])
        walks = r >= F(0.0)
    walked = pr.walked_objects(flat, n, point_mask, obj_mask)
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    reach, tested = np.zeros((n, flat.n_nodes), bool), np.zeros((n, flat.n_nodes), bool)
    cur = flat.obj_root.astype(np.int64)
    tested[:, cur] = walked & walks[:, None]
    reach[:, cur] = tested[:, cur] & opened[:, cur]
    while cur.size:
        inner = cur[left[cur] >= 0]
        for child in (left[inner], right[inner]):
            tested[:, child] = reach[:, inner]
            reach[:, child] = reach[:, inner] & opened[:, child]
        cur = np.concatenate([left[inner], right[inner]])
    leaf = left < 0
    tris = (reach[:, leaf] * flat.node_count[leaf].astype(np.int64)[None, :]).sum(1)
    return tested.sum(1).astype(np.int64), tris.astype(np.int64)
