"""The yardstick of the K-nearest-triangles queries (include/srt_points_multi.h).  It has no walk of its own:

  * candidates(...): tests/point_ref.py's reached set (reached_nodes, candidate_pairs) and its closest_on_triangles on every pair, every
    candidate with dist2 <= r2 kept, sorted by lexsort((tri, dist2, point)) -- the closest form's definition, for every k at once -- with
    point_ref's two work counts;
  * columns(cand, k): the first k candidates per point as the n x k outputs, n_within, n_found;
  * mandatory(...): tests/nearest_ref.mandatory evaluated at each point's k-th dist2 (+inf where fewer than k are found: only the radius
    bounds then) -- the least the nearest form tests;
  * shrinking_walk(...): nearest_ref.shrinking_walk with k slots: offers reach the slots a random number of triangle tests late, and the
    bound is read from slot k - 1 alone (a NaN while it is empty)."""
import bisect

import numpy as np

import nearest_ref as nr
import point_ref as pr

F = np.float32
INF = F(np.inf)
SAME_KEYS = ("n_within", "n_found", "tri", "dist2", "point", "vw", "region")
COLUMN_KEYS = SAME_KEYS[2:]


def candidates(flat, points, radius=None, point_mask=None, obj_mask=None, rec=None):
    """Every qualifying candidate of every point, sorted by (point, dist2, tri): dict of pt, tri (int64), dist2, v, w (float32), point
    (m x 3), region (uint8), rank (its place among its point's), n (points), and point_ref's counts (node_tests_each, tri_tests_each)."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    rec = pr.records_of(flat) if rec is None else np.ascontiguousarray(rec).view(F).reshape(-1, 12)
    r, r2 = pr.radius2(n, radius)
    reach, tested = pr.reached_nodes(flat, p, r, r2, pr.walked_objects(flat, n, point_mask, obj_mask))
    pt, tri = pr.candidate_pairs(flat, reach)
    kept = dict(pt=[np.zeros(0, np.int64)], tri=[np.zeros(0, np.int64)], dist2=[np.zeros(0, F)], v=[np.zeros(0, F)], w=[np.zeros(0, F)],
                point=[np.zeros((0, 3), F)], region=[np.zeros(0, np.uint8)])
    for a in range(0, pt.size, pr.PAIRS_A_CHUNK):
        ci, ct = pt[a:a + pr.PAIRS_A_CHUNK], tri[a:a + pr.PAIRS_A_CHUNK]
        c = pr.closest_on_triangles(p[ci], rec[ct])
        with np.errstate(invalid="ignore"):
            ok = c["dist2"] <= r2[ci]                     # closed; a NaN fails
        kept["pt"].append(ci[ok]); kept["tri"].append(ct[ok])
        for key, v in c.items():
            kept[key].append(v[ok])
    b = {key: np.concatenate(v) for key, v in kept.items()}
    order = np.lexsort((b["tri"], b["dist2"], b["pt"]))
    b = {key: v[order] for key, v in b.items()}
    within = np.bincount(b["pt"], minlength=n).astype(np.int64)
    b["rank"] = np.arange(b["pt"].size, dtype=np.int64) - np.repeat(np.cumsum(within) - within, within)
    b.update(n=n, n_within=within, node_tests_each=tested.sum(1).astype(np.int64), tri_tests_each=np.bincount(pt, minlength=n).astype(np.int64))
    return b


def columns(cand, k):
    """The closest form's result for k columns: n_within, n_found (n uint32), tri, dist2, region (n x k), point (n x k x 3), vw (n x k x 2),
    the counts (node_tests, tri_tests, _each) and hits, the points with n_found > 0."""
    n = cand["n"]
    out = dict(n_within=cand["n_within"].astype(np.uint32), n_found=np.minimum(cand["n_within"], k).astype(np.uint32), tri=np.full((n, k), -1, np.int32),
               dist2=np.full((n, k), INF, F), point=np.zeros((n, k, 3), F), vw=np.zeros((n, k, 2), F), region=np.zeros((n, k), np.uint8),
               node_tests_each=cand["node_tests_each"], tri_tests_each=cand["tri_tests_each"])
    first = cand["rank"] < k
    i, j = cand["pt"][first], cand["rank"][first]
    out["tri"][i, j] = cand["tri"][first]; out["dist2"][i, j] = cand["dist2"][first]; out["point"][i, j] = cand["point"][first]
    out["vw"][i, j, 0] = cand["v"][first]; out["vw"][i, j, 1] = cand["w"][first]; out["region"][i, j] = cand["region"][first]
    out.update(node_tests=int(out["node_tests_each"].sum()), tri_tests=int(out["tri_tests_each"].sum()), hits=int((out["n_found"] > 0).sum()))
    return out


def closest_points_multi(flat, points, k, radius=None, point_mask=None, obj_mask=None, rec=None):
    return columns(candidates(flat, points, radius, point_mask, obj_mask, rec), k)


def first(want, n):
    """The yardstick's result for the first n points of its batch (a point's result and counts do not depend on the others)."""
    out = {key: want[key][:n] for key in SAME_KEYS}
    out.update(node_tests=int(want["node_tests_each"][:n].sum()), tri_tests=int(want["tri_tests_each"][:n].sum()), hits=int((want["n_found"][:n] > 0).sum()),
               node_tests_each=want["node_tests_each"][:n], tri_tests_each=want["tri_tests_each"][:n])
    return out


def rows(want, index):
    """The rows `index` (a permutation, a slice, a mask) of a result, outputs only."""
    return {key: want[key][index] for key in SAME_KEYS if key in want}


def same(got, want, what="", keys=SAME_KEYS):
    """Every output of `got` (a DeviceScene.*_points_multi result, or tensors brought back) that `want` has too, bit for bit."""
    for key in keys:
        if key not in got or key not in want:
            continue
        g, w = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, key, g.shape, w.shape, g.dtype, w.dtype)
        if w.dtype == F:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(g.shape[0], -1).any(1))
        assert bad.size == 0, f"{what}: {key} differs at {bad.size} points, first {int(bad[0])}: got {got[key][bad[0]]}, want {want[key][bad[0]]}"


def same_counts(stats, want, n, what=""):
    got = (stats["primary_rays"], stats["hit_rays"], stats["node_tests_primary"], stats["tri_tests_primary"])
    assert got == (n, want["hits"], want["node_tests"], want["tri_tests"]), (what, got, (n, want["hits"], want["node_tests"], want["tri_tests"]))


def kth_dist2(want, k):
    """Per point the dist2 of column k - 1: the final bound of the nearest form, +inf where fewer than k are found."""
    return np.ascontiguousarray(want["dist2"][:, k - 1])


def mandatory(flat, points, want, k, radius=None, point_mask=None, obj_mask=None):
    """(node tests, triangle tests) per point that no walk of the nearest form can avoid."""
    return nr.mandatory(flat, points, kth_dist2(want, k), radius, point_mask=point_mask, obj_mask=obj_mask)


def own_outputs(flat, points, got, rec=None):
    """What the header promises of every filled column on ANY tree: the returned triangle's own dist2, point, vw and region (recomputed here),
    the columns sorted by (dist2, id) and distinct, the empty columns after the filled ones and n_found their number."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    rec = pr.records_of(flat) if rec is None else rec
    tri = got["tri"]
    n, k = tri.shape
    filled = tri >= 0
    assert np.array_equal(got["n_found"], filled.sum(1).astype(np.uint32)) and (filled[:, :-1] >= filled[:, 1:]).all()
    i, j = np.nonzero(filled)
    own = pr.closest_on_triangles(p[i], rec[tri[i, j]])
    want = dict(got, dist2=np.full((n, k), INF, F), point=np.zeros((n, k, 3), F), vw=np.zeros((n, k, 2), F), region=np.zeros((n, k), np.uint8))
    want["dist2"][i, j] = own["dist2"]; want["point"][i, j] = own["point"]; want["vw"][i, j, 0] = own["v"]; want["vw"][i, j, 1] = own["w"]
    want["region"][i, j] = own["region"]
    same(got, want, "own outputs", COLUMN_KEYS)
    both = filled[:, :-1] & filled[:, 1:]
    a, b = got["dist2"][:, :-1], got["dist2"][:, 1:]
    assert (~both | (a < b) | ((a == b) & (tri[:, :-1] < tri[:, 1:]))).all(), "sorted by (dist2, id), distinct"


def tie_batch(flat):
    """The batch of ties on a cube mesh: its eight vertices exactly, and the midpoints of the three edges at the first vertex.  A vertex is
    shared by several triangles at dist2 = 0, an edge by two; all of them are reported, lowest id first."""
    P = np.unique(np.ascontiguousarray(flat.tri_points, F).reshape(-1, 4)[:, :3], axis=0)
    assert len(P) == 8, "a cube"
    import itertools
    d = P[1:].astype(np.float64) - P[0].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # the three vertices an edge away: the one triple of mutually orthogonal directions (a face or space diagonal is orthogonal to at most one edge)
    best = min(itertools.combinations(range(7), 3), key=lambda t: abs(d[t[0]] @ d[t[1]]) + abs(d[t[0]] @ d[t[2]]) + abs(d[t[1]] @ d[t[2]]))
    ends = P[1:][list(best)]
    mids = ((P[0][None, :] + ends) * F(0.5)).astype(F)
    return np.concatenate([P, mids]).astype(F)


def equal_runs(want):
    """Per point the longest run of filled columns with equal dist2 bits; the ids inside a run of equal dist2 ascend (asserted)."""
    d2, tri = want["dist2"].view(np.uint32), want["tri"]
    filled = tri >= 0
    eq = (d2[:, 1:] == d2[:, :-1]) & filled[:, 1:] & filled[:, :-1]
    assert (tri[:, 1:][eq] > tri[:, :-1][eq]).all()
    best = np.zeros(len(tri), np.int64)
    run = filled[:, 0].astype(np.int64)
    best = np.maximum(best, run)
    for j in range(1, tri.shape[1]):
        run = np.where(eq[:, j - 1], run + 1, filled[:, j].astype(np.int64))
        best = np.maximum(best, run)
    return best


def shrinking_walk(flat, points, k,radius=None, point_mask=None, obj_mask=None, max_delay=0, seed=0, rec=None):
    """The nearest form simulated point by point in the device's node order: a tested candidate reaches the k slots 0 .. max_delay of this
    point's triangle tests later; there it passes the leaf filter !(dist2 > bound) and is kept if it is among the k smallest keys so far.
    The bound, for the filter and for the nodes, is slot k - 1 alone: a NaN while fewer than k keys are kept.  Returns columns()' dict
    without n_within, with the walk's own counts."""
    p = np.ascontiguousarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    rec = pr.records_of(flat) if rec is None else rec
    r, r2 = pr.radius2(n, radius)
    walked = pr.walked_objects(flat, n, point_mask, obj_mask)
    mn, mx = flat.node_min.reshape(-1, 3).astype(F), flat.node_max.reshape(-1, 3).astype(F)
    is_leaf = flat.node_left < 0
    rng = np.random.default_rng(seed)
    out = dict(n_found=np.zeros(n, np.uint32), tri=np.full((n, k), -1, np.int32), dist2=np.full((n, k), INF, F), point=np.zeros((n, k, 3), F),
               vw=np.zeros((n, k, 2), F), region=np.zeros((n, k), np.uint8), node_tests_each=np.zeros(n, np.int64), tri_tests_each=np.zeros(n, np.int64))
    nan = float("nan")
    plans = {}
    for i in range(n):
        with np.errstate(invalid="ignore"):
            if not r[i] >= F(0.0):
                continue
        key = walked[i].tobytes()
        if key not in plans:
            plans[key] = nr.preorder(flat, np.flatnonzero(walked[i]))
        nodes, end = plans[key]
        b2, lo = nr.low(p[i][None, :], mn, mx)
        with np.errstate(invalid="ignore"):
            fails = (b2 > r2[i]).tolist()
        lo = lo.tolist()
        slots, pending, tests = [], [], 0                 # slots: at most k keys (dist2, tri), ascending

        def arrive(cand):
            bound = slots[k - 1][0] if len(slots) == k else nan
            if cand[0] > bound:                           # the leaf filter: it cannot be among the k
                return
            bisect.insort(slots, cand)
            del slots[k:]

        at = 0
        while at < len(nodes):
            while pending and pending[0][0] <= tests:
                arrive(pending.pop(0)[1])
            bound = slots[k - 1][0] if len(slots) == k else nan
            j = nodes[at]
            out["node_tests_each"][i] += 1
            if fails[j] or (lo[j] > bound and lo[j] < float("inf")):
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
                    pending.append((tests + (int(rng.integers(0, max_delay + 1)) if max_delay else 0), (float(d2[t]), f + int(t))))
                pending.sort(key=lambda e: e[0])
            at += 1
        for _, cand in pending:
            arrive(cand)
        if slots:
            ids = np.array([t for _, t in slots], np.int64)
            c = pr.closest_on_triangles(np.repeat(p[i][None, :], len(ids), 0), rec[ids])
            m = len(ids)
            out["n_found"][i] = m
            out["tri"][i, :m] = ids; out["dist2"][i, :m] = c["dist2"]; out["point"][i, :m] = c["point"]
            out["vw"][i, :m, 0] = c["v"]; out["vw"][i, :m, 1] = c["w"]; out["region"][i, :m] = c["region"]
    out.update(node_tests=int(out["node_tests_each"].sum()), tri_tests=int(out["tri_tests_each"].sum()), hits=int((out["n_found"] > 0).sum()))
    return out
