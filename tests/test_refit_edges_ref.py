"""CPU: what tests/refit_edges.py hands to tests/test_gpu_refit_edges.py is what it says -- the exact fold against pose_ref's and
numpy's, the zero ties counted, derive_ref against a float64 evaluation of the same formulas, every family's tags, and the oracle
still seeing a frame in every edge scene."""
import numpy as np
import pytest

import leaf_vectors as lv
import pose_ref
import refit_edges as edges
import tree_shapes as ts

CASES = [(f, t) for t in edges.TREES for f in edges.FAMILIES] + [("records", "records")]
FLOOR_HIT, FLOOR_CHANGED = 0.08, 100


def min_max_by_numpy(flat, pts):
    """numpy's min / max over the triangles below every node (values only; an empty node keeps the start values)."""
    xyz = np.ascontiguousarray(pts, np.float32).reshape(-1, 3, 4)[..., :3]
    mn = np.full((flat.n_nodes, 3), edges.FLT_MAX, np.float32); mx = np.full((flat.n_nodes, 3), -edges.FLT_MAX, np.float32)
    def below(i):
        if flat.node_left[i] < 0:
            return list(edges.leaf_rows(flat, i)) if flat.node_count[i] else []
        return below(int(flat.node_left[i])) + below(int(flat.node_right[i]))
    for i in range(flat.n_nodes):
        r = below(i)
        if r:
            v = xyz[r].reshape(-1, 3)
            mn[i], mx[i] = v.min(0), v.max(0)
    return mn, mx


# ---- the boxes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,name", CASES)
def test_boxes_exact_is_pose_ref_as_floats(fam, name):
    flat = edges.tree(name)
    pts, _ = edges.points(fam, name)
    want = edges.edge_scene(fam, name)
    mn, mx = pose_ref.boxes(flat, pts)
    assert not np.isnan(want.node_min).any() and not np.isnan(want.node_max).any()
    assert np.array_equal(want.node_min, mn) and np.array_equal(want.node_max, mx), "equal as floats to pose_ref's fmin / fmax fold"
    if fam in edges.ALL_FINITE or fam == "records":
        assert np.isfinite(pts[..., :3]).all()
        if name != "records":
            nmn, nmx = min_max_by_numpy(flat, pts)
            assert np.array_equal(want.node_min, nmn) and np.array_equal(want.node_max, nmx), "numpy's min / max on finite points"
    if fam in edges.UNTOUCHED_BOXES or fam == "records":
        assert np.array_equal(edges.bits(want.node_min), edges.bits(flat.node_min)) and np.array_equal(edges.bits(want.node_max), edges.bits(flat.node_max)), \
            "bit for bit flat_scene's own boxes where no xyz was touched"
    else:
        assert not np.array_equal(edges.bits(want.node_min), edges.bits(flat.node_min)) or not np.array_equal(edges.bits(want.node_max), edges.bits(flat.node_max))


@pytest.mark.parametrize("name", edges.TREES + ("shuffled",))
def test_boxes_exact_on_untouched_points_any_node_order(name):
    """flat_scene's own tight boxes bit for bit, on a shuffled node array too; the leaves side by side are fold_exact leaf by leaf."""
    flat = ts.family(name) if name == "shuffled" else edges.tree(name)
    mn, mx = edges.boxes_exact(flat, flat.tri_points)
    assert np.array_equal(edges.bits(mn), edges.bits(flat.node_min)) and np.array_equal(edges.bits(mx), edges.bits(flat.node_max))
    if name != "shuffled":
        pts, _ = edges.points(("zeros", "nan_some", "inf", "subnormal"), name)
        mn, mx = edges.boxes_exact(flat, pts)
        for i in np.flatnonzero(flat.node_left < 0):
            a, b = edges.fold_exact(pts[edges.leaf_rows(flat, i), :, :3])
            assert np.array_equal(edges.bits(a), edges.bits(mn[i])) and np.array_equal(edges.bits(b), edges.bits(mx[i])), i


def test_fold_exact_by_hand():
    nan, inf, z, mz = np.float32(np.nan), np.float32(np.inf), np.float32(0.0), np.float32(-0.0)
    snan = edges.from_bits([edges.SIGNALLING_NAN | edges.SIGN_BIT])[0]
    mn, mx = edges.fold_exact(np.array([[nan, inf, mz], [snan, inf, z], [nan, -inf, mz]], np.float32))
    assert list(edges.bits(mn)) == list(edges.bits([edges.FLT_MAX, -inf, mz])) and list(edges.bits(mx)) == list(edges.bits([-edges.FLT_MAX, inf, mz]))
    mn, mx = edges.fold_exact(np.array([[z, edges.FLT_MAX, 1], [mz, -edges.FLT_MAX, 1]], np.float32))
    assert list(edges.bits(mn)) == list(edges.bits([z, -edges.FLT_MAX, 1])) and list(edges.bits(mx)) == list(edges.bits([z, edges.FLT_MAX, 1]))
    mn, mx = edges.fold_exact(np.zeros((0, 3), np.float32))
    assert (mn == edges.FLT_MAX).all() and (mx == -edges.FLT_MAX).all()
    l, r = (np.float32([z, 5, mz]), np.float32([mz, 5, 1])), (np.float32([mz, nan, z]), np.float32([z, nan, 1]))
    cmn, cmx = edges.combine(l[0], l[1], r[0], r[1])
    assert list(edges.bits(cmn)) == list(edges.bits(l[0])) and list(edges.bits(cmx)) == list(edges.bits(l[1])), "the left operand stays on ties and against NaN"


@pytest.mark.parametrize("name", edges.TREES)
def test_zeros_family_ties_with_either_sign_first(name):
    """Leaves whose exact minimum (z) / maximum (x) is -0 and leaves where it is +0, both zeros present in the leaf; inner nodes whose
    children tie with opposite signs, in each order, below height 6 and (h7) above it."""
    flat = edges.tree(name)
    pts, tags = edges.points("zeros", name)
    want = edges.edge_scene("zeros", name)
    h = edges.node_height(flat)
    PLUS, MINUS = 0, edges.SIGN_BIT
    counts = {}
    for what, axis, box in (("min z", 2, edges.bits(want.node_min)), ("max x", 0, edges.bits(want.node_max))):
        for i in tags["zeros"]["leaves"]:
            v = edges.bits(pts[edges.leaf_rows(flat, i), :, axis]).reshape(-1)
            assert box[i, axis] in (PLUS, MINUS), "the leaf's extreme is a zero"
            both = (v == PLUS).any() and (v == MINUS).any()
            first = v[np.flatnonzero((v == PLUS) | (v == MINUS))[0]]
            assert box[i, axis] == first, "the first zero in visit order stays"
            counts[(what, "leaf", int(box[i, axis]), both)] = counts.get((what, "leaf", int(box[i, axis]), both), 0) + 1
        for i in np.flatnonzero(flat.node_left >= 0):
            l, r = box[flat.node_left[i], axis], box[flat.node_right[i], axis]
            if {int(l), int(r)} == {PLUS, MINUS}:
                assert box[i, axis] == l, "the left child's zero stays"
                key = (what, "low" if h[i] <= edges.POSE_SUB_HEIGHT else "high", int(l))
                counts[key] = counts.get(key, 0) + 1
    print(name, counts)
    for what in ("min z", "max x"):
        for sign in (PLUS, MINUS):
            assert counts.get((what, "leaf", sign, True), 0) >= 1, (what, sign, "a leaf with both zeros whose extreme has this sign")
            if (flat.node_left >= 0).any():
                assert counts.get((what, "low", sign), 0) >= 1, (what, sign, "an inner node of height <= 6 whose left child ties with this sign")
    if name == "h7":
        assert counts.get(("min z", "high", PLUS), 0) >= 1 and counts.get(("max x", "high", MINUS), 0) >= 1, "the ties at the node k_pose_top climbs"


# ---- the records ---------------------------------------------------------------------------------------------------------------------
def ulp_against(f32, f64):
    """|f32 - f64| in units of the float32 spacing at f64."""
    return np.abs(f32.astype(np.float64) - f64) / np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)


@pytest.fixture(scope="module")
def derive_rows():
    """The record soup, the w family, and 100 000 triangles of the test's own that cancel little: points of +-1 about a centre of +-1,
    scaled by 2^-20 .. 2^20, every vertex with a w of its own in [0.25, 4]."""
    rng = np.random.default_rng(5)
    own = np.empty((100000, 3, 4), np.float32)
    own[..., :3] = (rng.uniform(-1, 1, (100000, 1, 3)) + rng.uniform(-1, 1, (100000, 3, 3))) * np.exp2(rng.integers(-20, 21, (100000, 1, 1)))
    own[..., 3] = rng.uniform(0.25, 4.0, (100000, 3))
    own[..., :3] *= own[..., 3:]
    return np.concatenate([lv.record_points()[0], edges.points("w", "h7")[0], own])


# Measured on the 12 269 well-conditioned rows (of ~139 000) with the float64 evaluation as the yardstick, in float32 ulp of each
# element: points 0.50, edges 3.89, normal 12.39, tvec 0.50, qvec 10.63 (99.9 % of the elements: 0.5, 2.9, 5.7, 0.5, 6.2).  A divide
# and 0 - x round once; an edge is a difference of two rounded quotients that may lose two bits; a normal or qvec component is a
# difference of products of such, relative to ITSELF and not to the vector.  The bounds are the measured maxima rounded up.
DERIVE_ULP = dict(point=1, edge=4, normal=13, tvec=1, qvec=11)
FIELDS = dict(point=("tris", slice(0, 3)), edge=("tris", slice(3, 9)), normal=("tris", slice(9, 12)), tvec=("tris_o", slice(0, 3)), qvec=("tris_o", slice(9, 12)))


def test_derive_ref_against_float64_on_well_conditioned_rows(derive_rows):
    """A row is well conditioned when every named intermediate of the float64 evaluation is finite and of normal float32 size and no
    difference loses more than two bits (|a - b| >= max(|a|, |b|) / 4)."""
    t32, o32 = edges.derive_ref(derive_rows)
    t64, o64, part = edges.derive_ref(derive_rows, np.float64, parts=True)
    ok = np.ones(derive_rows.shape[0], bool)
    for k, v in part.items():
        if k not in ("w1", "w2", "w3"):
            ok &= np.isfinite(v) & (np.abs(v) >= edges.TINY) & (np.abs(v) <= edges.FLT_MAX)
    ok &= np.isfinite(derive_rows[..., 3]).all(1) & (np.abs(derive_rows[..., 3]) >= edges.TINY).all(1)
    for d, a, b in edges.DIFFERENCES:
        with np.errstate(all="ignore"):
            ok &= np.abs(part[d]) >= 0.25 * np.maximum(np.abs(part[a]), np.abs(part[b]))
    assert ok.sum() >= 5000, int(ok.sum())
    got = {"tris": (t32, t64), "tris_o": (o32, o64)}
    for name, (rec, sl) in FIELDS.items():
        u = ulp_against(got[rec][0][ok][:, sl], got[rec][1][ok][:, sl])
        print(f"derive_ref against float64, {name}: max {u.max():.2f} ulp on {int(ok.sum())} rows (bound {DERIVE_ULP[name]})")
        assert u.max() <= DERIVE_ULP[name], (name, float(u.max()))


def test_derive_ref_nan_inf_and_zero_sit_where_clamped_float64_puts_them(derive_rows):
    """Every row, the overflowing, underflowing and dividing-by-zero ones included: the float64 evaluation with every operation's result
    clamped to float32's range gives NaN, +-inf and 0 in exactly the places derive_ref does.  Left out: the rows where a float64
    intermediate lies within 1e-5 (relative) of a clamp's threshold -- there the two precisions may round to different sides --, rows
    with a subnormal intermediate, whose float32 rounding is coarser than any relative bound, and rows where a difference of unequal
    operands is below 2^-20 of them: float32 holds 24 bits, so such a difference is rounding noise and may be exactly 0 in one
    precision and not in the other (collinear points)."""
    t32, o32 = edges.derive_ref(derive_rows)
    t64, o64, part = edges.derive_ref(derive_rows, np.float64, clamp=edges.clamp_to_float32_range, parts=True)
    near = np.zeros(derive_rows.shape[0], bool)
    for v in part.values():
        a = np.abs(v)
        with np.errstate(all="ignore"):
            near |= (np.abs(a / 2.0 ** 128 - 1) < 1e-5) | ((a > 0) & (a < float(edges.TINY)))
    for d, a, b in edges.DIFFERENCES:
        with np.errstate(all="ignore"):
            near |= (np.abs(part[d]) < 2.0 ** -20 * np.maximum(np.abs(part[a]), np.abs(part[b]))) & (part[a] != part[b])
    keep = ~near
    special = ~np.isfinite(t32).all(1) | ~np.isfinite(o32).all(1) | (t32 == 0).any(1)
    assert (special & keep).sum() >= 3000 and keep.sum() >= 0.8 * keep.size, (int((special & keep).sum()), int(keep.sum()))
    for a, b, what in ((t32, t64, "tris"), (o32, o64, "tris_o")):
        a, b = a[keep], b[keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f"{what}: {int((np.isnan(a) != np.isnan(b)).sum())} NaN places differ"
        assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b)), f"{what}: inf"
        assert np.array_equal(a == 0, b == 0), f"{what}: {int(((a == 0) != (b == 0)).sum())} zeros differ"
    assert np.isnan(t32).any() and np.isinf(t32).any() and (t32 == 0).any()


# ---- the families hold what they claim ---------------------------------------------------------------------------------------------------
def both_sides_of_256(flat, tri):
    return flat.n_tris <= 257 or ((np.asarray(tri) <= 255).any() and (np.asarray(tri) >= 256).any())


@pytest.mark.parametrize("name", edges.TREES)
def test_trees_and_tags(name):
    flat = edges.tree(name)
    base = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)
    h = edges.node_height(flat)
    if name in ("h6", "h7"):
        assert flat.n_tris > 256 and flat.n_tris % 256 and h[flat.obj_root[0]] == int(name[1]) and (flat.node_count == 31).any() and (flat.node_count[flat.node_left < 0] == 0).any()
        assert (h > edges.POSE_SUB_HEIGHT).sum() == (name == "h7")
    if name == "h7":
        root = flat.obj_root[0]
        assert h[flat.node_left[root]] <= 6 and h[flat.node_right[root]] <= 6 and flat.node_left[flat.node_left[root]] >= 0 and flat.node_left[flat.node_right[root]] >= 0
    assert flat.n_objects >= 3 and flat.node_count.max() == 31
    # nan_some
    p, t = edges.points("nan_some", name); t = t["nan_some"]
    v = edges.bits(p)[t["tri"], t["vertex"], t["axis"]]
    assert {(int(a), int(b)) for a, b in zip(t["vertex"], t["axis"])} == {(a, b) for a in range(3) for b in range(3)}
    assert set(v) == {edges.QUIET_NAN, edges.SIGNALLING_NAN, edges.QUIET_NAN | edges.SIGN_BIT, edges.SIGNALLING_NAN | edges.SIGN_BIT}
    assert np.isnan(p).sum() == t["tri"].size and 0.09 <= t["tri"].size / flat.n_tris <= 0.18 and both_sides_of_256(flat, t["tri"])
    # nan_leaf
    p, t = edges.points("nan_leaf", name); t = t["nan_leaf"]
    assert flat.node_count[t["big"]] == 31
    if t["has_children"]:
        assert t["left"] in flat.node_left and t["right"] in flat.node_right
    rows = np.concatenate([edges.leaf_rows(flat, i) for i in t["leaves"]])
    assert len(set(t["leaves"])) == 3 and np.isnan(p[rows, :, :3]).all() and np.isnan(p).sum() == 9 * rows.size
    assert {edges.QUIET_NAN, edges.SIGNALLING_NAN} <= set(edges.bits(p[rows, :, :3]).reshape(-1) & ~np.uint32(edges.SIGN_BIT))
    want = edges.edge_scene("nan_leaf", name)
    assert (want.node_min[t["leaves"]] == edges.FLT_MAX).all() and (want.node_max[t["leaves"]] == -edges.FLT_MAX).all()
    # nan_object
    p, t = edges.points("nan_object", name); t = t["nan_object"]
    want = edges.edge_scene("nan_object", name)
    r = flat.obj_root[t["objs"]]
    assert np.isnan(p[t["tri"], :, :3]).all() and (want.node_min[r] == edges.FLT_MAX).all() and (want.node_max[r] == -edges.FLT_MAX).all()
    # inf
    p, t = edges.points("inf", name); t = t["inf"]
    v = p[t["tri"], t["vertex"], t["axis"]]
    assert {(int(a), int(b)) for a, b in zip(t["vertex"], t["axis"])} == {(a, b) for a in range(3) for b in range(3)}
    assert np.isposinf(v).any() and np.isneginf(v).any() and np.isinf(v).all() and both_sides_of_256(flat, t["tri"])
    assert np.isposinf(p[t["plus"], :, :3]).all() and np.isneginf(p[t["minus"], :, :3]).all()
    r = edges.leaf_rows(flat, t["sandwich"])
    assert np.isposinf(p[r[0], :, :3]).all() and np.isfinite(p[r[1]]).all() and np.isneginf(p[r[2:], :, :3]).all()
    want = edges.edge_scene("inf", name)
    assert np.isneginf(want.node_min[t["sandwich"]]).all() and np.isposinf(want.node_max[t["sandwich"]]).all()
    # fltmax
    p, t = edges.points("fltmax", name); t = t["fltmax"]
    v = p[t["tri"], t["vertex"], t["axis"]]
    assert set(edges.bits(v)) == set(edges.bits([edges.FLT_MAX, -edges.FLT_MAX, edges.BELOW_MAX, -edges.BELOW_MAX])) and both_sides_of_256(flat, t["tri"])
    assert set(t["axis"]) == {0, 1, 2} and set(t["vertex"]) == {0, 1, 2}
    # subnormal
    p, t = edges.points("subnormal", name); t = t["subnormal"]
    m = t["mask"]
    assert edges.is_subnormal(p[..., :3])[m].all() and all(m[..., a].sum() >= 3 for a in range(3)) and both_sides_of_256(flat, np.flatnonzero(m.any((1, 2))))
    assert (p[..., :3][m] > 0).any() and (p[..., :3][m] < 0).any()
    flushed = np.where(edges.is_subnormal(p), np.float32(0.0), p)
    fl = edges.boxes_exact(flat, flushed)
    want = edges.edge_scene("subnormal", name)
    assert (fl[0] != want.node_min).any() and (fl[1] != want.node_max).any(), "a fold that flushed its inputs would leave other boxes"
    neither = 0                                                 # a COMPARE that flushed sees ties everywhere and keeps the first element
    for j, i in enumerate(t["leaves"]):
        a = j % 3
        first = edges.bits(p[edges.leaf_rows(flat, int(i))[0], 0, a:a + 1])[0]
        neither += int(first != edges.bits(want.node_min[i, a:a + 1])[0] and first != edges.bits(want.node_max[i, a:a + 1])[0])
    print(name, "subnormal leaves whose first element is neither extreme:", neither, "of", len(t["leaves"]))
    assert neither >= 3 and 2 * neither >= len(t["leaves"]), "the first element of a subnormal leaf is rarely its minimum or maximum"
    # w
    p, t = edges.points("w", name); t = t["w"]
    assert {(int(a), int(b)) for a, b in zip(t["kind"], t["vertex"])} == {(a, b) for a in range(7) for b in range(3)}
    assert np.array_equal(edges.bits(p[..., :3]), edges.bits(base[..., :3])) and both_sides_of_256(flat, t["tri"])
    wv = p[t["tri"], t["vertex"], 3]
    k = t["kind"]
    assert ((wv[k == 0] >= 0.25) & (wv[k == 0] <= 4)).all() and (wv[k == 1] < 0).all() and (np.abs(np.log10(np.abs(wv[k == 2]))) > 29).all()
    assert (edges.bits(wv[k == 3]) == 0).all() and (edges.bits(wv[k == 4]) == edges.SIGN_BIT).all() and edges.is_subnormal(wv[k == 5]).all() and np.isnan(wv[k == 6]).all()
    assert 0.2 <= t["tri"].size / flat.n_tris <= 0.3


@pytest.mark.parametrize("name", ("sliced", "roots33"))
def test_matrix_kinds(name):
    flat = edges.tree(name)
    sp = edges.special_objects(flat)
    assert 1 <= sp.size <= flat.n_objects // 2
    base = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)
    sel = np.isin(flat.tri_obj, sp)
    for kind in edges.MATRIX_KINDS:
        m = edges.matrices(kind, flat)
        rest = np.setdiff1d(np.arange(flat.n_objects), sp)
        R = m[rest].reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)
        assert np.allclose(R @ R.transpose(0, 2, 1), np.eye(3), atol=1e-5) and (np.linalg.det(R) > 0).all(), "the other objects keep a rigid turn"
        p = pose_ref.transform_objects(flat, m)
        if np.isfinite(m).all():
            assert np.array_equal(np.isfinite(p[~sel]), np.ones_like(p[~sel], bool))
        q = p[sel]
        if kind == "inf_entry":
            assert np.isinf(m[sp]).sum() == sp.size and not np.isfinite(q).all()
        elif kind == "nan_entry":
            assert np.isnan(m[sp]).sum() == sp.size and np.isnan(q).any()
        elif kind == "scale_2p100":
            assert np.isfinite(q).all() and (np.abs(q[..., :3]) > 2.0 ** 90).any()
        elif kind == "turn_2p125":
            assert np.isinf(q).any() and np.isnan(q).any()
        elif kind == "scale_2m140":
            assert edges.is_subnormal(q[..., :3]).mean() > 0.9
        elif kind == "zero":
            assert np.array_equal(edges.bits(q), np.zeros(q.shape, np.uint32))
        elif kind == "proj_generic":
            assert ((q[..., 3] >= 0.25) & (q[..., 3] <= 4.0)).all() and (q[..., 3] != 1.0).all()
        elif kind == "proj_zero":
            assert all((p[flat.tri_obj == k][..., 3] == 0).any() for k in sp) and (q[..., 3] != 0).any()
        elif kind == "mirror":
            assert (np.linalg.det(m[sp].reshape(-1, 4, 4)[:, :3, :3].astype(np.float64)) < 0).all()


# ---- the oracle still sees a frame ---------------------------------------------------------------------------------------------------
def check_floors(oracle, want, base_hit, what):
    for L in (1, 9):
        c = oracle.render(want, ts.frame_params(L), pow="device")
        hit = c["hit_id"] >= 0
        changed = int((c["hit_id"] != base_hit).sum())
        print(f"{what} L {L}: {int(hit.sum())} of {hit.size} pixels hit, {changed} changed, {int(np.isnan(c['rgb_linear']).sum())} NaN colours")
        assert hit.sum() >= FLOOR_HIT * hit.size, (what, int(hit.sum()))
        assert changed >= FLOOR_CHANGED, (what, changed)
        assert np.isfinite(c["t"][hit]).all(), what


@pytest.mark.parametrize("name", edges.TREES)
def test_oracle_takes_every_edge_scene(oracle, name):
    base = oracle.render(edges.tree(name), ts.frame_params(1))["hit_id"]
    for fam in list(edges.FAMILIES) + [edges.WALK_MIX, edges.BUILD_MIX]:
        check_floors(oracle, edges.edge_scene(fam, name), base, f"{name} {fam}")


@pytest.mark.parametrize("name", ("sliced", "roots33"))
def test_oracle_takes_every_posed_scene(oracle, name):
    flat = edges.tree(name)
    base = oracle.render(flat, ts.frame_params(1))["hit_id"]
    for kind in edges.MATRIX_KINDS:
        check_floors(oracle, edges.pose_flat(flat, edges.matrices(kind, flat)), base, f"{name} {kind}")
