"""The device leaf functions beyond scene-scale inputs (-m gpu): the slab test in its three forms, the triangle test in both forms,
barycentric coordinates and the triangle records derived on the device, on the input families of tests/leaf_vectors.py (coordinates
scaled by 2^-120 .. 2^116, non-zero origins, w != 1, zero / subnormal / non-finite direction components, flat, empty and infinite
boxes), against the oracle that tests/test_oracle_golden.py pins to the reference over the same families.  Extreme values go through
the srt_kat_* vectors only; every scene that is traversed has finite coordinates of ordinary size."""
import os

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import leaf_vectors as lv
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def leaf():
    return {"box": lv.box_families(), "tri": lv.tri_families(), "kat": np.load(os.path.join(gu.GOLDEN, "leaf_kat.npz"))}


def _bounds(fams):
    b = np.cumsum([0] + [f.ray.shape[0] for f in fams])
    return [(f, int(b[i]), int(b[i + 1])) for i, f in enumerate(fams)]


def test_slab_forms_and_filter_soundness(srt, oracle, leaf):
    """srt_kat_ray_aabb on every ray / box family, one launch.  The literal and the branch-free form equal the oracle on every row.
    The filtered form is SOUND: where it does not say `ambiguous`, its answer is the oracle's -- on every family, also those with a
    zero, subnormal, huge, infinite or NaN direction component and with boxes flat at the origin's coordinate, where both quotients
    of an axis are NaN.  On the ordinary families (primary-, shadow-, camera-like and corner rays at 2^-60 .. 2^60) it must decide some
    rows and leave some ambiguous: a filter that calls everything ambiguous, or nothing, is not what the kernels are built around.
    The share of rows the filter decides is reported per family in gpu_frames.RESIDUALS["leaf_filter_decided"]."""
    fams = leaf["box"]
    ray = np.concatenate([f.ray for f in fams]); box = np.concatenate([f.box for f in fams])
    want = oracle.ray_aabb(ray, box)
    exact, nb, filt, amb = srt.kat_ray_aabb(ray, box)
    share = gf.RESIDUALS.setdefault("leaf_filter_decided", {})
    errors = []
    for f, a, b in _bounds(fams):
        for name, got in (("literal", exact), ("branch-free", nb)):
            bad = np.flatnonzero(got[a:b] != want[a:b])
            if len(bad):
                i = a + int(bad[0])
                errors.append(f"{f.name}: {len(bad)} of {b - a} rows of the {name} form differ from the oracle; first row {int(bad[0])}: ray {ray[i]!r} "
                              f"box {box[i]!r} quotients {lv.box_quotients(ray[i], box[i])!r} device {int(got[i])} oracle {int(want[i])}")
        ok = amb[a:b] == 0
        share[f.name] = float(ok.mean())
        bad = np.flatnonzero(ok & (filt[a:b] != want[a:b]))
        if len(bad):
            i = a + int(bad[0])
            errors.append(f"{f.name}: the filter decided {len(bad)} of {b - a} rows wrongly without saying ambiguous; first row {int(bad[0])}: ray {ray[i]!r} "
                          f"box {box[i]!r} quotients {lv.box_quotients(ray[i], box[i])!r} filtered {int(filt[i])} oracle {int(want[i])}")
        if f.ordinary and not (ok.any() and (~ok).any()):
            errors.append(f"{f.name}: an ordinary family must have rows the filter decides and ambiguous rows; decided share {ok.mean():.4f}")
    print("filter-decided share per family:", {k: round(v, 4) for k, v in share.items()})
    assert not errors, f"{len(errors)} failures:\n" + "\n".join(errors)


def test_triangle_test_in_both_forms(srt, oracle, leaf):
    """srt_kat_ray_triangle equals the oracle on every triangle family (same bits, or NaN on both sides); the origin form
    (srt_kat_ray_triangle_origin: the record with tvec and qvec that every primary ray reads) equals the general form on every row
    whose ray leaves the origin; both equal what the compiled reference returned on the recorded subsample (leaf_kat.npz)."""
    fams = leaf["tri"]
    ray = np.concatenate([f.ray for f in fams]); tri = np.concatenate([f.tri for f in fams])
    want = oracle.ray_triangle(ray, tri)
    got = srt.kat_ray_triangle(ray, tri)
    ok = gf.same_f32(got, want)
    for f, a, b in _bounds(fams):
        bad = np.flatnonzero(~ok[a:b])
        assert not len(bad), f"{f.name}: {len(bad)} of {b - a} rows differ from the oracle; first row {int(bad[0])}: ray {ray[a + bad[0]]!r} tri {tri[a + bad[0]]!r} " \
                             f"device {got[a + bad[0]]!r} oracle {want[a + bad[0]]!r}"
    dirs, tris, names = lv.origin0_rows(fams)
    ray0 = np.zeros((dirs.shape[0], 6), np.float32); ray0[:, 3:] = dirs
    general = srt.kat_ray_triangle(ray0, tris)
    origin = srt.kat_ray_triangle_origin(dirs, tris)
    assert gf.same_f32(general, oracle.ray_triangle(ray0, tris)).all()
    bad = np.flatnonzero(~gf.same_f32(origin, general))
    assert not len(bad), f"{names[bad[0]]}: the origin form differs from the general form on {len(bad)} of {len(names)} rows; first: dir {dirs[bad[0]]!r} " \
                         f"tri {tris[bad[0]]!r} origin form {origin[bad[0]]!r} general {general[bad[0]]!r}"
    assert (np.isfinite(origin) & (origin > 0)).sum() > 2000, "the origin-form rows must contain hits at finite t"
    k = leaf["kat"]
    assert gf.same_f32(srt.kat_ray_triangle(k["tri_ray"], k["tri_tri"]), k["tri_t"]).all(), "general form differs from the recorded reference"
    o0 = np.all(k["tri_ray"][:, :3] == 0, axis=1)
    assert o0.sum() > 500
    assert gf.same_f32(srt.kat_ray_triangle_origin(k["tri_ray"][o0, 3:], k["tri_tri"][o0]), k["tri_t"][o0]).all(), "origin form differs from the recorded reference"


def test_barycentric(srt, oracle, leaf):
    """srt_kat_barycentric: the reference's known answers (kat.npz) and the oracle on every triangle family, bit for bit."""
    k = gu.load_kat()
    got = srt.kat_barycentric(k["bc_in"])
    assert np.array_equal(gf.bits(got), gf.bits(k["bc_uvw"])), "device barycentric differs from the reference's known answers"
    assert np.array_equal(gf.bits(got), gf.bits(oracle.barycentric(k["bc_in"])))
    inp = lv.bary_inputs(leaf["tri"])
    bad = ~gf.same_f32(srt.kat_barycentric(inp), oracle.barycentric(inp)).all(1)
    assert not bad.any(), f"{int(bad.sum())} of {len(bad)} rows differ from the oracle; first input {inp[np.flatnonzero(bad)[0]]!r}"
    sub = [lv.Family(f.name, "tri", f.ray[lv.subsample(f.ray.shape[0])], tri=f.tri[lv.subsample(f.ray.shape[0])]) for f in leaf["tri"]]
    assert gf.same_f32(srt.kat_barycentric(lv.bary_inputs(sub)), leaf["kat"]["bc_uvw"]).all(), "differs from the recorded reference"


# ---- records -------------------------------------------------------------------------------------------------------------------------
FLOAT_COLS = {"tris": slice(0, 12), "tris_o": slice(0, 12), "nodes": slice(0, 6), "root_nodes": slice(0, 6), "wide": slice(0, 12)}


def records_equal(got, want, what, tri_points=None):
    """Device records against the host's: the float fields with gpu_frames.same_f32 semantics -- the same bits, or NaN on both sides
    (the host's and the device's arithmetic may give a COMPUTED NaN different sign bits: x86 SSE produces the negative default NaN,
    the GPU the positive one) -- and the integer fields (skip, leaf, child links) exactly."""
    for k, fs in FLOAT_COLS.items():
        g, w = got[k], want[k]
        assert g.shape == w.shape, (what, k)
        same = gf.same_f32(g[:, fs].view(np.float32), w[:, fs].view(np.float32))
        bad = np.argwhere(~same)
        by_w = ""
        if len(bad) and tri_points is not None and k in ("tris", "tris_o"):         # which triangles: those whose divides by w are exact, or the others
            rec = np.unique(bad[:, 0])
            w1 = np.all(np.asarray(tri_points).reshape(-1, 3, 4)[rec, :, 3] == 1.0, axis=1)
            by_w = f"; of the {len(rec)} differing records {int(w1.sum())} have w == 1 throughout, {int((~w1).sum())} have not"
        assert not len(bad), f"{what}: {k} differs in {len(bad)} floats; first: record {int(bad[0][0])} field {int(bad[0][1])} " \
                             f"device {g[:, fs].view(np.float32)[tuple(bad[0])]!r} host {w[:, fs].view(np.float32)[tuple(bad[0])]!r}" + by_w
        rest = np.ones(g.shape[1], bool); rest[fs] = False
        assert np.array_equal(g[:, rest], w[:, rest]), f"{what}: integer fields of {k} differ"


def source_attrs(om, flat, names):
    """per-triangle attributes in source order, from the flat (visit-order) arrays and the hierarchies' permutations"""
    tc, nrm, tex = np.zeros_like(flat.tri_texcoord), np.zeros_like(flat.tri_normals), np.full(flat.n_tris, -1, np.int32)
    base = 0
    for nme in names:
        _, order, _, _ = om.hierarchy(nme)
        src = base + order.astype(np.int64); vis = base + np.arange(order.shape[0])
        tc.reshape(-1, 6)[src] = flat.tri_texcoord.reshape(-1, 6)[vis]; nrm.reshape(-1, 9)[src] = flat.tri_normals.reshape(-1, 9)[vis]
        tex[src] = flat.tri_tex[vis]
        base += order.shape[0]
    return tc, nrm, tex


COUNTS = (1, 8, 9, 17, 300)


def build_objects(pts, counts=COUNTS, start=0, colors=None):
    """objects o0, o1, ... of the given triangle counts, cut from pts in order, built with the host mirror's builder"""
    from simple_raytracer_amd import host
    om = host.ObjectManager()
    at = start
    for k, n in enumerate(counts):
        om.add_object(f"o{k}", pts[at:at + n]); om.setColor(f"o{k}", colors[k] if colors is not None else (0.2 + 0.15 * k, 0.9 - 0.1 * k, 0.5))
        om.createBoundingHierarchy(f"o{k}")
        at += n
    return om


def update_frame_from(ds, om, names, flat):
    hs = [om.hierarchy(nme) for nme in names]
    assert any(not np.array_equal(h[1], np.arange(h[1].shape[0])) for h in hs), "the build must leave a non-identity permutation"
    ds.update_frame([h[0] for h in hs], [h[1] for h in hs], [h[2] for h in hs], [h[3] for h in hs], obj_color=flat.obj_color, obj_material=flat.obj_material)


def test_device_record_derivation_beyond_scene_scale(srt, oracle, leaf):
    """derive_triangle on the device (k_update_tris) against the host's, where the nine divides by w are NOT exact and 1 / sqrt sees
    ill-formed triangles: a soup of every triangle family (w in [0.25, 4], negative w, w near 1e+-30, zero area, slivers, scales 2^-100
    .. 2^60) plus triangles whose cross product overflows or underflows (normal inf, NaN or 0 * inf), as several objects of 1, 8, 9,
    17 and 300 triangles, twice over.  srt_scene_update_frame with the build's permutation must leave the records a fresh
    srt_scene_create of the flattened frame has: tris, tris_o, nodes, wide and root_nodes.  Records only: nothing traverses that scene.
    Then the sub-scene of finite, ordinary-scale triangles (w != 1 included) goes the same way and is rendered against the oracle."""
    pts, w1 = lv.record_points()
    rng = np.random.default_rng(3)
    soup = COUNTS + (2000,)                    # one big object on top, so that a dozen frames hold every triangle of the families
    per = sum(soup)
    assert (~w1).sum() > 2 * per
    # every object mixes w == 1 and w != 1 rows and all scales: shuffle once, deterministically
    pts = pts[rng.permutation(pts.shape[0])]
    sets = pts.shape[0] // per
    assert sets >= 12
    om0 = build_objects(pts, soup, start=pts.shape[0] - per)
    flat0 = om0.flatten(); names = flat0.names
    ds = srt.DeviceScene(flat0)
    ds.set_source(*source_attrs(om0, flat0, names))
    total = 0
    for s in range(sets):
        om = build_objects(pts, soup, start=s * per)
        flat = om.flatten()
        update_frame_from(ds, om, names, flat)
        fresh = srt.DeviceScene(flat)
        records_equal(ds.records(), fresh.records(), f"soup {s}", flat.tri_points)
        total += flat.n_tris
        fresh.close()
    ds.close()
    assert total >= 0.95 * pts.shape[0]
    per = sum(COUNTS)
    # the ordinary sub-scene: finite coordinates at scale 0, w in [0.25, 4] and negative w among them, in front of the camera
    fams = {f.name: f for f in leaf["tri"]}
    sub = np.concatenate([fams[n].tri for n in ("kat_rt2@2^0", "w_pos@2^0", "w_neg@2^0", "degenerate@2^0", "origin_on@2^0")]).reshape(-1, 3, 4)
    sub = sub[rng.permutation(sub.shape[0])]
    assert np.isfinite(sub).all() and np.abs(sub).max() < 1e5 and (sub[..., 3] != 1).any()
    oma, omb = build_objects(sub, start=0), build_objects(sub, start=per)
    fa, fb = oma.flatten(), omb.flatten()
    ds = srt.DeviceScene(fa)
    ds.set_source(*source_attrs(oma, fa, fa.names))
    update_frame_from(ds, omb, fa.names, fb)
    fresh = srt.DeviceScene(fb)
    records_equal(ds.records(), fresh.records(), "ordinary sub-scene", fb.tri_points)
    p = abi.make_params(160, 120, abi.light_staircase((120.0, -300.0, -50.0), 2))
    c = oracle.render(fb, p, pow="device")
    assert (c["hit_id"] >= 0).sum() > 500
    for what, h in (("updated", ds), ("fresh", fresh)):
        gf.compare_exact(srt, h.render(p), c, gf.owned(p), fb, p, f"ordinary sub-scene, {what}")


def test_update_after_a_topology_change(srt, oracle, leaf):
    """srt_scene_update to a scene with the same totals but other trees (two objects of 20 and 9 triangles become 9 and 20: ten nodes
    either way), then srt_scene_set_source and srt_scene_update_frame on the new shape: scene_update_impl must have refreshed the
    per-object ranges, first triangles, leaf table and wide-record indices the device half of the rebuild reads.  Records equal a
    fresh scene's; the frame is the oracle's."""
    fams = {f.name: f for f in leaf["tri"]}
    pts = np.concatenate([fams["kat_rt2@2^0"].tri, fams["w_pos@2^0"].tri]).reshape(-1, 3, 4)
    pts = pts[np.random.default_rng(4).permutation(pts.shape[0])]
    cols = [(0.9, 0.3, 0.2), (0.2, 0.5, 0.9)]
    omA = build_objects(pts, (20, 9), 0, cols)
    omB = build_objects(pts, (9, 20), 100, cols)
    omC = build_objects(pts, (9, 20), 200, cols)
    fA, fB, fC = omA.flatten(), omB.flatten(), omC.flatten()
    assert fA.n_nodes == fB.n_nodes == fC.n_nodes == 10 and fA.n_tris == fB.n_tris == 29 and fA.names == fB.names
    assert not np.array_equal(fA.node_count, fB.node_count), "the two scenes must have different trees"
    p = abi.make_params(160, 120, abi.light_staircase((120.0, -300.0, -50.0), 2))
    ds = srt.DeviceScene(fA)
    gf.compare_exact(srt, ds.render(p), oracle.render(fA, p, pow="device"), gf.owned(p), fA, p, "before the change")
    ds.update(fB)
    fresh = srt.DeviceScene(fB)
    records_equal(ds.records(), fresh.records(), "srt_scene_update to other trees")
    gf.compare_exact(srt, ds.render(p), oracle.render(fB, p, pow="device"), gf.owned(p), fB, p, "after srt_scene_update")
    ds.set_source(*source_attrs(omB, fB, fB.names))
    update_frame_from(ds, omC, fB.names, fC)
    ds.flat = fC
    freshC = srt.DeviceScene(fC)
    records_equal(ds.records(), freshC.records(), "srt_scene_update_frame after the change")
    c = oracle.render(fC, p, pow="device")
    assert (c["hit_id"] >= 0).sum() > 300
    gf.compare_exact(srt, ds.render(p), c, gf.owned(p), fC, p, "srt_scene_update_frame after the change")


def planar_mesh(axis):
    """40 triangles in the plane x = 0 (axis 0) or y = 0 (axis 1): a 4 x 5 grid of quads over +-60 x [200, 400] in front of the camera"""
    other = 1 - axis
    tris = []
    for a in range(4):
        for b in range(5):
            u0, u1 = -60.0 + 30.0 * a, -30.0 + 30.0 * a
            z0, z1 = 200.0 + 40.0 * b, 240.0 + 40.0 * b
            def v(u, z):
                q = [0.0, 0.0, z, 1.0]; q[other] = u; return q
            tris.append([v(u0, z0), v(u1, z0), v(u1, z1)]); tris.append([v(u0, z0), v(u1, z1), v(u0, z1)])
    return np.array(tris, np.float32)


def test_edge_on_walls_through_the_camera_end_to_end(srt, oracle):
    """A wall in the plane x = 0 and one in the plane y = 0, seen edge-on: every node box of such an object is flat at 0 on that axis, and
    for the rays of the pixel column i = 0 (row j = 0) both quotients of that axis are 0 * inf = NaN at every node.  The reference walks
    those trees to the leaves (a NaN rejects nothing) and finds no hit (det = 0); a filter that drops the NaN pair would cut the walk
    short -- same picture, other work counters.  Hit ids, t, the colours (strict bar) and all four work counters of the counting
    build must be the oracle's, through the shipped pipeline and the variants of test_adversarial_scenes_match_oracle.  A cube
    behind the walls straddles x = 0 and the light has x = 0, so that shadow rays with d.x = 0 leave the column's hit points."""
    from simple_raytracer_amd import host
    T = host.Transformation
    W, H, L = 96, 64, 2
    light = (0.0, -300.0, 100.0)
    def scene(only=None):
        om = host.ObjectManager()
        if only in (None, "wall_x"):
            om.add_object("wall_x", planar_mesh(0)); om.setColor("wall_x", (0.8, 0.2, 0.2)); om.createBoundingHierarchy("wall_x")
        if only in (None, "wall_y"):
            om.add_object("wall_y", planar_mesh(1)); om.setColor("wall_y", (0.2, 0.8, 0.2)); om.createBoundingHierarchy("wall_y")
        if only is None:
            om.add_object("cube", gu.load_mesh("cube")); om.setColor("cube", (0.3, 0.4, 0.9))
            om.transformTriangles("cube", T.scaleObj(60.0, 60.0, 60.0)); om.transformTriangles("cube", T.rotateObjY(T.radians(20.0)))
            om.transformTriangles("cube", T.changeObjPosition(5.0, 3.0, 600.0)); om.createBoundingHierarchy("cube")
        return om.flatten()
    # the scene proves something only if the oracle walks the walls' trees beyond their roots on the column i = 0 / the row j = 0
    fx = scene("wall_x")
    col = oracle.render(fx, abi.make_params(1, H, abi.light_staircase(light, 1), flags=abi.SRT_FLAG_COUNT_WORK))       # width 1: the column i = 0
    assert col["stats"]["node_tests_primary"] > 3 * H, col["stats"]["node_tests_primary"]
    fy = scene("wall_y")
    row = oracle.render(fy, abi.make_params(W, 1, abi.light_staircase(light, 1), flags=abi.SRT_FLAG_COUNT_WORK))       # height 1: the row j = 0
    assert row["stats"]["node_tests_primary"] > 3 * W, row["stats"]["node_tests_primary"]
    flat = scene()
    assert flat.n_objects == 3 and flat.n_tris == 92
    p = abi.make_params(W, H, abi.light_staircase(light, L), flags=abi.SRT_FLAG_COUNT_WORK)
    c = oracle.render(flat, p, pow="device")
    hit_col = c["hit_id"][:, W // 2] >= 0
    assert (c["hit_id"] >= 0).sum() > 200 and hit_col.any(), "the cube must be hit on the column i = 0"
    ds = srt.DeviceScene(flat)
    for variant in (0, 4, 3, 6, 21, 22):
        pv = abi.make_params(W, H, abi.light_staircase(light, L), flags=abi.SRT_FLAG_COUNT_WORK | (variant << 8))
        o = ds.render(pv)
        gf.compare_exact(srt, o, c, gf.owned(pv), flat, pv, f"edge-on walls, variant {variant}")
        for k in ("node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow"):
            assert o["stats"][k] == c["stats"][k], f"variant {variant} ({ds.pipeline}): {k} is {o['stats'][k]}, the oracle's {c['stats'][k]}"
