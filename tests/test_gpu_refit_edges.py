"""GPU (-m gpu): srt_scene_refit_device and srt_scene_pose on the points of tests/refit_edges.py -- NaN of both kinds, +-inf, +-FLT_MAX,
zeros of both signs, subnormals, w of every kind -- against the exact fold (refit_edges.boxes_exact) and two opinions on the triangle
records: srt_scene_create's host derivation and refit_edges.derive_ref.

No tolerance here is a measured number.  Box floats and the words beside them are compared as uint32 (-0 is not +0); both triangle
records are the same bits, or NaN on both sides (the host's and the device's computed NaN differ in sign); frames are compared with
gpu_frames.compare_exact, work counts and query answers are the oracle's.  tests/test_refit_edges_ref.py shows on the CPU that the
families hold what they claim and that the oracle still sees a frame in each."""
import dataclasses

import numpy as np
import pytest

import gpu_frames as gf
import pose_ref
import ray_query_ref as rq
import refit_edges as edges
import refit_ref
import tree_shapes as ts
from simple_raytracer_amd import abi
from test_gpu_refit import DeviceBuffers

pytestmark = pytest.mark.gpu
CASES = [(f, t) for t in edges.TREES for f in edges.FAMILIES] + [("records", "records")]
EMPTY_BOX = edges.bits([edges.FLT_MAX] * 3 + [-edges.FLT_MAX] * 3)
IDENTITY = np.eye(4, dtype=np.float32).reshape(16)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture()
def dev(srt):
    d = DeviceBuffers(srt)
    yield d
    d.free()


def created_records(srt, want):
    fresh = srt.DeviceScene(want)
    r = fresh.records()
    fresh.close()
    return r


def box_bits(rec, key, rows):
    return pose_ref.split_boxes(rec, key)[0].view(np.uint32)[rows]


# ---- a. boxes, bit for bit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,name", CASES)
def test_refit_boxes_and_records_bit_for_bit(srt, dev, fam, name):
    """A direct refit from 16-byte aligned xyzw points against a scene created from the points and boxes_exact, and against derive_ref."""
    flat = edges.tree(name)
    pts, tags = edges.points(fam, name)
    ds = srt.DeviceScene(flat); ds.refit_prepare()
    ds.refit_device(dev.put(pts), stride=4); ds.sync()
    got = ds.records()
    ds.close()
    edges.same_records_bits(got, created_records(srt, edges.edge_scene(fam, name)), f"{fam} on {name}", derived=edges.derive_ref(pts))
    if fam == "nan_leaf":                                       # (flat_scene numbers its nodes in pre-order, as the device does)
        assert (box_bits(got, "nodes", tags[fam]["leaves"]) == EMPTY_BOX).all(), "an all-NaN leaf keeps the start values"
    if fam == "nan_object":
        assert (box_bits(got, "root_nodes", tags[fam]["objs"]) == EMPTY_BOX).all(), "an all-NaN object's root keeps the start values"
        assert (box_bits(got, "nodes", flat.obj_root[tags[fam]["objs"]]) == EMPTY_BOX).all()


# ---- b. every build of k_refit_tris -----------------------------------------------------------------------------------------------------
FORMS = (("direct xyzw aligned", False, 4, 0), ("direct xyzw float-aligned", False, 4, 4), ("direct xyz", False, 3, 4),
         ("indexed xyzw aligned", True, 4, 0), ("indexed xyzw float-aligned", True, 4, 4), ("indexed xyz", True, 3, 0))


@pytest.mark.parametrize("fam,name", [("records", "records"), (edges.BUILD_MIX, "h7")])
def test_every_build_of_refit_tris(srt, dev, fam, name):
    """The six load forms, each without and with normals, on one scene.  The xyz forms get the same points with every w taken as 1
    (they cannot carry another).  The normals hold NaN payloads of both kinds, -0 and subnormals and must come back as the same
    uint32: the flat copy, the indexed gather and the LDS staging move words.  A refit without normals leaves the rows of the one before."""
    base = edges.tree(name)
    rng = np.random.default_rng(12)
    nT = base.n_tris
    cur = edges.edge_normals(rng, nT, 9)
    flat = dataclasses.replace(base, tri_normals=cur)
    pts4, _ = edges.points(fam, name)
    pts3 = pts4.copy(); pts3[..., 3] = 1.0
    assert (pts4[..., 3] != 1.0).any()
    ds = srt.DeviceScene(flat)
    want, derived, welded = {}, {}, {}
    for stride, p in ((4, pts4), (3, pts3)):
        want[stride] = created_records(srt, edges.edge_flat(flat, p, cur))
        derived[stride] = edges.derive_ref(p)
        welded[stride] = refit_ref.weld(dataclasses.replace(flat, tri_points=p))
    prepared = None
    for what, indexed, stride, misalign in FORMS:
        p = pts4 if stride == 4 else pts3
        verts, tv = welded[stride]
        nV = verts.shape[0]
        if indexed and prepared != stride:
            ds.refit_prepare(tv, nV); prepared = stride
        elif prepared is None:
            ds.refit_prepare(); prepared = 0
        if indexed:
            assert np.array_equal(edges.bits(refit_ref.expand(verts[:, :stride], tv, stride)), edges.bits(p))
        src = dev.put(np.ascontiguousarray((verts if indexed else p.reshape(-1, 4))[:, :stride]), misalign=misalign)
        for with_normals in (False, True):
            kw = dict(stride=stride, n_verts=nV if indexed else 0)
            if with_normals:
                n_in = edges.edge_normals(rng, nV if indexed else nT, 3 if indexed else 9)
                cur = refit_ref.expand_normals(n_in, tv) if indexed else n_in
                kw["normals"] = dev.put(n_in, misalign=misalign)
            ds.refit_device(src, **kw); ds.sync()
            edges.same_records_bits(ds.records(), dict(want[stride], tri_normals=cur), f"{name}: {what}, normals {with_normals}", derived=derived[stride])
    ds.close()


# ---- c. pose ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("roots33", "sliced"))
@pytest.mark.parametrize("kind", edges.MATRIX_KINDS)
def test_pose_with_edge_matrices(srt, kind, name):
    flat = edges.tree(name)
    mats = edges.matrices(kind, flat)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    ds.pose(mats)
    got = ds.records()
    ds.close()
    want = edges.pose_flat(flat, mats)
    edges.same_records_bits(got, created_records(srt, want), f"{kind} on {name}", derived=edges.derive_ref(want.tri_points))


SOUP_MATRICES = (("identity", IDENTITY),                                                        # -0 + 0 = +0: the reference adds as the device does
                 ("scale 2^-3", np.diag(np.float32([0.125, 0.125, 0.125, 1.0])).reshape(16)),
                 ("projective", np.float32([1, 0, 0, 0.001,   0, 1, 0, -0.002,   0, 0, 1, 0.0005,   0, 0, 0, 0.75])))      # w' generic: inexact divides


def test_pose_of_the_record_soup(srt):
    """leaf_vectors.record_points() through k_pose_tris: its own copy of derive_triangle on w != 1, slivers, overflow and subnormals."""
    flat = edges.tree("records")
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    for what, m in SOUP_MATRICES:
        mats = np.tile(np.ascontiguousarray(m, np.float32), (flat.n_objects, 1))
        ds.pose(mats)
        want = edges.pose_flat(flat, mats)
        if what == "projective":
            w = want.tri_points[..., 3]
            assert (np.isfinite(w) & (w != 1.0) & (w != 0.0)).mean() > 0.9
        edges.same_records_bits(ds.records(), created_records(srt, want), f"soup, {what}", derived=edges.derive_ref(want.tri_points))
    ds.close()


# ---- d. the walks on what the refit left --------------------------------------------------------------------------------------------------
def ray_batch(name):
    if name in ts.FAMILIES:
        return ts.ray_batch(name)
    flat = edges.tree(name)
    return np.concatenate([rq.unrelated_rays(flat, ts.N_UNRELATED, seed=606), ts.aimed_rays(flat)])


@pytest.mark.parametrize("name", ("sliced", "roots33", "h7"))
def test_walks_on_a_refitted_edge_scene(srt, oracle, dev, name):
    """nan_some + nan_leaf + nan_object + inf + w: frames at 1, 9 and 16 light samples and a counting frame against the oracle on the
    exact flat scene (a box off by one bit in effect changes the counts), then the ray batch with counts."""
    flat = edges.tree(name)
    pts, _ = edges.points(edges.WALK_MIX, name)
    want = edges.edge_scene(edges.WALK_MIX, name)
    ds = srt.DeviceScene(flat); ds.refit_prepare()
    ds.refit_device(dev.put(pts), stride=4); ds.sync()
    pipes = []
    for p in (ts.frame_params(1), ts.frame_params(9), ts.frame_params(16), ts.frame_params(2, flags=abi.SRT_FLAG_COUNT_WORK)):
        o = ds.render(p)
        c = oracle.render(want, p, pow="device")
        gf.compare_exact(srt, o, c, gf.owned(p), want, p, f"{name} L {p.n_lights} flags {p.flags}")
        if p.flags & abi.SRT_FLAG_COUNT_WORK:
            assert c["stats"]["node_tests"] > 0 and c["stats"]["tri_tests"] > 0
            assert o["stats"]["node_tests"] == c["stats"]["node_tests"] and o["stats"]["tri_tests"] == c["stats"]["tri_tests"], name
        assert (c["hit_id"] >= 0).mean() >= 0.08
        pipes.append(ds.pipeline)
    assert len(set(pipes)) > 1, pipes
    rays = ray_batch(name)
    hit, t, n_node, n_tri = ts.oracle_rays(oracle, want, rays)
    q = ds.trace_rays(rays, count=True)
    bad = q["hit_id"] != hit
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(edges.bits(q["t"]), edges.bits(t)), name
    assert (q["stats"]["node_tests_primary"], q["stats"]["tri_tests_primary"]) == (n_node, n_tri), name
    assert (hit >= 0).sum() >= 20
    ds.close()


# ---- e. the scene box follows a refit and a pose --------------------------------------------------------------------------------------------
def left_half_scene():
    """Five one-node objects, all in the left half of the frame."""
    rng = np.random.default_rng(404)
    centres = [(-70.0, -35.0, 200.0), (-35.0, -30.0, 190.0), (-60.0, 5.0, 210.0), (-30.0, 30.0, 200.0), (-75.0, 40.0, 195.0)]
    objs = [dict(tris=ts.patch(rng, s, c, (8.0, 8.0, 6.0), 12.0), leaves=(s,), shape="root_leaf", color=ts.COLORS[k], material=ts.MATERIALS[k % 3])
            for k, (s, c) in enumerate(zip((9, 31, 5, 17, 12), centres))]
    flat = ts.flat_scene(objs)
    assert flat.node_max[:, 0].max() < -2.0
    return flat


def rays_miss_box(rays, lo, hi, margin):
    """float64 slab test of rays (n x 6) against [lo - margin, hi + margin]: True where the ray misses."""
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        t0, t1 = (lo - margin - o) / d, (hi + margin - o) / d
    near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
    return far < np.maximum(near, 0.0)


def test_scene_box_follows_a_refit_and_a_pose(srt, oracle, dev):
    """One object goes to the right half, entirely outside the created scene's union box, and comes back -- by refit, then by pose.
    The pixels that see it there are rays that miss the OLD union box: a scene box that was not refreshed drops exactly those."""
    flat = left_half_scene()
    k, shift = 1, np.float32(110.0)
    moved = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4).copy()
    moved[flat.tri_obj == k, :, 0] += shift
    want = edges.edge_flat(flat, moved)
    p = ts.frame_params(2)
    c = oracle.render(want, p, pow="device")
    sees = (c["hit_id"] >= 0) & (want.tri_obj[np.maximum(c["hit_id"], 0)] == k)
    lo, hi = flat.node_min[flat.obj_root].astype(np.float64).min(0), flat.node_max[flat.obj_root].astype(np.float64).max(0)
    assert sees.sum() >= 50 and rays_miss_box(ts.frame_rays()[sees.reshape(-1)], lo, hi, 1.0).all(), int(sees.sum())
    c0 = oracle.render(flat, p, pow="device")
    translate = np.tile(IDENTITY, (flat.n_objects, 1)); translate[k, 12] = shift
    assert np.array_equal(edges.bits(pose_ref.transform_objects(flat, translate)), edges.bits(moved))
    ds = srt.DeviceScene(flat); ds.refit_prepare(); ds.set_pose_source()
    there, back = dev.put(moved), dev.put(flat.tri_points)
    for what, go, come in (("refit", lambda: ds.refit_device(there, stride=4), lambda: ds.refit_device(back, stride=4)),
                           ("pose", lambda: ds.pose(translate), lambda: ds.pose(np.tile(IDENTITY, (flat.n_objects, 1))))):
        go(); ds.sync()
        o = ds.render(p)
        assert (o["hit_id"][sees] >= 0).all(), f"{what}: the moved object is seen outside the created scene's box"
        gf.compare_exact(srt, o, c, gf.owned(p), want, p, f"{what}: moved")
        come(); ds.sync()
        gf.compare_exact(srt, ds.render(p), c0, gf.owned(p), flat, p, f"{what}: back")
    ds.close()


# ---- f. order and determinism ---------------------------------------------------------------------------------------------------------------
def test_refits_are_deterministic_and_leave_nothing_behind(srt, dev):
    """Two refits from one buffer: the same bytes.  Edge points, then the original points: the created scene's records byte for byte
    -- nothing non-finite lingers in the triangles' own boxes or in the box arrays."""
    name = "h7"
    flat = edges.tree(name)
    fams = ("zeros", "subnormal", "fltmax", "nan_some", "nan_leaf", "nan_object", "inf", "w")      # (zeros first: it needs z > 0 as created)
    assert set(fams) == set(edges.FAMILIES)
    pts, _ = edges.points(fams, name)
    ds = srt.DeviceScene(flat); ds.refit_prepare()
    created = ds.records()
    edge, plain = dev.put(pts), dev.put(flat.tri_points)
    ds.refit_device(edge, stride=4); ds.sync()
    first = ds.records()
    edges.same_records_bits(first, created_records(srt, edges.edge_scene(fams, name)), "every family at once", derived=edges.derive_ref(pts))
    ds.refit_device(edge, stride=4); ds.sync()
    refit_ref.same_bytes(ds.records(), first, "the same buffer twice")
    ds.refit_device(plain, stride=4); ds.sync()
    refit_ref.same_bytes(ds.records(), created, "the original points after the edge points")
    ds.close()
