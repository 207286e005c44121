"""GPU (-m gpu): srt_nearest_points and its _device form (include/srt_nearest.h) -- every output bit for bit against srt_closest_points on
the same handle and against tests/point_ref.py, on the cube, the scene and batches of tests/point_edges.py, ground_bunny and the nesting
trees of tests/tree_shapes.py, at 1, 63, 64, 65 and 257 points; the radii around the winner's own distance; masks; after a pose and a
refit; the order of the points (alone, reversed, interleaved with far-away points); the counters between the mandatory set
(tests/nearest_ref.py) and srt_closest_points'; on the trees that do not nest, what the header still promises.  Every point used here on
a nesting scene is checked against the margin on the CPU by tests/test_nearest_ref.py (fixtures())."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_ref as nr
import point_edges as pe
import point_ref as pr
import pose_ref
import test_gpu_points as tp
import tree_shapes as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
INF = F(np.inf)
NESTING_SCENES = ("cube", "ground_bunny", "sliced", "comb256", "roots33", "roots300", "shuffled")
POSED = ("sliced", "roots33")
COUNTS = tp.COUNTS
N = tp.N


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def far_points(flat, n, seed=41):
    """n points 20 to 60 scene extents away from the scene, in every direction."""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(flat.tri_points, F)[..., :3].reshape(-1, 3)
    mn, mx = P.min(0), P.max(0)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return ((mn + mx) / 2 + d * np.linalg.norm(mx - mn) * rng.uniform(20, 60, (n, 1))).astype(F)


def moved_points(flat):
    """The vertices srt_scene_refit_device gets in the refit case: a bend no matrix does."""
    moved = np.ascontiguousarray(flat.tri_points, F).reshape(-1, 3, 4).copy()
    moved[..., 1] += F(6.0) * np.sin(F(0.05) * moved[..., 0])
    moved[..., 2] += F(3.0)
    return moved


def pose_mats(flat):
    return np.stack([tp.turn(k, flat.n_objects) for k in range(flat.n_objects)])


def fixtures():
    """(label, flat scene, points) of every call these tests make on a scene whose boxes nest."""
    import refit_ref
    for name in NESTING_SCENES:
        flat, pts, _, _ = tp.case(name)
        yield name, flat, pts
        yield name + ", far", flat, far_points(flat, N)
    for name in POSED:
        flat, pts, _, _ = tp.case(name)
        yield name + ", posed", pose_ref.pose_flat(flat, pose_mats(flat)), pts
    flat, pts, _, _ = tp.case("ground_bunny")
    yield "ground_bunny, refitted", refit_ref.refit_flat(flat, moved_points(flat)), pts


def edge_points():
    """tests/point_edges.py's scene is NOT one whose boxes nest: the fold that makes a leaf's box loses every vertex after a NaN, so the box
    of the leaf with the NaN and the inf triangle leaves out a vertex of the finite triangle beside them.  The equality is asserted on
    it all the same; tests/test_nearest_ref.py checks what it rests on for these points (nearest_ref.winners_hold and the simulated walk)."""
    return (pe.scene(),) + pe.batches()["all"]


def same_as_closest(ds, flat, pts, rad, what, want=None, pm=None, obj_mask=None, strictly=False, floor=True):
    """Both calls on the same handle: equal bits, hits; the counters between the mandatory set's and srt_closest_points'."""
    near = ds.nearest_points(pts, radius=rad, point_mask=pm, count=True)
    close = ds.closest_points(pts, radius=rad, point_mask=pm, count=True)
    pr.same(near, close, what + ": against srt_closest_points")
    if want is not None:
        pr.same(near, want, what + ": against the yardstick")
    a, b = near["stats"], close["stats"]
    if floor:
        need_nodes, need_tris = nr.mandatory(flat, pts, close["dist2"], rad, point_mask=None if pm is None or pm is True else pm, obj_mask=obj_mask)
    else:                                             # (the large scene: the floor is computed for some of its calls)
        need_nodes = need_tris = np.zeros(1, np.int64)
    print(what, "points", len(pts), "node tests", int(need_nodes.sum()), "<=", a["node_tests_primary"], "<=", b["node_tests_primary"],
          "triangle tests", int(need_tris.sum()), "<=", a["tri_tests_primary"], "<=", b["tri_tests_primary"])
    assert (a["primary_rays"], a["hit_rays"]) == (b["primary_rays"], b["hit_rays"]), what
    assert need_nodes.sum() <= a["node_tests_primary"] <= b["node_tests_primary"], what
    assert need_tris.sum() <= a["tri_tests_primary"] <= b["tri_tests_primary"], what
    if strictly:
        assert a["node_tests_primary"] < b["node_tests_primary"] and a["tri_tests_primary"] < b["tri_tests_primary"], what
    plain = ds.nearest_points(pts, radius=rad, point_mask=pm)
    pr.same(plain, close, what + ", no counting")
    assert plain["stats"]["hit_rays"] == b["hit_rays"] and plain["stats"]["node_tests_primary"] == 0 and plain["stats"]["tri_tests_primary"] == 0
    return near


def around(d2):
    """The radii around a winner's distance: the least r with r * r >= dist2 (the winner qualifies, closed), its neighbours above and below."""
    with np.errstate(invalid="ignore"):
        r = np.sqrt(d2).astype(F)
        for _ in range(4):
            r = np.where(r * r < d2, np.nextafter(r, INF), r).astype(F)
        for _ in range(4):
            lower = np.nextafter(r, F(0.0))
            r = np.where((lower * lower >= d2) & (r > 0), lower, r).astype(F)
    return r, np.nextafter(r, INF), np.nextafter(r, F(0.0))


@pytest.mark.parametrize("name", NESTING_SCENES)
def test_against_closest_points(srt, name):
    flat, pts, rad, want = tp.case(name)
    assert nr.nests(flat)
    small = flat.n_tris < 10000
    ds = srt.DeviceScene(flat)
    for n in COUNTS:
        same_as_closest(ds, flat, pts[:n], rad[:n], f"{name}, {n} points", pr.first(want, n), floor=small or n == N)
    # no radius: the winner is brute force, and the shrinking walk tests less than the scene
    inf = same_as_closest(ds, flat, pts, None, name + ", no radius", strictly=(name == "ground_bunny"))
    tri, d2 = pr.brute_force(flat, pts[:65])
    assert np.array_equal(inf["tri"][:65], tri) and np.array_equal(inf["dist2"][:65].view(np.uint32), d2.view(np.uint32))
    pr.same(ds.nearest_points(pts, radius=np.inf), inf, name + ", one radius for all")
    # the radii around the winner's own distance, and the radii that find nothing or walk nothing
    at, above, below = around(inf["dist2"])
    # (the winner qualifies at r * r == dist2, but the b2 of a box above it can lie over its dist2 -- the very thing the margin is for --
    # and then BOTH calls find nothing: what is asserted is the equality, and the winner wherever one is found)
    for r, what in ((at, "at"), (above, "above")):
        got = same_as_closest(ds, flat, pts, r, f"{name}, radius {what} the distance", pr.closest_points(flat, pts, r) if small else None, floor=small)
        found = got["tri"] >= 0
        assert found.mean() > 0.9
        pr.same({k: got[k][found] for k in pr.SAME_KEYS}, {k: inf[k][found] for k in pr.SAME_KEYS}, f"{name}, radius {what} the distance: the winner")
    got = same_as_closest(ds, flat, pts, below, name + ", radius below the distance", floor=small)
    assert (got["tri"][inf["dist2"] > 0] == -1).all()
    for r in (0.0, -0.0, -1.0, np.nan):
        got = same_as_closest(ds, flat, pts, np.full(N, r, F), f"{name}, radius {r}", pr.closest_points(flat, pts, np.full(N, r, F)), floor=small)
        assert (got["tri"] == -1).all() or r == 0.0
    # any output may be NULL
    only = ds.nearest_points(pts, radius=rad, want=("vw",))
    assert set(only) == {"vw", "stats"} and np.array_equal(only["vw"].view(np.uint32), want["vw"].view(np.uint32))
    assert ds.nearest_points(pts, radius=rad, want=())["stats"]["hit_rays"] == want["hits"]
    ds.close()


@pytest.mark.parametrize("name", NESTING_SCENES)
def test_the_order_of_the_points(srt, name):
    """What a naive shrinking walk loses: the same 257 points alone, reversed, and interleaved with 257 far-away points -- other waves,
    other flushes, other bounds at every node -- give the same bits per point."""
    flat, pts, _, _ = tp.case(name)
    ds = srt.DeviceScene(flat)
    alone = ds.nearest_points(pts)
    pr.same(alone, ds.closest_points(pts), name)
    pr.same(ds.nearest_points(pts[::-1]), {k: alone[k][::-1] for k in pr.SAME_KEYS}, name + ", reversed")
    far = far_points(flat, N)
    mixed = np.empty((2 * N, 3), F)
    mixed[0::2], mixed[1::2] = pts, far
    both = ds.nearest_points(mixed)
    pr.same({k: both[k][0::2] for k in pr.SAME_KEYS}, alone, name + ", interleaved")
    pr.same(both, ds.closest_points(mixed), name + ", interleaved, against srt_closest_points")
    perm = np.random.default_rng(3).permutation(2 * N)
    pr.same(ds.nearest_points(mixed[perm]), {k: both[k][perm] for k in pr.SAME_KEYS}, name + ", permuted")
    ds.close()


NAMES = tuple(pe.batches())


@pytest.mark.parametrize("name", NAMES)
def test_edges(srt, name):
    """The batches of tests/point_edges.py: points on every Voronoi border and one ulp off it, radii at and one ulp below the distance, 0,
    -0, -1, NaN, points that are NaN, inf or 1e19, zero-area and non-finite triangles, an empty leaf: equal bits, nothing pruned wrongly."""
    flat = pe.scene()
    p, r = pe.batches()[name]
    ds = srt.DeviceScene(flat)
    same_as_closest(ds, flat, p, r, name, pr.closest_points(flat, p, r))
    ds.close()


@pytest.mark.parametrize("name,hide", [("sliced", 1), ("roots33", 32)])
def test_masks(srt, name, hide):
    objects = {"sliced": ts.sliced_objects, "roots33": lambda: ts.roots_objects(33)}[name]()
    full, less, ids = tp.reduced(objects, hide)
    _, pts, rad, want = tp.case(name)
    ds = srt.DeviceScene(full)
    same_as_closest(ds, full, pts, rad, name + ", masks of all ones", want, pm=np.full(N, 0xFFFFFFFF, np.uint32))
    om = np.where(np.arange(full.n_objects) == hide, 2, 1 | (4 << (np.arange(full.n_objects) % 8))).astype(np.uint32)
    ds.set_object_masks(om)
    for radius in (rad, None):
        small = pr.closest_points(less, pts, radius)
        w = dict(small, tri=np.where(small["tri"] >= 0, ids[np.maximum(small["tri"], 0)], -1).astype(np.int32))
        got = same_as_closest(ds, full, pts, radius, f"{name}, object {hide} hidden", w, pm=np.full(N, 1, np.uint32), obj_mask=om)
        assert not np.isin(got["tri"], np.flatnonzero(full.tri_obj == hide)).any()
        pm = np.resize(np.uint32([0xFFFFFFFF, 1, 2, 0, 4, 8]), N)
        got = same_as_closest(ds, full, pts, radius, name + ", a mask per point", pr.closest_points(full, pts, radius, point_mask=pm, obj_mask=om), pm=pm, obj_mask=om)
        assert (got["tri"][pm == 0] == -1).all()
    same_as_closest(ds, full, pts, None, name + ", unmasked beside a table")
    ds.close()


@pytest.mark.parametrize("name", POSED)
def test_after_pose(srt, name):
    flat, pts, rad, before = tp.case(name)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = pose_mats(flat)
    ds.pose(mats)
    moved = pose_ref.pose_flat(flat, mats)
    assert nr.nests(moved)
    got = same_as_closest(ds, moved, pts, rad, name + ", posed", pr.closest_points(moved, pts, rad))
    assert not np.array_equal(got["dist2"], before["dist2"])
    same_as_closest(ds, moved, pts, None, name + ", posed, no radius", pr.closest_points(moved, pts))
    ds.close()


@pytest.mark.parametrize("name", ["loose", "shrunk"])
def test_trees_that_do_not_nest(srt, name):
    """No equality is claimed: the call returns, finds a triangle wherever srt_closest_points does, the outputs are the returned triangle's
    own, and its dist2 is not below srt_closest_points'."""
    flat = ts.family(name)
    assert not nr.nests(flat)
    pts, ext = tp.points_for(flat, N, 17)
    rec = pr.records_of(flat)
    ds = srt.DeviceScene(flat)
    for rad in (None, tp.radii_for(ext, N, 17, 64)):
        near, close = ds.nearest_points(pts, radius=rad, count=True), ds.closest_points(pts, radius=rad, count=True)
        assert np.array_equal(near["tri"] >= 0, close["tri"] >= 0)
        hit = near["tri"] >= 0
        own = pr.closest_on_triangles(pts[hit], rec[near["tri"][hit]])
        own = dict(tri=near["tri"][hit], dist2=own["dist2"], point=own["point"], vw=np.stack([own["v"], own["w"]], 1), region=own["region"])
        pr.same({k: near[k][hit] for k in pr.SAME_KEYS}, own, name + ": the returned triangle's own outputs")
        assert (near["dist2"] >= close["dist2"]).all()
        if rad is not None:
            with np.errstate(invalid="ignore"):
                assert (near["dist2"][hit] <= (rad * rad)[hit]).all()
        assert near["stats"]["node_tests_primary"] <= close["stats"]["node_tests_primary"] and near["stats"]["tri_tests_primary"] <= close["stats"]["tri_tests_primary"]
        print(name, "other winners than srt_closest_points:", int((near["tri"] != close["tri"]).sum()), "of", N)
    ds.close()


def test_argument_errors(srt):
    import ctypes as C
    from simple_raytracer_amd import abi
    L = srt.load()
    ds = srt.DeviceScene(pe.scene())
    f32p = C.POINTER(C.c_float)
    pts = np.zeros((4, 3), F)
    tri = np.full(4, -7, np.int32)
    po = abi.PointOut(tri.ctypes.data, None, None, None, None)
    ok = L.srt_nearest_points
    assert ok(ds.h, 0, None, None, None, 0, C.byref(po), None) == abi.SRT_OK
    assert ok(None, 4, pts.ctypes.data_as(f32p), None, None, 0, C.byref(po), None) == abi.SRT_ERR_ARG
    assert ok(ds.h, 4, None, None, None, 0, C.byref(po), None) == abi.SRT_ERR_ARG
    assert ok(ds.h, 4, pts.ctypes.data_as(f32p), None, None, 0, None, None) == abi.SRT_ERR_ARG
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT, 1 << 9):
        assert ok(ds.h, 4, pts.ctypes.data_as(f32p), None, None, flags, C.byref(po), None) == abi.SRT_ERR_ARG, flags
        assert L.srt_nearest_points_device(ds.h, 4, None, None, None, flags, None, C.byref(po)) == abi.SRT_ERR_ARG
    assert L.srt_nearest_points_device(ds.h, 4, None, None, None, 0, None, C.byref(po)) == abi.SRT_ERR_ARG
    assert L.srt_nearest_points_device(ds.h, 0, None, None, None, 0, None, C.byref(po)) == abi.SRT_OK
    assert L.srt_nearest_points_device(ds.h, 4, None, None, None, 0, None, None) == abi.SRT_ERR_ARG
    assert (tri == -7).all()
    o = ds.nearest_points(np.zeros((0, 3), F))
    assert o["tri"].shape == (0,) and o["point"].shape == (0, 3) and o["stats"]["primary_rays"] == 0
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "nearest_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"nearest {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_point():
    """Device pointers from torch tensors: a second stream beside a pending render, the host form's bits, float-aligned pointers, a
    shared handle, masks (own process: torch initialises HIP first)."""
    run_case("device")


def test_after_refit_device():
    """srt_scene_refit_device from a torch tensor, then both calls on the same stream: equal bits, and the yardstick on the moved scene."""
    run_case("refit")


def test_captured_into_a_hip_graph():
    """srt_nearest_points_device captured once into a hipGraph and replayed twice: the same bits."""
    run_case("graph")
