"""GPU (-m gpu): srt_closest_points_multi, srt_nearest_points_multi and their _device forms (include/srt_points_multi.h) -- every output bit
for bit against tests/points_multi_ref.py, column 0 against srt_closest_points on the same handle, the nearest form against the closest
form, on the scenes and the 257 points of tests/test_gpu_points.py at 1, 63, 64, 65 and 257 points and k = 1, 3, 4, 5, 8, 9, 16 (both sides
of every slot count the kernel is built with); the counters -- the closest form's exactly srt_closest_points', the nearest form's between
the mandatory set's and those --; the batches of tests/point_edges.py; ties; masks; after a pose; the order of the points; NULL outputs;
argument errors; on the trees that do not nest, what the header still promises.  tests/test_points_multi_ref.py checks on the CPU that
these inputs reach the empty columns, the partly filled rows and the overflow of the last slot."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import nearest_ref as nr
import point_edges as pe
import point_ref as pr
import points_multi_ref as pm
import pose_ref
import test_gpu_nearest as tn
import test_gpu_points as tp
import tree_shapes as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SCENES = ("cube", "sliced", "roots33", "comb256", "shuffled", "ground_bunny")
KS = (1, 3, 4, 5, 8, 9, 16)
COUNTS = tp.COUNTS
N = tp.N


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@functools.lru_cache(maxsize=None)
def cands(name, radii=True):
    """The yardstick's candidates of tests/test_gpu_points.case(name), with its radii or without a radius: made once, for every k."""
    flat, pts, rad, _ = tp.case(name)
    return pm.candidates(flat, pts, rad if radii else None)


def closest_is_the_yardstick(ds, pts, rad, k, want, what, pmask=None):
    got = ds.closest_points_multi(pts, k, radius=rad, point_mask=pmask, count=True)
    pm.same(got, want, what)
    pm.same_counts(got["stats"], want, len(pts), what)
    return got


def nearest_is_the_closest_form(ds, flat, pts, rad, k, close, what, want=None, pmask=None, obj_mask=None, floor=True, strictly=False):
    """The nearest form against the closest form's result `close` on the same handle (and the yardstick): equal columns and n_found; the
    counters between the mandatory set's and the closest form's."""
    near = ds.nearest_points_multi(pts, k, radius=rad, point_mask=pmask, count=True)
    pm.same(near, close, what + ": against the closest form", pm.SAME_KEYS[1:])
    assert "n_within" not in near
    if want is not None:
        pm.same(near, want, what + ": against the yardstick")
    a, b = near["stats"], close["stats"]
    need_nodes = need_tris = np.zeros(1, np.int64)
    if floor:
        need_nodes, need_tris = pm.mandatory(flat, pts, close, k, rad, point_mask=None if pmask is None or pmask is True else pmask, obj_mask=obj_mask)
    print(what, "k", k, "points", len(pts), "node tests", int(need_nodes.sum()), "<=", a["node_tests_primary"], "<=", b["node_tests_primary"],
          "triangle tests", int(need_tris.sum()), "<=", a["tri_tests_primary"], "<=", b["tri_tests_primary"])
    assert (a["primary_rays"], a["hit_rays"]) == (b["primary_rays"], b["hit_rays"]), what
    assert need_nodes.sum() <= a["node_tests_primary"] <= b["node_tests_primary"], what
    assert need_tris.sum() <= a["tri_tests_primary"] <= b["tri_tests_primary"], what
    if strictly:
        assert a["node_tests_primary"] < b["node_tests_primary"] and a["tri_tests_primary"] < b["tri_tests_primary"], what
    return near


@pytest.mark.parametrize("name", SCENES + ("loose",))
def test_closest_form_against_the_yardstick(srt, name):
    flat, pts, rad, single = tp.case(name)
    cand = cands(name)
    ds = srt.DeviceScene(flat)
    one = ds.closest_points(pts, radius=rad, count=True)
    for k in KS:
        want = pm.columns(cand, k)
        for n in COUNTS:
            closest_is_the_yardstick(ds, pts[:n], rad[:n], k, pm.first(want, n), f"{name}, k {k}, {n} points")
        got = ds.closest_points_multi(pts, k, radius=rad)
        pm.same(got, want, f"{name}, k {k}, no counting")
        assert got["stats"]["hit_rays"] == want["hits"] and got["stats"]["node_tests_primary"] == 0 and got["stats"]["tri_tests_primary"] == 0
        # column 0 is srt_closest_points on the same handle; the counters are its counters
        pr.same({key: got[key][:, 0] for key in pr.SAME_KEYS}, one, f"{name}, k {k}: column 0")
        counted = ds.closest_points_multi(pts, k, radius=rad, count=True, want=("n_found",))["stats"]
        assert counted == one["stats"], (name, k, counted, one["stats"])
    k = 5
    want = pm.columns(cand, k)
    # any output may be NULL; n_within alone; nothing wanted still counts the hits
    for key in pm.SAME_KEYS:
        only = ds.closest_points_multi(pts, k, radius=rad, want=(key,))
        assert set(only) == {key, "stats"}
        pm.same(only, want, f"{name}: only {key}")
        rest = ds.closest_points_multi(pts, k, radius=rad, want=tuple(x for x in pm.SAME_KEYS if x != key))
        assert key not in rest
        pm.same(rest, want, f"{name}: all but {key}")
    assert ds.closest_points_multi(pts, k, radius=rad, want=())["stats"]["hit_rays"] == want["hits"]
    # another order of the points gives the same rows in that order
    perm = np.random.default_rng(3).permutation(N)
    pm.same(ds.closest_points_multi(pts[perm], k, radius=rad[perm]), pm.rows(want, perm), name + ", permuted")
    # no radius: every triangle within
    if flat.n_tris < 10000:
        free = pm.columns(cands(name, False), 16)
        assert (free["n_within"] <= flat.n_tris).all() and free["tri_tests"] == N * flat.n_tris
        closest_is_the_yardstick(ds, pts, None, 16, free, name + ", no radius")
    ds.close()


@pytest.mark.parametrize("name", SCENES)
def test_nearest_form(srt, name):
    flat, pts, rad, _ = tp.case(name)
    assert nr.nests(flat)
    small = flat.n_tris < 10000
    cand = cands(name)
    ds = srt.DeviceScene(flat)
    for k in KS:
        want = pm.columns(cand, k)
        for n in COUNTS:
            w = pm.first(want, n)
            close = ds.closest_points_multi(pts[:n], k, radius=rad[:n], count=True)
            nearest_is_the_closest_form(ds, flat, pts[:n], rad[:n], k, close, f"{name}, {n} points", w, floor=small or (n == N and k == 16))
        plain = ds.nearest_points_multi(pts, k, radius=rad)
        pm.same(plain, want, f"{name}, k {k}, no counting")
        assert plain["stats"]["hit_rays"] == want["hits"] and plain["stats"]["node_tests_primary"] == 0 and plain["stats"]["tri_tests_primary"] == 0
    # no radius: the walk tests less than the scene; column 0 is srt_nearest_points
    one = ds.nearest_points(pts)
    for k in (1, 4, 16):
        close = ds.closest_points_multi(pts, k, count=True)
        near = nearest_is_the_closest_form(ds, flat, pts, None, k, close, name + ", no radius", pm.columns(cands(name, False), k) if small else None,
                                           floor=small or k == 16, strictly=(name == "ground_bunny"))
        pr.same({key: near[key][:, 0] for key in pr.SAME_KEYS}, one, f"{name}, no radius, k {k}: column 0")
        assert (near["n_found"] == min(k, flat.n_tris)).all()
    # any output may be NULL
    want = pm.columns(cand, 5)
    for key in pm.SAME_KEYS[1:]:
        only = ds.nearest_points_multi(pts, 5, radius=rad, want=(key,))
        assert set(only) == {key, "stats"}
        pm.same(only, want, f"{name}: only {key}")
    assert ds.nearest_points_multi(pts, 5, radius=rad, want=())["stats"]["hit_rays"] == want["hits"]
    ds.close()


@pytest.mark.parametrize("name", SCENES)
def test_the_order_of_the_points(srt, name):
    """The same 257 points alone, reversed, permuted and interleaved with 257 far-away points -- other waves, other flushes, other bounds at
    every node -- give the same rows per point, in both forms."""
    flat, pts, _, _ = tp.case(name)
    ds = srt.DeviceScene(flat)
    far = tn.far_points(flat, N)
    mixed = np.empty((2 * N, 3), F)
    mixed[0::2], mixed[1::2] = pts, far
    perm = np.random.default_rng(3).permutation(2 * N)
    for k in (3, 16):
        alone = ds.closest_points_multi(pts, k)
        both = ds.closest_points_multi(mixed, k)
        pm.same(pm.rows(both, slice(0, None, 2)), alone, f"{name}, k {k}, interleaved")
        near = ds.nearest_points_multi(pts, k)
        pm.same(near, alone, f"{name}, k {k}, nearest form", pm.SAME_KEYS[1:])
        pm.same(ds.nearest_points_multi(pts[::-1], k), pm.rows(near, slice(None, None, -1)), f"{name}, k {k}, reversed")
        nboth = ds.nearest_points_multi(mixed, k)
        pm.same(nboth, both, f"{name}, k {k}, interleaved, nearest form", pm.SAME_KEYS[1:])
        pm.same(ds.nearest_points_multi(mixed[perm], k), pm.rows(nboth, perm), f"{name}, k {k}, permuted")
        pm.same(ds.closest_points_multi(mixed[perm], k), pm.rows(both, perm), f"{name}, k {k}, permuted, closest form")
    ds.close()


EDGE_NAMES = tuple(pe.batches())


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_edges(srt, name):
    """The batches of tests/point_edges.py: points on every Voronoi border and one ulp off it, radii at and one ulp below a distance, 0, -0,
    -1, NaN, points that are NaN, inf or 1e19, zero-area and non-finite triangles, an empty leaf; object 1 repeats object 0, so every
    column there has its tie.  (The scene does not nest, tests/test_gpu_nearest.edge_points; the equality is asserted all the same.)"""
    flat = pe.scene()
    p, r = pe.batches()[name]
    cand = pm.candidates(flat, p, r)
    ds = srt.DeviceScene(flat)
    for k in (1, 3, 16):
        want = pm.columns(cand, k)
        close = closest_is_the_yardstick(ds, p, r, k, want, f"{name}, k {k}")
        nearest_is_the_closest_form(ds, flat, p, r, k, close, f"{name}, k {k}", want)
    ds.close()


def test_ties(srt):
    """Points exactly on the cube's eight vertices and on three edge midpoints: the triangles that share the vertex or the edge all come
    back, equal dist2 bits, lowest id first."""
    flat = gu.GoldenScene("cube").flat
    pts = pm.tie_batch(flat)
    ds = srt.DeviceScene(flat)
    for k in (3, 8, 16):
        want = pm.closest_points_multi(flat, pts, k)
        close = closest_is_the_yardstick(ds, pts, None, k, want, f"ties, k {k}")
        near = nearest_is_the_closest_form(ds, flat, pts, None, k, close, f"ties, k {k}", want)
        assert (pm.equal_runs(near)[:8] >= 3).all()
        zero = closest_is_the_yardstick(ds, pts, 0.0, k, pm.closest_points_multi(flat, pts, k, 0.0), f"ties, radius 0, k {k}")
        assert (zero["n_within"][:8] >= 3).all()
    ds.close()


@pytest.mark.parametrize("name,hide", [("sliced", 1), ("roots33", 32)])
def test_masks(srt, name, hide):
    objects = {"sliced": ts.sliced_objects, "roots33": lambda: ts.roots_objects(33)}[name]()
    full, less, ids = tp.reduced(objects, hide)
    _, pts, rad, _ = tp.case(name)
    ds = srt.DeviceScene(full)
    om = np.where(np.arange(full.n_objects) == hide, 2, 1 | (4 << (np.arange(full.n_objects) % 8))).astype(np.uint32)
    each = np.resize(np.uint32([0xFFFFFFFF, 1, 2, 0, 4, 8]), N)
    for k in (4, 9):
        want = pm.columns(cands(name), k)
        # all ones, by a table never set or of ones, and masks of ones: the unmasked call's bits and counts
        for table in (None, np.full(full.n_objects, 0xFFFFFFFF, np.uint32)):
            if table is not None:
                ds.set_object_masks(table)
            for pmask in (True, np.full(N, 0xFFFFFFFF, np.uint32)):
                close = closest_is_the_yardstick(ds, pts, rad, k, want, f"{name}, all ones", pmask)
                nearest_is_the_closest_form(ds, full, pts, rad, k, close, f"{name}, all ones", want, pmask=pmask)
        ds.set_object_masks(om)
        for radius in (rad, None):
            # object `hide` hidden from every point: the reduced scene's result, its ids renumbered
            small = pm.closest_points_multi(less, pts, k, radius)
            w = dict(small, tri=np.where(small["tri"] >= 0, ids[np.maximum(small["tri"], 0)], -1).astype(np.int32))
            ones = np.full(N, 1, np.uint32)
            close = closest_is_the_yardstick(ds, pts, radius, k, w, f"{name}, object {hide} hidden", ones)
            nearest_is_the_closest_form(ds, full, pts, radius, k, close, f"{name}, object {hide} hidden", w, pmask=ones, obj_mask=om)
            assert not np.isin(close["tri"], np.flatnonzero(full.tri_obj == hide)).any()
            # a mask per point: some see everything, some all but `hide`, some only `hide`, some nothing
            w = pm.closest_points_multi(full, pts, k, radius, point_mask=each, obj_mask=om)
            close = closest_is_the_yardstick(ds, pts, radius, k, w, f"{name}, a mask per point", each)
            nearest_is_the_closest_form(ds, full, pts, radius, k, close, f"{name}, a mask per point", w, pmask=each, obj_mask=om)
            assert (close["tri"][each == 0] == -1).all() and (close["n_within"][each == 0] == 0).all()
        # the unmasked call ignores the table
        closest_is_the_yardstick(ds, pts, rad, k, want, f"{name}, unmasked beside a table")
        ds.set_object_masks(np.full(full.n_objects, 0xFFFFFFFF, np.uint32))
    ds.close()


@pytest.mark.parametrize("name", ["sliced", "roots33"])
def test_after_pose(srt, name):
    """srt_scene_pose moves the records both forms read: the yardstick on pose_ref's flat scene."""
    flat, pts, rad, _ = tp.case(name)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = tn.pose_mats(flat)
    ds.pose(mats)                                               # asynchronous on the scene's own stream: the queries are ordered behind it
    moved = pose_ref.pose_flat(flat, mats)
    assert nr.nests(moved)
    before = pm.columns(cands(name), 8)
    for radius in (rad, None):
        want = pm.closest_points_multi(moved, pts, 8, radius)
        close = closest_is_the_yardstick(ds, pts, radius, 8, want, name + ", posed")
        nearest_is_the_closest_form(ds, moved, pts, radius, 8, close, name + ", posed", want)
    assert not np.array_equal(pm.closest_points_multi(moved, pts, 8, rad)["dist2"], before["dist2"])
    ds.close()


@pytest.mark.parametrize("name", ["loose", "shrunk"])
def test_trees_that_do_not_nest(srt, name):
    """No equality is claimed of the nearest form: every filled column is a qualifying candidate with its own outputs, the columns are
    sorted and distinct, n_found is the closest form's, and column j's dist2 is not below the closest form's."""
    flat = ts.family(name)
    assert not nr.nests(flat)
    pts, ext = tp.points_for(flat, N, 17)
    ds = srt.DeviceScene(flat)
    for rad in (None, tp.radii_for(ext, N, 17, 64)):
        for k in (1, 4, 16):
            want = pm.closest_points_multi(flat, pts, k, rad)
            close = closest_is_the_yardstick(ds, pts, rad, k, want, f"{name}, k {k}")
            near = ds.nearest_points_multi(pts, k, radius=rad, count=True)
            pm.own_outputs(flat, pts, near)
            assert np.array_equal(near["n_found"], close["n_found"])
            assert (near["dist2"] >= close["dist2"]).all()
            if rad is not None:
                with np.errstate(invalid="ignore"):
                    assert (near["dist2"] <= (rad * rad)[:, None])[near["tri"] >= 0].all()
            assert near["stats"]["hit_rays"] == close["stats"]["hit_rays"]
            assert near["stats"]["node_tests_primary"] <= close["stats"]["node_tests_primary"] and near["stats"]["tri_tests_primary"] <= close["stats"]["tri_tests_primary"]
            print(name, "k", k, "rows that differ from the closest form's:", int((near["tri"] != close["tri"]).any(1).sum()), "of", N)
    ds.close()


def test_argument_errors(srt):
    import ctypes as C
    from simple_raytracer_amd import abi
    L = srt.load()
    ds = srt.DeviceScene(pe.scene())
    f32p = C.POINTER(C.c_float)
    pts = np.zeros((4, 3), F)
    p = pts.ctypes.data_as(f32p)
    tri, nw = np.full((4, 16), -7, np.int32), np.full(4, 77, np.uint32)
    po = abi.PointMultiOut(None, None, tri.ctypes.data, None, None, None, None)
    with_n = abi.PointMultiOut(nw.ctypes.data, None, tri.ctypes.data, None, None, None, None)
    for host, dev in ((L.srt_closest_points_multi, L.srt_closest_points_multi_device), (L.srt_nearest_points_multi, L.srt_nearest_points_multi_device)):
        assert host(ds.h, 0, None, None, None, 4, 0, C.byref(po), None) == abi.SRT_OK
        assert host(None, 4, p, None, None, 4, 0, C.byref(po), None) == abi.SRT_ERR_ARG
        assert host(ds.h, 4, None, None, None, 4, 0, C.byref(po), None) == abi.SRT_ERR_ARG
        assert host(ds.h, 4, p, None, None, 4, 0, None, None) == abi.SRT_ERR_ARG
        for k in (0, 17, 1 << 31):
            assert host(ds.h, 4, p, None, None, k, 0, C.byref(po), None) == abi.SRT_ERR_ARG, k
            assert dev(ds.h, 4, 0x1000, None, None, k, 0, None, C.byref(po)) == abi.SRT_ERR_ARG, k
            assert host(ds.h, 0, None, None, None, k, 0, C.byref(po), None) == abi.SRT_ERR_ARG, k
        for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT, 1 << 9):
            assert host(ds.h, 4, p, None, None, 4, flags, C.byref(po), None) == abi.SRT_ERR_ARG, flags
            assert dev(ds.h, 4, 0x1000, None, None, 4, flags, None, C.byref(po)) == abi.SRT_ERR_ARG, flags
        assert dev(ds.h, 4, None, None, None, 4, 0, None, C.byref(po)) == abi.SRT_ERR_ARG
        assert dev(ds.h, 0, None, None, None, 4, 0, None, C.byref(po)) == abi.SRT_OK
        assert dev(ds.h, 4, 0x1000, None, None, 4, 0, None, None) == abi.SRT_ERR_ARG
        assert dev(ds.h, 4, 0x1000, None, None, 4, 0, None, C.byref(abi.PointMultiOut())) == abi.SRT_OK      # nothing wanted: nothing launched
    # n_within is not defined under pruning
    assert L.srt_nearest_points_multi(ds.h, 4, p, None, None, 4, 0, C.byref(with_n), None) == abi.SRT_ERR_ARG
    assert L.srt_nearest_points_multi_device(ds.h, 4, 0x1000, None, None, 4, 0, None, C.byref(with_n)) == abi.SRT_ERR_ARG
    assert L.srt_nearest_points_multi(ds.h, 0, None, None, None, 4, 0, C.byref(with_n), None) == abi.SRT_ERR_ARG
    assert (tri == -7).all() and (nw == 77).all()
    with pytest.raises(srt.SrtError):
        ds.nearest_points_multi(pts, 4, want=("n_within", "tri"))
    # (the same struct is fine in the closest form: n_within is every triangle whose dist2 is not a NaN)
    assert L.srt_closest_points_multi(ds.h, 4, p, None, None, 16, 0, C.byref(with_n), None) == abi.SRT_OK
    assert np.array_equal(nw, pm.closest_points_multi(pe.scene(), pts, 16)["n_within"]) and (tri[:, 0] >= 0).all()
    o = ds.closest_points_multi(np.zeros((0, 3), F), 3)
    assert o["tri"].shape == (0, 3) and o["point"].shape == (0, 3, 3) and o["n_within"].shape == (0,) and o["stats"]["primary_rays"] == 0
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "points_multi_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"points multi {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_points():
    """Device pointers from torch tensors: a second stream beside a pending render, the yardstick's bits, outputs NULL, float-aligned
    pointers, masks, a shared handle (own process: torch initialises HIP first)."""
    run_case("device")


def test_after_refit_device():
    """srt_scene_refit_device from a torch tensor, then both forms on the same stream: the yardstick on the moved flat scene."""
    run_case("refit")


def test_captured_into_a_hip_graph():
    """Both _device forms captured once into a hipGraph and replayed twice: the same bits."""
    run_case("graph")
