"""GPU (-m gpu): srt_closest_points and its _device form on whole scenes -- the golden cube and ground_bunny, and the trees of
tests/tree_shapes.py the host builder never makes (a comb of height 256, leaves of 31 triangles taken in slices, 33 and 300 leaf-roots,
shuffled nodes, boxes that do not nest) -- every output bit for bit against tests/point_ref.py, the work counts included, at 1, 63, 64,
65 and 257 points: a partial wave, a full one, one lane of the next, a second workgroup, the queue's full flushes and its tail."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import point_ref as pr
import pose_ref
import tree_shapes as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SCENES = ("cube", "ground_bunny", "comb256", "sliced", "roots33", "roots300", "shuffled", "loose")
COUNTS = (1, 63, 64, 65, 257)
N = max(COUNTS)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def flat_of(name):
    return gu.GoldenScene(name).flat if name in ("cube", "ground_bunny") else ts.family(name)


def points_for(flat, n, seed):
    """n points: half of them a little off a vertex of the scene, half anywhere in and around its bounding box."""
    rng = np.random.default_rng(seed)
    P = np.ascontiguousarray(flat.tri_points, F)[..., :3].reshape(-1, 3)
    mn, mx = P.min(0), P.max(0)
    ext = float(np.linalg.norm(mx - mn))
    near = P[rng.integers(0, len(P), n)] + rng.normal(0.0, 0.01 * ext, (n, 3))
    box = mn + (mx - mn) * rng.uniform(-0.3, 1.3, (n, 3))
    return np.where((np.arange(n) % 2 == 0)[:, None], near, box).astype(F), ext


def radii_for(ext, n, seed, unbounded):
    """n radii between a 300th and a third of the scene's extent; `unbounded` of them +inf, two that walk nothing."""
    rng = np.random.default_rng(seed + 100)
    r = (ext * 10.0 ** rng.uniform(-2.5, -0.5, n)).astype(F)
    r[rng.permutation(n)[:unbounded]] = np.inf
    r[5], r[70] = -1.0, np.nan
    return r


@functools.lru_cache(maxsize=None)
def case(name):
    """(flat, points, radii, the yardstick's result) of a scene, made once and never changed.  ground_bunny's 69,463 triangles get 8
    unbounded points, the small scenes 64."""
    flat = flat_of(name)
    pts, ext = points_for(flat, N, 17)
    rad = radii_for(ext, N, 17, 8 if name == "ground_bunny" else 64)
    return flat, pts, rad, pr.closest_points(flat, pts, rad)


@pytest.mark.parametrize("name", SCENES)
def test_against_the_yardstick(srt, name):
    flat, pts, rad, want = case(name)
    assert 0.15 * N < want["hits"] < N, want["hits"]
    ds = srt.DeviceScene(flat)
    for n in COUNTS:
        w = pr.first(want, n)
        got = ds.closest_points(pts[:n], radius=rad[:n], count=True)
        pr.same(got, w, f"{name}, {n} points")
        pr.same_counts(got["stats"], w, n, f"{name}, {n} points")
        plain = ds.closest_points(pts[:n], radius=rad[:n])
        pr.same(plain, w, f"{name}, {n} points, no counting")
        assert plain["stats"]["hit_rays"] == w["hits"] and plain["stats"]["node_tests_primary"] == 0
    print(name, "points", N, "found", want["hits"], "node tests", want["node_tests"], "triangle tests", want["tri_tests"])
    # any output may be NULL; another order of the points gives the same rows in that order
    only = ds.closest_points(pts, radius=rad, want=("vw",))
    assert set(only) == {"vw", "stats"} and np.array_equal(only["vw"].view(np.uint32), want["vw"].view(np.uint32))
    assert ds.closest_points(pts, radius=rad, want=())["stats"]["hit_rays"] == want["hits"]
    perm = np.random.default_rng(3).permutation(N)
    pr.same(ds.closest_points(pts[perm], radius=rad[perm]), {k: want[k][perm] for k in pr.SAME_KEYS}, name + ", permuted")
    ds.close()


@pytest.mark.parametrize("name", ["cube", "sliced", "roots33", "comb256", "loose"])
def test_without_a_radius(srt, name):
    """radius NULL is +inf for every point: every node passes, every triangle is a candidate, and the winner is brute force."""
    flat, pts, _, _ = case(name)
    want = pr.closest_points(flat, pts)
    assert want["node_tests"] == N * flat.n_nodes and want["tri_tests"] == N * flat.n_tris
    tri, d2 = pr.brute_force(flat, pts[:65])
    assert np.array_equal(want["tri"][:65], tri) and np.array_equal(want["dist2"][:65].view(np.uint32), d2.view(np.uint32))
    ds = srt.DeviceScene(flat)
    got = ds.closest_points(pts, count=True)
    pr.same(got, want, name)
    pr.same_counts(got["stats"], want, N, name)
    pr.same(ds.closest_points(pts, radius=np.inf), want, name + ", one radius for all")
    ds.close()


def reduced(objects, hide):
    """The flat scene without object `hide`, and the map from its triangle ids to the full scene's."""
    full, less = ts.flat_scene(objects), ts.flat_scene([o for k, o in enumerate(objects) if k != hide])
    ids = np.flatnonzero(full.tri_obj != hide)
    assert ids.size == less.n_tris and np.array_equal(full.tri_points[ids].view(np.uint32), less.tri_points.view(np.uint32))
    return full, less, ids


@pytest.mark.parametrize("name,hide", [("sliced", 1), ("sliced", 0), ("roots33", 32), ("comb256", 0)])
def test_masks(srt, name, hide):
    objects = {"sliced": ts.sliced_objects, "roots33": lambda: ts.roots_objects(33), "comb256": lambda: ts.comb_objects(256)}[name]()
    full, less, ids = reduced(objects, hide)
    _, pts, rad, want = case(name)
    ds = srt.DeviceScene(full)
    # all ones, by a table never set, a table of ones and masks of ones: the unmasked call's bits and counts
    for table in (None, np.full(full.n_objects, 0xFFFFFFFF, np.uint32)):
        if table is not None:
            ds.set_object_masks(table)
        for pm in (True, np.full(N, 0xFFFFFFFF, np.uint32)):
            got = ds.closest_points(pts, radius=rad, point_mask=pm, count=True)
            pr.same(got, want, f"{name}, all ones")
            pr.same_counts(got["stats"], want, N, f"{name}, all ones")
    # object `hide` hidden from every point: the reduced scene's result, its ids renumbered
    om = np.where(np.arange(full.n_objects) == hide, 2, 1 | (4 << (np.arange(full.n_objects) % 8))).astype(np.uint32)
    ds.set_object_masks(om)
    small = pr.closest_points(less, pts, rad)
    w = dict(small, tri=np.where(small["tri"] >= 0, ids[np.maximum(small["tri"], 0)], -1).astype(np.int32))
    masked = pr.closest_points(full, pts, rad, point_mask=np.full(N, 1, np.uint32), obj_mask=om)
    pr.same(masked, w, "the yardstick's masks against the reduced scene")
    assert (masked["node_tests"], masked["tri_tests"]) == (small["node_tests"], small["tri_tests"])
    got = ds.closest_points(pts, radius=rad, point_mask=np.full(N, 1, np.uint32), count=True)
    pr.same(got, w, f"{name}, object {hide} hidden")
    pr.same_counts(got["stats"], w, N, f"{name}, object {hide} hidden")
    assert not np.isin(got["tri"], np.flatnonzero(full.tri_obj == hide)).any()
    # a mask per point: some see everything, some all but `hide`, some only `hide`, some nothing
    pm = np.resize(np.uint32([0xFFFFFFFF, 1, 2, 0, 4, 8]), N)
    w = pr.closest_points(full, pts, rad, point_mask=pm, obj_mask=om)
    got = ds.closest_points(pts, radius=rad, point_mask=pm, count=True)
    pr.same(got, w, f"{name}, a mask per point")
    pr.same_counts(got["stats"], w, N, f"{name}, a mask per point")
    assert (got["tri"][pm == 0] == -1).all()
    # the unmasked call ignores the table
    pr.same(ds.closest_points(pts, radius=rad), want, f"{name}, unmasked beside a table")
    ds.close()


def turn(k, n):
    """Object k's matrix (column-major 4 x 4): a turn about z by 20 + 10 k degrees, a stretch of y, a shift."""
    a = np.deg2rad(20.0 + 10.0 * k)
    m = np.eye(4)
    m[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.diag([1.0, 1.1, 1.0])
    m[:3, 3] = (3.0 * k - 4.0, 2.0, -5.0 + k)
    return m.T.reshape(16).astype(F)


@pytest.mark.parametrize("name", ["sliced", "roots33", "ground_bunny"])
def test_after_pose(srt, name):
    """srt_scene_pose moves the records the query reads: the yardstick on pose_ref's flat scene."""
    flat, pts, rad, before = case(name)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = np.stack([turn(k, flat.n_objects) for k in range(flat.n_objects)])
    ds.pose(mats)                                               # asynchronous on the scene's own stream: the query is ordered behind it
    got = ds.closest_points(pts, radius=rad, count=True)
    moved = pose_ref.pose_flat(flat, mats)
    want = pr.closest_points(moved, pts, rad)
    assert np.array_equal(ds.records()["tris"][:, :9], pr.records_of(moved)[:, :9].view(np.uint32))
    pr.same(got, want, name + ", posed")
    pr.same_counts(got["stats"], want, N, name + ", posed")
    assert not np.array_equal(want["tri"], before["tri"]) or not np.array_equal(want["dist2"], before["dist2"])
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "points_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"points {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_point():
    """Device pointers from torch tensors: a second stream beside a pending render, the host form's bits, float-aligned pointers, a
    shared handle, masks, and renders before and after that are untouched (own process: torch initialises HIP first)."""
    run_case("device")


def test_after_refit_device():
    """srt_scene_refit_device from a torch tensor, then the query on the same stream: the yardstick on the moved flat scene."""
    run_case("refit")


def test_captured_into_a_hip_graph():
    """srt_closest_points_device captured once into a hipGraph and replayed twice: the same bits."""
    run_case("graph")
