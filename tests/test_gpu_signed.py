"""GPU (-m gpu): srt_signed_points and its _device form (include/srt_signed.h), every output bit for bit against tests/sign_ref.py -- the
four sign outputs, the five point outputs, the sign rays' work counts exactly, the nearest phase's between the mandatory set's
(tests/nearest_ref.py) and srt_closest_points' -- on the scenes of tests/test_gpu_points.py at 1, 63, 64, 65 and 257 points, with 1, 2, 3
(the default table) and 16 directions, in both vote modes; the lattice batch on a cube that is one leaf of 12 triangles; against
srt_nearest_points and srt_trace_rays_multi on the same handle; masks, a pose, the radii that walk nothing, points that are NaN, inf or
1e19, containment only, every output alone, the argument errors; the _device form in a process of its own.
ground_bunny's bunny is NOT closed (223 edges without a partner): it is here for bit parity, not for a true sign (tests/test_sign_ref.py)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import nearest_ref as nr
import point_edges as pe
import point_ref as pr
import pose_ref
import sign_ref as sg
import test_gpu_nearest as tn
import test_gpu_points as tp
import tree_shapes as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SCENES = ("cube", "sliced", "comb256", "roots33", "shuffled", "ground_bunny")
COUNTS = tp.COUNTS
N = tp.N
N_DIRS = (1, 2, 3, 16)
ALL_KEYS = sg.SIGN_KEYS + pr.SAME_KEYS
EDGE_BATCHES = ("wild points, no radius", "wild points, radius 5", "degenerate and non-finite triangles, no radius", "radii mixed", "radius -1", "radius NaN")


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def table16():
    """16 directions of any length between 0.3 and 3, none along an axis; the tables of 1 and 2 directions are its first rows."""
    rng = np.random.default_rng(23)
    d = rng.normal(size=(16, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.3, 3.0, (16, 1))).astype(F)


DIRS16 = table16()


def dirs_of(nd):
    return None if nd == 3 else DIRS16[:nd]


class Reference:
    """Made once and never changed, each part when it is first asked for: the scene and points of tests/test_gpu_points.py; rows(3) and
    rows(16), the yardstick's rows under the default table and under the 16 directions (ground_bunny: the 16 for its first 65 points --
    the yardstick's node pass is rays x nodes); the floor of the nearest phase's counts per point."""

    def __init__(self, name):
        self.name = name
        self.flat, self.pts, self.rad, self.near = tp.case(name)
        self.most = {3: N, 16: 65 if name == "ground_bunny" else N}

    @functools.lru_cache(maxsize=None)
    def rows(self, table):
        from oracle import pyoracle
        w = sg.signs(pyoracle, self.flat, self.pts[:self.most[table]], None if table == 3 else DIRS16)
        w.update({k: self.near[k][:self.most[table]] for k in pr.SAME_KEYS})
        return w

    @functools.lru_cache(maxsize=None)
    def floor(self):
        return nr.mandatory(self.flat, self.pts, self.near["dist2"], self.rad)


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(name)


def wanted(r, n, nd, parity):
    return sg.first(r.rows(3 if nd == 3 else 16), n, nd, parity)


def same_counts(stats, want, n, nd, what, near=None, floor=None):
    """The sign rays' counts exactly; the nearest phase's between the mandatory set's and srt_closest_points'."""
    got = (stats["primary_rays"], stats["shadow_rays"], stats["node_tests_shadow"], stats["tri_tests_shadow"])
    assert got == (n, n * nd, want["node_tests_shadow"], want["tri_tests_shadow"]), (what, got, want["node_tests_shadow"], want["tri_tests_shadow"])
    if near is not None:
        assert stats["hit_rays"] == near["hits"], (what, stats["hit_rays"], near["hits"])
        assert int(floor[0][:n].sum()) <= stats["node_tests_primary"] <= near["node_tests"], (what, stats, near["node_tests"])
        assert int(floor[1][:n].sum()) <= stats["tri_tests_primary"] <= near["tri_tests"], (what, stats, near["tri_tests"])


@pytest.mark.parametrize("name", SCENES)
def test_against_the_yardstick(srt, name):
    r = reference(name)
    pts, rad = r.pts, r.rad
    ds = srt.DeviceScene(r.flat)
    for nd in N_DIRS:
        for n in COUNTS:
            if n > r.most[3 if nd == 3 else 16]:
                continue
            near = pr.first(r.near, n)
            for parity in (False, True):
                what = f"{name}, {n} points, {nd} directions, parity {parity}"
                want = wanted(r, n, nd, parity)
                got = ds.signed_points(pts[:n], radius=rad[:n], dirs=dirs_of(nd), parity=parity, count=True)
                assert set(got) == set(ALL_KEYS) | {"stats"}
                sg.same(got, want, what)
                same_counts(got["stats"], want, n, nd, what, near, r.floor())
            plain = ds.signed_points(pts[:n], radius=rad[:n], dirs=dirs_of(nd))
            sg.same(plain, wanted(r, n, nd, False), f"{name}, {n} points, {nd} directions, no counting")
            st = plain["stats"]
            assert (st["hit_rays"], st["shadow_rays"], st["node_tests_primary"], st["node_tests_shadow"], st["tri_tests_shadow"]) == (near["hits"], n * nd, 0, 0, 0)
    w = r.rows(3)
    print(name, "points", N, "inside", int(w["inside"].sum()), "sign rays' node tests", int(w["node_tests_each"].sum()), "triangle tests", int(w["tri_tests_each"].sum()))
    ds.close()


@pytest.mark.parametrize("parity", [False, True])
def test_the_lattice_batch(srt, oracle, parity):
    """Dyadic points and directions along axes, face diagonals and body diagonals on a cube that is one leaf of 12 triangles: rays through
    shared edges, the faces' split diagonals and vertices, points on a face, an edge and a vertex (t = 0), the origin; the leaf goes in slices."""
    flat = sg.lattice_scene()
    pts, dirs = sg.lattice_batch()
    want = sg.signed_points(oracle, flat, pts, dirs=dirs, parity=parity)
    ds = srt.DeviceScene(flat)
    got = ds.signed_points(pts, dirs=dirs, parity=parity, count=True)
    sg.same(got, want, "lattice")
    same_counts(got["stats"], sg.first(want, len(pts)), len(pts), 16, "lattice")
    assert got["stats"]["hit_rays"] == len(pts) and (got["sdist"][np.abs(pts).max(1) == 1] == 0).all()
    ds.close()


@pytest.mark.parametrize("name", ["cube", "sliced", "ground_bunny"])
def test_against_the_shipped_calls(srt, name):
    """On the same handle: the point outputs are srt_nearest_points' bits; unmasked crossings are srt_trace_rays_multi's n_hits on the
    n x n_dirs rays written out on the host."""
    r = reference(name)
    pts, rad = r.pts, r.rad
    ds = srt.DeviceScene(r.flat)
    for radius in (rad, None):
        got = ds.signed_points(pts, radius=radius)
        pr.same(got, ds.nearest_points(pts, radius=radius), name + ": against srt_nearest_points")
        sg.same({k: got[k] for k in ("sdist",)}, dict(sdist=sg.sdist_of(got["inside"], got["dist2"])), name + ": sdist of the call's own dist2")
    for nd in (3, 16):
        d = sg.DEFAULT_DIRS if nd == 3 else DIRS16
        got = ds.signed_points(pts, dirs=dirs_of(nd), want=("crossings", "winding"))
        hits = ds.trace_rays_multi(sg.sign_rays(pts, d), 1, want=("n_hits",))["n_hits"]
        assert np.array_equal(got["crossings"], hits.reshape(N, nd)), (name, nd)
        assert ((got["crossings"].astype(np.int64) - got["winding"]) % 2 == 0).all() and (np.abs(got["winding"]) <= got["crossings"]).all()
    ds.close()


@pytest.mark.parametrize("name,hide", [("sliced", 1), ("roots33", 32)])
def test_masks(srt, oracle, name, hide):
    """A hidden object contributes no crossing: the reduced scene's result, and the yardstick's masks point by point."""
    objects = {"sliced": ts.sliced_objects, "roots33": lambda: ts.roots_objects(33)}[name]()
    full, less, ids = tp.reduced(objects, hide)
    r = reference(name)
    pts, rad = r.pts, r.rad
    ds = srt.DeviceScene(full)
    got = ds.signed_points(pts, radius=rad, point_mask=np.full(N, 0xFFFFFFFF, np.uint32), count=True)
    sg.same(got, wanted(r, N, 3, False), name + ", masks of all ones")
    same_counts(got["stats"], wanted(r, N, 3, False), N, 3, name + ", masks of all ones")
    om = np.where(np.arange(full.n_objects) == hide, 2, 1 | (4 << (np.arange(full.n_objects) % 8))).astype(np.uint32)
    ds.set_object_masks(om)
    small = sg.signed_points(oracle, less, pts, rad)
    w = dict(small, tri=np.where(small["tri"] >= 0, ids[np.maximum(small["tri"], 0)], -1).astype(np.int32))
    got = ds.signed_points(pts, radius=rad, point_mask=np.full(N, 1, np.uint32), count=True)
    sg.same(got, w, f"{name}, object {hide} hidden")
    same_counts(got["stats"], sg.first(w, N), N, 3, f"{name}, object {hide} hidden")
    for parity in (False, True):
        pm = np.resize(np.uint32([0xFFFFFFFF, 1, 2, 0, 4, 8]), N)
        w = sg.signed_points(oracle, full, pts, rad, point_mask=pm, obj_mask=om, dirs=DIRS16[:5], parity=parity)
        got = ds.signed_points(pts, radius=rad, point_mask=pm, dirs=DIRS16[:5], parity=parity, count=True)
        sg.same(got, w, name + ", a mask per point")
        same_counts(got["stats"], sg.first(w, N), N, 5, name + ", a mask per point")
        assert (got["crossings"][pm == 0] == 0).all() and (got["inside"][pm == 0] == 0).all()
    sg.same(ds.signed_points(pts, radius=rad), wanted(r, N, 3, False), name + ", unmasked beside a table")
    ds.close()


@pytest.mark.parametrize("name", tn.POSED)
def test_after_pose(srt, oracle, name):
    r = reference(name)
    flat, pts, rad = r.flat, r.pts, r.rad
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = tn.pose_mats(flat)
    ds.pose(mats)
    moved = pose_ref.pose_flat(flat, mats)
    want = sg.signed_points(oracle, moved, pts, rad)
    got = ds.signed_points(pts, radius=rad, count=True)
    sg.same(got, want, name + ", posed")
    same_counts(got["stats"], sg.first(want, N), N, 3, name + ", posed")
    assert not np.array_equal(want["crossings"], r.rows(3)["crossings"])
    ds.close()


@pytest.mark.parametrize("name", ["cube", "sliced"])
def test_the_sign_does_not_depend_on_the_radius(srt, name):
    """Radii None, finite, -1 and NaN: the same winding, crossings and inside; -1 and NaN walk nothing in the nearest phase, so sdist is
    -inf or +inf.  Containment only runs no nearest phase and gives the same `inside`; every output alone gives its own bits."""
    r = reference(name)
    pts, rad = r.pts, r.rad
    want = wanted(r, N, 3, False)
    ds = srt.DeviceScene(r.flat)
    assert 0 < want["inside"].sum() < N or name != "cube"
    for radius in (None, rad, -1.0, np.nan):
        got = ds.signed_points(pts, radius=radius, count=True)
        what = f"{name}, radius {radius if not isinstance(radius, np.ndarray) else 'array'}"
        sg.same({k: got[k] for k in ("inside", "winding", "crossings")}, want, what)
        near = pr.closest_points(r.flat, pts, radius)
        pr.same(got, near, what)
        sg.same(dict(sdist=got["sdist"]), dict(sdist=sg.sdist_of(want["inside"], near["dist2"])), what)
        same_counts(got["stats"], want, N, 3, what)
        if isinstance(radius, float):
            assert np.isinf(got["sdist"]).all() and np.array_equal(got["sdist"] < 0, want["inside"] != 0) and (got["tri"] == -1).all()
            assert (got["stats"]["hit_rays"], got["stats"]["node_tests_primary"], got["stats"]["tri_tests_primary"]) == (0, 0, 0)
    only = ds.signed_points(pts, radius=rad, want=("inside",), count=True)
    assert set(only) == {"inside", "stats"} and np.array_equal(only["inside"], want["inside"])
    same_counts(only["stats"], want, N, 3, name + ", containment only")
    assert (only["stats"]["hit_rays"], only["stats"]["node_tests_primary"], only["stats"]["tri_tests_primary"]) == (0, 0, 0)
    for k in ALL_KEYS:
        got = ds.signed_points(pts, radius=rad, want=(k,))
        assert set(got) == {k, "stats"}
        sg.same(got, want, f"{name}, {k} alone")
    # no sign output wanted: the call is srt_nearest_points
    got = ds.signed_points(pts, radius=rad, want=pr.SAME_KEYS, count=True)
    pr.same(got, r.near, name + ", no sign output")
    assert got["stats"]["shadow_rays"] == 0 and got["stats"]["node_tests_shadow"] == 0 and got["stats"]["hit_rays"] == r.near["hits"]
    ds.close()


@pytest.mark.parametrize("batch", EDGE_BATCHES)
def test_edges(srt, oracle, batch):
    """tests/point_edges.py: points that are NaN, inf or 1e19, degenerate and non-finite triangles, an empty leaf, radii that walk nothing."""
    flat = pe.scene()
    p, rad = pe.batches()[batch]
    ds = srt.DeviceScene(flat)
    for dirs, parity in ((None, False), (DIRS16, True)):
        want = sg.signed_points(oracle, flat, p, rad, dirs=dirs, parity=parity)
        got = ds.signed_points(p, radius=rad, dirs=dirs, parity=parity, count=True)
        sg.same(got, want, batch)
        same_counts(got["stats"], sg.first(want, len(p)), len(p), 3 if dirs is None else 16, batch)
    ds.close()


def test_argument_errors(srt):
    """Every error comes back before anything is touched: no output buffer changes."""
    from simple_raytracer_amd import abi
    L = srt.load()
    ds = srt.DeviceScene(pe.scene())
    f32p = C.POINTER(C.c_float)
    pts = np.zeros((4, 3), F)
    pp = pts.ctypes.data_as(f32p)
    tri, inside, wind = np.full(4, -7, np.int32), np.full(4, 9, np.uint8), np.full((4, 16), -7, np.int32)
    po = abi.PointOut(tri.ctypes.data, None, None, None, None)
    so = abi.SignOut(None, inside.ctypes.data, wind.ctypes.data, None)
    dirs = np.ones((17, 3), F)
    host, dev = L.srt_signed_points, L.srt_signed_points_device
    sign = lambda d, n, flags=0: C.byref(abi.Sign(None if d is None else d.ctypes.data, n, flags))
    assert host(ds.h, 0, None, None, None, None, 0, C.byref(po), C.byref(so), None) == abi.SRT_OK
    assert dev(ds.h, 0, None, None, None, None, 0, None, C.byref(po), C.byref(so)) == abi.SRT_OK
    assert dev(ds.h, 4, 0x1000, None, None, None, 0, None, C.byref(abi.PointOut()), C.byref(abi.SignOut())) == abi.SRT_OK      # nothing wanted: nothing launched
    assert dev(ds.h, 4, 0x1000, None, None, None, 0, None, None, C.byref(abi.SignOut())) == abi.SRT_OK
    bad = [
        (None, pp, None, 0, C.byref(po), C.byref(so)),                          # no handle
        (ds.h, None, None, 0, C.byref(po), C.byref(so)),                        # no points
        (ds.h, pp, None, 0, None, None),                                        # neither out nor sout
        (ds.h, pp, sign(dirs, 17), 0, C.byref(po), C.byref(so)),                # n_dirs > 16
        (ds.h, pp, sign(dirs, 0), 0, C.byref(po), C.byref(so)),                 # dirs without a count
        (ds.h, pp, sign(None, 3), 0, C.byref(po), C.byref(so)),                 # a count without dirs
        (ds.h, pp, sign(dirs, 3, 2), 0, C.byref(po), C.byref(so)),              # an unknown bit in sign->flags
        (ds.h, pp, sign(dirs, 3, abi.SIGN_PARITY | 4), 0, None, C.byref(so)),
    ]
    bad += [(ds.h, pp, None, flags, C.byref(po), C.byref(so)) for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT, 1 << 9)]
    for k, (h, p, sgn, flags, out, sout) in enumerate(bad):
        assert host(h, 4, p, None, None, sgn, flags, out, sout, None) == abi.SRT_ERR_ARG, k
        assert dev(h, 4, p, None, None, sgn, flags, None, out, sout) == abi.SRT_ERR_ARG, k
    assert (tri == -7).all() and (inside == 9).all() and (wind == -7).all()
    # the largest table is taken; the outputs are then written
    assert host(ds.h, 4, pp, None, None, sign(dirs, 16), 0, C.byref(po), C.byref(so), None) == abi.SRT_OK
    assert (inside <= 1).all() and (wind != -7).all()
    o = ds.signed_points(np.zeros((0, 3), F))
    assert o["inside"].shape == (0,) and o["winding"].shape == (0, 3) and o["stats"]["primary_rays"] == 0
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "signed_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"signed {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_point():
    """Device pointers from torch tensors: a second stream beside a pending render, the yardstick's bits, float-aligned pointers, a caller's
    table on the device, masks, a shared handle (own process: torch initialises HIP first)."""
    run_case("device")


def test_after_refit_device():
    """srt_scene_refit_device from a torch tensor, then the call on the same stream: the yardstick on the moved scene."""
    run_case("refit")


def test_captured_into_a_hip_graph():
    """srt_signed_points_device captured once into a hipGraph and replayed twice: the same bits."""
    run_case("graph")
