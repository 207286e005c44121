"""GPU (-m gpu): srt_closest_points at its edges -- the batches of tests/point_edges.py on its scene, every output bit for bit against the
float32 yardstick tests/point_ref.py (region and vw as bits, dist2 as bits, the point, the triangle), and both work counts."""
import numpy as np
import pytest

import point_edges as pe
import point_ref as pr

pytestmark = pytest.mark.gpu
NAMES = ("lattice, no radius", "radius = distance (closed)", "radius one ulp below the distance", "radius 0 on the surface", "radius 0 off the surface",
         "radius -0", "radius -1", "radius NaN", "radius +inf", "radius -inf", "radius tiny", "radius huge", "radii mixed", "wild points, no radius",
         "wild points, radius 1e19", "wild points, radius 5", "degenerate and non-finite triangles, no radius",
         "degenerate and non-finite triangles, radius 3", "all")


@pytest.fixture(scope="module")
def ds():
    from simple_raytracer_amd import lib
    lib.load()
    d = lib.DeviceScene(pe.scene())
    yield d
    d.close()


@pytest.fixture(scope="module")
def batches():
    b = pe.batches()
    assert tuple(b) == NAMES
    return b


def test_the_records_are_the_yardsticks(ds):
    """The yardstick reads tests/refit_edges.derive_ref's records; the device's own are the same words (P1, e1, e2), NaN and inf included."""
    got = ds.records()["tris"][:, :9]
    assert np.array_equal(got, pr.records_of(pe.scene())[:, :9].view(np.uint32))


@pytest.mark.parametrize("name", NAMES)
def test_edges(ds, batches, name):
    flat = pe.scene()
    p, r = batches[name]
    want = pr.closest_points(flat, p, r)
    got = ds.closest_points(p, radius=r, count=True)
    pr.same(got, want, name)
    st = got["stats"]
    print(name, "points", len(p), "found", want["hits"], "node tests", st["node_tests_primary"], want["node_tests"], "triangle tests", st["tri_tests_primary"],
          want["tri_tests"])
    assert (st["primary_rays"], st["hit_rays"], st["node_tests_primary"], st["tri_tests_primary"]) == (len(p), want["hits"], want["node_tests"], want["tri_tests"]), name
    plain = ds.closest_points(p, radius=r)
    pr.same(plain, want, name + ", no counting")
    assert plain["stats"]["hit_rays"] == want["hits"] and plain["stats"]["node_tests_primary"] == 0 and plain["stats"]["tri_tests_primary"] == 0


def test_what_the_edges_are(ds, batches):
    """The cases the batches are there for, read off the device's answers."""
    def q(name):
        return ds.closest_points(*batches[name][:1], radius=batches[name][1])
    closed, below = q("radius = distance (closed)"), q("radius one ulp below the distance")
    assert (closed["tri"] == 0).all() and np.array_equal(closed["dist2"], np.float32([0.25, 1.0, 4.0, 9.0])) and (closed["region"] == 0).all()
    assert (below["tri"] == -1).all() and np.isinf(below["dist2"]).all() and not below["point"].any() and not below["vw"].any()
    on = q("radius 0 on the surface")
    assert (on["tri"] >= 0).all() and not on["dist2"].any() and not np.signbit(on["dist2"]).any()
    assert on["region"].tolist() == [4, 5, 6, 1, 2, 3, 0, 4, 3]
    # identical triangles in two objects: the lowest id wins, everywhere
    flat = pe.scene()
    lat = q("lattice, no radius")
    assert (lat["tri"] >= 0).all() and not np.isin(flat.tri_obj[lat["tri"]], (1,)).any()
    for name in ("radius -1", "radius NaN", "radius -inf"):
        o = q(name)
        assert (o["tri"] == -1).all() and np.isinf(o["dist2"]).all() and not o["region"].any()
    wild = q("wild points, no radius")
    assert (wild["tri"][:3] == -1).all(), "a NaN point finds nothing"
    assert (np.isinf(wild["dist2"]) & (wild["tri"] >= 0)).any(), "dist2 overflows to +inf and still qualifies under r = +inf"
    # the results do not depend on the order of the points
    p, r = batches["all"]
    perm = np.random.default_rng(2).permutation(len(p))
    a, b = ds.closest_points(p, radius=r), ds.closest_points(p[perm], radius=r[perm])
    pr.same(b, {k: a[k][perm] for k in pr.SAME_KEYS}, "permuted")


def test_argument_errors(ds):
    import ctypes as C
    from simple_raytracer_amd import abi, lib
    L = lib.load()
    f32p = C.POINTER(C.c_float)
    pts = np.zeros((4, 3), np.float32)
    tri = np.full(4, -7, np.int32)
    po = abi.PointOut(tri.ctypes.data, None, None, None, None)
    ok = lambda *a: L.srt_closest_points(*a)
    assert ok(ds.h, 0, None, None, None, 0, C.byref(po), None) == abi.SRT_OK
    assert ok(None, 4, pts.ctypes.data_as(f32p), None, None, 0, C.byref(po), None) == abi.SRT_ERR_ARG
    assert ok(ds.h, 4, None, None, None, 0, C.byref(po), None) == abi.SRT_ERR_ARG
    assert ok(ds.h, 4, pts.ctypes.data_as(f32p), None, None, 0, None, None) == abi.SRT_ERR_ARG
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT, 1 << 9):
        assert ok(ds.h, 4, pts.ctypes.data_as(f32p), None, None, flags, C.byref(po), None) == abi.SRT_ERR_ARG, flags
        assert L.srt_closest_points_device(ds.h, 4, None, None, None, flags, None, C.byref(po)) == abi.SRT_ERR_ARG
    assert L.srt_closest_points_device(ds.h, 4, None, None, None, 0, None, C.byref(po)) == abi.SRT_ERR_ARG
    assert L.srt_closest_points_device(ds.h, 0, None, None, None, 0, None, C.byref(po)) == abi.SRT_OK
    assert L.srt_closest_points_device(ds.h, 4, None, None, None, 0, None, None) == abi.SRT_ERR_ARG
    assert (tri == -7).all()
    o = ds.closest_points(np.zeros((0, 3), np.float32))
    assert o["tri"].shape == (0,) and o["point"].shape == (0, 3) and o["stats"]["primary_rays"] == 0
