"""CPU: the yardstick of the ray queries with a t interval (tests/ray_range_ref.py) pinned against the oracle as it stands -- at
(0, +inf) it is ray_query_ref's closest hit, ray by ray and bit for bit, and ray_query_ref's two-frame shadow read-out -- and the
batches it is used on have what the GPU cases need: rays with a second candidate behind the first."""
import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import ray_range_ref as rr
from simple_raytracer_amd import build, lib

# scene -> (rays of unrelated_rays, triangles, hits, rays with two or more finite candidates, NaN candidates)
PINNED = {"cubes4_a40": (400, 48, 282, 253, 0), "ground_bunny": (200, 69463, 143, 138, 0)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_range(n):
    return np.tile(np.array([0.0, np.inf], np.float32), (n, 1))


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import host
    build.build_host()
    return host.Transformation


@pytest.mark.parametrize("name", sorted(PINNED))
def test_open_interval_is_the_oracle(oracle, name):
    """Range (0, +inf), and no range at all, give oracle_trace's ids and t bits on unrelated rays; the batch's counts are pinned, and
    at least half of the hit rays have a second finite candidate (so 't_min = next float after the first hit' has something to find)."""
    n, n_tris, hits, multi, nans = PINNED[name]
    g = gu.GoldenScene(name)
    assert g.flat.n_tris == n_tris
    rays = rq.unrelated_rays(g.flat, n)
    c = rr.candidates(oracle, g.flat, rays)
    want_hit, want_t = rq.oracle_trace(oracle, g.flat, rays)
    for tr in (open_range(n), None):
        hit, t = rr.closest(c, tr)
        assert np.array_equal(hit, want_hit) and np.array_equal(bits(t), bits(want_t)), name
    got = (int((want_hit >= 0).sum()), int((c.finite() >= 2).sum()), int(c.nan().sum()))
    print(name, "hits, rays with >= 2 finite candidates, NaN candidates:", got)
    assert got == (hits, multi, nans)
    assert got[1] * 2 >= got[0]
    assert ((c.finite() >= 1) == (want_hit >= 0)).all()


def test_open_interval_is_the_shadow_readout(oracle, T):
    """cubes4_a40, the occlusion case of ray_query_ref: the shadow ray of every hit pixel, the hit object skipped, range (0, +inf) and
    no range: the two-frame read-out."""
    name = "cubes4_a40"
    g = gu.GoldenScene(name)
    W, H, M, focal, light = rq.FRAME_W, rq.FRAME_H, rq.rigid(T, 4.0), rq.FOCAL[name], rq.SHADOW_LIGHT[name]
    hit, t, shadowed, usable = rq.shadow_readout(oracle, g.flat, W, H, M, focal, light)
    sel = hit >= 0
    assert np.array_equal(usable, sel)
    sray = rq.shadow_rays(rq.frame_rays(W, H, M, focal)[sel], t[sel], light)
    skip = g.flat.tri_obj[hit[sel]].astype(np.int32)
    c = rr.candidates(oracle, g.flat, sray)
    for tr in (open_range(sray.shape[0]), None):
        assert np.array_equal(rr.occluded(c, g.flat, tr, skip).astype(bool), shadowed[sel])
    assert 0.01 <= shadowed[sel].mean() <= 0.99


def test_the_definition_on_a_hand_made_set():
    """closed interval, NaN bounds, NaN t, -inf, +inf, the two zeros, lowest id among equal t, t_min > t_max."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    t = np.array([2.0, 1.0, 1.0, -inf, inf, nan, -0.0, 0.0], np.float32)

    def one(tr, t=t):
        c = rr.Candidates(1, np.zeros(t.size, np.int64), np.arange(t.size, dtype=np.int64) + 10, t)
        (hit,), (tt,) = rr.closest(c, None if tr is None else np.array([tr], np.float32))
        return int(hit), float(tt), bool(np.signbit(tt))
    assert one(None) == (16, 0.0, True) == one((0.0, inf)) == one((-inf, inf)) == one((nan, nan))       # -0 at id 16 ties with +0 at id 17
    assert one((0.5, inf)) == (11, 1.0, False)                    # ids 11 and 12 tie: the lowest
    assert one((1.0, 1.0)) == (11, 1.0, False)                    # closed
    assert one((np.nextafter(np.float32(1.0), inf), inf)) == (10, 2.0, False)
    assert one((np.nextafter(np.float32(1.0), inf), np.nextafter(np.float32(2.0), -inf)))[0] == -1
    assert one((3.0, inf))[:2] == (-1, float(inf))                # +inf is in range and is no hit
    assert one((2.0, 1.0))[0] == -1
    flat = type("F", (), {"tri_obj": np.zeros(32, np.int32)})

    def occ(tr, tt):
        tt = np.asarray(tt, np.float32)
        c = rr.Candidates(1, np.zeros(tt.size, np.int64), np.arange(tt.size, dtype=np.int64), tt)
        return int(rr.occluded(c, flat, None if tr is None else np.array([tr], np.float32))[0])
    assert occ(None, [-inf]) == 0 and occ(None, [nan]) == 1 and occ(None, [inf]) == 1 and occ(None, []) == 0
    assert occ((0.0, 1.0), [nan]) == 1 and occ((0.0, 1.0), [inf]) == 0 and occ((0.0, 1.0), [1.0]) == 1 and occ((0.0, 1.0), [1.5]) == 0
    assert occ((1.0, 0.0), [0.5]) == 0 and occ((nan, 1.0), [0.5]) == 1 and occ((nan, 1.0), [1.5]) == 0


def test_python_interface():
    """The four entry points are in the symbol list the header is compared with, and the methods take t_range."""
    import inspect
    assert {"srt_trace_rays_range_device", "srt_trace_rays_range", "srt_occluded_range_device", "srt_occluded_range"} <= set(lib.ABI_SYMBOLS)
    for name in ("trace_rays", "occluded", "trace_rays_device", "occluded_device"):
        p = inspect.signature(getattr(lib.DeviceScene, name)).parameters
        assert "t_range" in p and p["t_range"].default is None, name


def test_argument_errors_without_device_work():
    """A NULL handle is refused before anything is touched: SRT_ERR_ARG, on a machine without a device too."""
    import ctypes as C
    from simple_raytracer_amd import abi
    build.build_all()
    L = lib.load()
    rays = np.zeros((4, 6), np.float32); tr = np.zeros((4, 2), np.float32)
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    hit = np.full(4, -7, np.int32); occ = np.full(4, 9, np.uint8)
    st = abi.Stats()
    r, q = rays.ctypes.data_as(f32p), tr.ctypes.data_as(f32p)
    assert L.srt_trace_rays_range(None, 4, r, q, 0, hit.ctypes.data_as(i32p), None, None, C.byref(st)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_range(None, 0, None, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_range(None, 4, r, q, None, occ.ctypes.data_as(u8p)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_range_device(None, 4, None, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_range_device(None, 4, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert (hit == -7).all() and (occ == 9).all()
