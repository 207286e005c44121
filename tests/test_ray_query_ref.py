"""CPU: the yardstick of the ray-query tests (tests/ray_query_ref.py) pinned against the oracle itself, and the parts of the feature
that need no device -- the Python methods exist, and srt_trace_rays / srt_occluded refuse their arguments before any device work."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
from simple_raytracer_amd import abi, build, lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import host
    build.build_host()
    return host.Transformation


def test_a_frame_is_its_rays_one_by_one(oracle):
    """ground_bunny at 160 x 120 under a sheared, scaled matrix: 200 random pixels re-traced as 1 x 1 frames whose ray is
    frame_rays' give the frame's hit id and t bits -- so frame_rays reproduces the oracle's directions and the 1 x 1 trick its ray."""
    g = gu.GoldenScene("ground_bunny")
    W, H, focal = 160, 120, 33.0
    c = oracle.render(g.flat, rq.camera_params(W, H, rq.SHEAR, focal, g.light))
    rays = rq.frame_rays(W, H, rq.SHEAR, focal)
    assert not np.signbit(rays[:, 3:6][rays[:, 3:6] == 0]).any(), "a -0 direction component would not survive the 1 x 1 frame"
    pick = np.random.default_rng(7).choice(W * H, 200, replace=False)
    hit, t = rq.oracle_trace(oracle, g.flat, rays[pick])
    want_hit, want_t = c["hit_id"].reshape(-1)[pick], c["t"].reshape(-1)[pick]
    assert (want_hit >= 0).sum() >= 20 and (want_hit < 0).sum() >= 20
    assert np.array_equal(hit, want_hit)
    assert np.array_equal(bits(t), bits(want_t))


@pytest.mark.parametrize("name", sorted(rq.SHADOW_LIGHT))
def test_two_frames_read_out_every_shadow(oracle, T, name):
    """The two-frame read-out leaves no hit pixel out (no zero or non-finite unshadowed colour), and the moved light puts at least
    1 % of the hit pixels in shadow and leaves at least 1 % lit."""
    g = gu.GoldenScene(name)
    hit, t, shadowed, usable = rq.shadow_readout(oracle, g.flat, rq.FRAME_W, rq.FRAME_H, rq.rigid(T, 4.0), rq.FOCAL[name], rq.SHADOW_LIGHT[name])
    is_hit = hit >= 0
    assert is_hit.sum() > 10000
    assert np.array_equal(usable, is_hit), f"{int((is_hit & ~usable).sum())} hit pixels cannot be read out"
    assert not shadowed[~is_hit].any()
    share = shadowed[is_hit].mean()
    assert 0.01 <= share <= 0.99, share


def test_unrelated_rays_hit_and_miss(oracle):
    for name in ("ground_bunny", "cubes4_a40"):
        g = gu.GoldenScene(name)
        rays = rq.unrelated_rays(g.flat, 400)
        assert np.isfinite(rays).all() and not np.signbit(rays[:, 3:6][rays[:, 3:6] == 0]).any()
        hit, _ = rq.oracle_trace(oracle, g.flat, rays)
        assert 0.2 <= (hit >= 0).mean() <= 0.8, name


def test_python_methods_exist():
    for name in ("trace_rays", "occluded", "trace_rays_device", "occluded_device"):
        assert callable(getattr(lib.DeviceScene, name, None)), name
    assert {"srt_trace_rays_device", "srt_trace_rays", "srt_occluded_device", "srt_occluded"} <= set(lib.ABI_SYMBOLS)


def test_argument_errors_without_device_work():
    """A NULL handle is refused before anything is touched: SRT_ERR_ARG, on a machine without a device too."""
    build.build_all()
    L = lib.load()
    rays = np.zeros((4, 6), np.float32)
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    hit = np.full(4, -7, np.int32); occ = np.full(4, 9, np.uint8)
    st = abi.Stats()
    assert L.srt_trace_rays(None, 4, rays.ctypes.data_as(f32p), 0, hit.ctypes.data_as(i32p), None, None, C.byref(st)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays(None, 0, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded(None, 4, rays.ctypes.data_as(f32p), None, occ.ctypes.data_as(u8p)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_device(None, 4, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_device(None, 4, None, None, None, None) == abi.SRT_ERR_ARG
    assert (hit == -7).all() and (occ == 9).all()
