"""CPU-only: the yardstick of the shaded-ray tests (tests/shade_query_ref.py) holds on the oracle itself -- a pixel of a camera-mode
frame and that pixel's ray as a 1 x 1 frame of its own give the same hit, t, pre-tone-map colour and bytes -- and the argument checks
of srt_shade_rays that need no device."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import shade_query_ref as sq
from simple_raytracer_amd import abi, build, lib

W, H, N_LIGHTS = 48, 27, 5


@pytest.mark.parametrize("name,flags", [("cubes4_a40", 0), ("texquad", 0), ("ground_bunny", 0), ("texquad", abi.SRT_FLAG_SMOOTH_NORMALS)])
def test_a_frame_is_its_rays(oracle, name, flags):
    """48 x 27 frame, the SHEAR matrix, a 5-sample staircase at the golden light, pow = "device": every pixel equals its own ray's
    1 x 1 frame (focal 1, ray_matrix columns (0, 0, d, o)) in hit id, t bits, rgb_linear bits and rgb8 bytes."""
    g = gu.GoldenScene(name)
    flat = sq.texquad_with_normals(g) if flags & abi.SRT_FLAG_SMOOTH_NORMALS else g.flat
    focal = rq.FOCAL[name] * W / rq.FRAME_W                      # the view of the 320 x 180 cases
    lights = abi.light_staircase(g.light, N_LIGHTS)
    c = sq.frame_shade(oracle, flat, W, H, rq.SHEAR, focal, lights, flags=flags)
    rays = rq.frame_rays(W, H, rq.SHEAR, focal)
    hit, t, lin, rgb8 = sq.oracle_shade(oracle, flat, rays, lights, flags=flags)
    n_hit = int((hit >= 0).sum())
    print(name, flags, "hits", n_hit, "of", W * H)
    assert 0 < n_hit < W * H
    assert np.array_equal(hit, c["hit_id"].reshape(-1))
    assert np.array_equal(sq.bits(t), sq.bits(c["t"].reshape(-1)))
    assert np.array_equal(sq.bits(lin), sq.bits(c["rgb_linear"].reshape(-1, 3)))
    assert np.array_equal(rgb8, c["rgb8"].reshape(-1, 3))
    # the colours are worth comparing: hits are not all one colour, misses carry the background
    assert len(np.unique(rgb8[hit >= 0], axis=0)) > 4
    assert (rgb8[hit < 0] == np.array(abi.REFERENCE_BACKGROUND, np.uint8)).all() and (lin[hit < 0] == 0).all()


def test_smooth_normals_change_the_frame(oracle):
    """The flag reaches the oracle: texquad's smooth frame is not its flat frame (else the smooth case above pins nothing new)."""
    g = gu.GoldenScene("texquad")
    focal = rq.FOCAL["texquad"] * W / rq.FRAME_W
    lights = abi.light_staircase(g.light, N_LIGHTS)
    flat = sq.texquad_with_normals(g)
    a = sq.frame_shade(oracle, flat, W, H, rq.SHEAR, focal, lights)
    b = sq.frame_shade(oracle, flat, W, H, rq.SHEAR, focal, lights, flags=abi.SRT_FLAG_SMOOTH_NORMALS)
    assert np.array_equal(a["hit_id"], b["hit_id"]) and not np.array_equal(sq.bits(a["rgb_linear"]), sq.bits(b["rgb_linear"]))


@pytest.fixture(scope="module")
def L():
    build.build_all()
    return lib.load()


def test_both_entry_points_are_bound(L):
    assert "srt_shade_rays" in lib.ABI_SYMBOLS and "srt_shade_rays_device" in lib.ABI_SYMBOLS
    assert hasattr(L, "srt_shade_rays") and hasattr(L, "srt_shade_rays_device")
    assert hasattr(lib.DeviceScene, "shade_rays") and hasattr(lib.DeviceScene, "shade_rays_device")


def test_argument_errors_without_a_device(L):
    """No handle can exist without a device, so every call here has a NULL handle, alone and together with the other NULLs: all are
    SRT_ERR_ARG, nothing is written (the cases with a live handle are in tests/test_gpu_shade_query.py)."""
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    rays = np.zeros((4, 6), np.float32); rays[:, 5] = 1.0
    out = np.full(4, -7, np.int32)
    p = sq.shade_params(np.zeros((1, 3), np.float32))
    st = abi.Stats()
    r, o = rays.ctypes.data_as(f32p), out.ctypes.data_as(i32p)
    assert L.srt_shade_rays(None, 4, r, C.byref(p), o, None, None, None, C.byref(st)) == abi.SRT_ERR_ARG
    assert L.srt_shade_rays(None, 4, r, None, o, None, None, None, None) == abi.SRT_ERR_ARG                 # NULL p
    assert L.srt_shade_rays(None, 4, None, C.byref(p), o, None, None, None, None) == abi.SRT_ERR_ARG        # NULL rays, n > 0
    assert L.srt_shade_rays(None, 0, None, C.byref(p), None, None, None, None, None) == abi.SRT_ERR_ARG     # n = 0 does not excuse the handle
    assert L.srt_shade_rays_device(None, 4, None, C.byref(p), None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_shade_rays_device(None, 4, None, None, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert (out == -7).all() and st.primary_rays == 0
