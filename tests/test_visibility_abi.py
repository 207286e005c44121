"""CPU-only: the ABI surface of the visibility masks (include/srt.h, "Visibility masks") -- the nine entry points declared, exported and
listed, the srt_visibility mirror, the Python keywords, and the argument errors that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from simple_raytracer_amd import abi, build, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srt_scene_set_object_masks", "srt_trace_rays_masked_device", "srt_trace_rays_masked", "srt_occluded_masked_device", "srt_occluded_masked",
       "srt_shade_paths_masked_device", "srt_shade_paths_masked", "srt_render_paths_masked_device", "srt_render_paths_masked")
_f32p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def L():
    build.build_all()
    return lib.load()


def test_header_declares_and_library_exports_the_nine_entry_points(L):
    hdr = open(os.path.join(ROOT, "include", "srt.h")).read()
    declared = set(re.findall(r"^int\s+(srt_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared, name
        assert name in lib.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"typedef\s+struct\s+srt_visibility\s*\{\s*uint32_t\s+primary\s*,\s*bounce\s*,\s*shadow\s*;\s*\}\s*srt_visibility\s*;", hdr)
    assert re.search(r"#define\s+SRT_ABI_VERSION\s+3\b", hdr) and L.srt_abi_version() == 3      # additive only
    # what is left out is said in the header
    assert "srt_trace_rays_multi" in hdr[hdr.index("NOT HERE"):hdr.index("typedef struct srt_visibility")]


def test_the_python_mirror(L):
    assert C.sizeof(abi.Visibility) == 12 and [f[0] for f in abi.Visibility._fields_] == ["primary", "bounce", "shadow"]
    v = abi.visibility((0xFFFFFFFF, 1, 0))
    assert (v.primary, v.bounce, v.shadow) == (0xFFFFFFFF, 1, 0) and abi.visibility(None) is None and abi.visibility(v) is v
    assert hasattr(lib.DeviceScene, "set_object_masks")
    for method in ("trace_rays", "trace_rays_device", "occluded", "occluded_device"):
        assert inspect.signature(getattr(lib.DeviceScene, method)).parameters["ray_mask"].default is None, method
    for method in ("shade_paths", "shade_paths_device", "render_paths", "render_paths_device"):
        assert inspect.signature(getattr(lib.DeviceScene, method)).parameters["visibility"].default is None, method


def test_a_null_handle_is_refused_without_device_work(L):
    p = abi.make_params(8, 8, abi.light_staircase(np.float32([0.0, 0.0, 0.0]), 1))
    pd = abi.PathDesc(2, 1e-3, None)
    rule, vis = abi.shadow_rule((1e-3, 1.0, False)), abi.visibility((1, 2, 3))
    rays = np.zeros((1, 6), np.float32)
    masks = np.ones(1, np.uint32)
    rp, mp = rays.ctypes.data_as(_f32p), masks.ctypes.data_as(_u32p)
    for m in (None, mp):
        assert L.srt_scene_set_object_masks(None, 1, m, None) == abi.SRT_ERR_ARG
        assert L.srt_trace_rays_masked(None, 1, rp, None, m, 0, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_occluded_masked(None, 1, rp, None, m, None, None) == abi.SRT_ERR_ARG
    for m in (None, masks.ctypes.data):
        assert L.srt_trace_rays_masked_device(None, 1, rays.ctypes.data, None, m, 0, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_occluded_masked_device(None, 1, rays.ctypes.data, None, m, None, None, None) == abi.SRT_ERR_ARG
    for r in (None, C.byref(rule)):
        for v in (None, C.byref(vis)):
            assert L.srt_shade_paths_masked(None, 1, rp, None, C.byref(p), C.byref(pd), r, v, None, None, None, None) == abi.SRT_ERR_ARG
            assert L.srt_shade_paths_masked_device(None, 1, rays.ctypes.data, None, C.byref(p), C.byref(pd), r, v, None, None, None, None) == abi.SRT_ERR_ARG
            assert L.srt_render_paths_masked(None, C.byref(p), C.byref(pd), r, v, None, None, None, None) == abi.SRT_ERR_ARG
            assert L.srt_render_paths_masked_device(None, C.byref(p), C.byref(pd), r, v, None, None, None, None) == abi.SRT_ERR_ARG
