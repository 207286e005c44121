"""GPU (-m gpu): refract_dir at its edges.  The goniometer of tests/refract_edges.py (tests/test_refract_edges_ref.py proves on the CPU that
its rows reach k < 0 next to k >= 0, k == 0, NaN k, c == +0, L == 0, L == inf, denormal and infinite values) through srt_shade_paths_refract
and srt_render_paths_refract against tests/refract_ref.py, bit for bit in every output -- seg_rays' segment 1 is refract_dir's own result.
Floats compare by bits; where the yardstick is NaN the device must be NaN; no tolerance anywhere."""
import numpy as np
import pytest

import refract_edges as re
import refract_ref as rf
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import surface_ref as sf
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
bits = sf.bits
TMIN = re.BOUNCE_T_MIN
_refs = {}


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def flags_of(smooth):
    return abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0


def reference(oracle, smooth, n_lights):
    """The yardstick's rows of the whole batch: computed once, shared, never changed."""
    key = (smooth, n_lights)
    if key not in _refs:
        ref = rf.shade_paths(oracle, re.scene(), re.batch()[0], re.lights(n_lights), re.DEPTH, re.IOR, re.REFLECTANCE, TMIN, flags=flags_of(smooth))
        for v in ref.values():
            v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def cut(ref, n):
    return {k: (v[:n] if k in ("rgb_linear", "rgb8") else v[:, :n]) for k, v in ref.items() if k in sp.ALL_KEYS}


def check_stats(o, want, n, n_lights):
    hits = int((want["seg_hit_id"] >= 0).sum())
    assert o["stats"]["primary_rays"] == n and o["stats"]["hit_rays"] == hits and o["stats"]["shadow_rays"] == hits * n_lights, o["stats"]


@gpu
@pytest.mark.parametrize("n_lights", [1, 3])
@pytest.mark.parametrize("smooth", [False, True])
def test_the_batch(srt, oracle, smooth, n_lights):
    flat, rays = re.scene(), re.batch()[0]
    want = reference(oracle, smooth, n_lights)
    ds = srt.DeviceScene(flat)
    before = ds.trace_rays(rays, want=("hit_id", "t"))
    for count in (False, True):
        o = ds.shade_paths(rays, sq.shade_params(re.lights(n_lights)), re.DEPTH, re.REFLECTANCE, TMIN, count=count, smooth=smooth, ior=re.IOR)
        sp.assert_same(o, want, f"smooth {smooth}, {n_lights} lights, counting {count}")
        if count:
            check_stats(o, want, rays.shape[0], n_lights)
    after = ds.trace_rays(rays, want=("hit_id", "t"))
    assert np.array_equal(before["hit_id"], after["hit_id"]) and np.array_equal(bits(before["t"]), bits(after["t"])), "the batch left something behind"
    assert np.array_equal(before["hit_id"], want["seg_hit_id"][0]) and np.array_equal(bits(before["t"]), bits(want["seg_t"][0]))
    ds.close()


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_leading_parts_of_the_batch(srt, oracle, n):
    """A ray's row depends on the ray alone: wave and workgroup edges."""
    flat, rays = re.scene(), re.batch()[0]
    ds = srt.DeviceScene(flat)
    for smooth in (False, True):
        o = ds.shade_paths(rays[:n], sq.shade_params(re.lights(3)), re.DEPTH, re.REFLECTANCE, TMIN, smooth=smooth, ior=re.IOR)
        sp.assert_same(o, cut(reference(oracle, smooth, 3), n), f"the first {n} rays, smooth {smooth}")
    ds.close()


@gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_the_frame(srt, oracle, smooth):
    """The goniometer's rays are no camera's, so the frame form runs a frame of its own over the sheets (refract_edges.frame_params) against
    refract_ref.render_paths."""
    flat = re.scene()
    p = re.frame_params(3, flags=flags_of(smooth))
    want = rf.render_paths(oracle, flat, p, re.DEPTH, re.IOR, re.REFLECTANCE, TMIN)
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.render_paths(p, re.DEPTH, re.REFLECTANCE, TMIN, count=count, ior=re.IOR)
        sp.assert_same(rpr.flat_rows(o), rpr.flat_rows(want), f"frame, smooth {smooth}, counting {count}")
        if count:
            check_stats(o, want, 256, 3)
    ds.close()
