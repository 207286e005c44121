"""No GPU, no library: which C symbol every query method of lib.DeviceScene reaches, over the full cross of its optional arguments, and with
how many arguments -- the count the prototype of that symbol in include/srt.h has.  The scene is made without __init__ and its library is
a recorder that answers 0.  The host calls that patch params.flags for one call leave them as they were, also when the call raises."""
import itertools
import os
import re

import numpy as np
import pytest

from simple_raytracer_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3
GEOMETRY = ("srt_rows_owned", "srt_cols_owned")      # what render_paths asks before its call: answered, not recorded, never failing
RULE, VIS = (1e-3, 1.0, True), (1, 2, 4)
N_OBJECTS = 2


def prototypes():
    """name -> number of parameters, from the header."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srt.h")).read(), flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"^int\s+(srt_[a-z_0-9]+)\s*\((.*?)\)\s*;", hdr, re.M | re.S)}


ARGC = prototypes()


class Boom(RuntimeError):
    pass


class Recorder:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def __getattr__(self, name):
        def call(*args):
            if name in GEOMETRY:
                return 2
            self.calls.append((name, len(args)))
            if self.fail:
                raise Boom(name)
            return 0
        return call


class Flat:
    n_objects = N_OBJECTS


def scene(fail=False):
    ds = lib.DeviceScene.__new__(lib.DeviceScene)
    ds.h, ds.flat, ds.L = None, Flat(), Recorder(fail)      # (h None: __del__ and close() have nothing to destroy)
    return ds


def reached(ds, symbol):
    assert ds.L.calls == [(symbol, ARGC[symbol])], (ds.L.calls, symbol, ARGC[symbol])


def params(flags=abi.SRT_FLAG_NO_TIMING):
    return abi.make_params(4, 2, np.zeros((1, 3), np.float32), flags=flags)


RAYS = np.zeros((N, 6), np.float32)
T_RANGE = np.tile(np.float32([0.0, 1.0]), (N, 1))
MASKS = np.arange(N, dtype=np.uint32)


def closest_symbol(stem, t_range, ray_mask, suffix):
    return stem + ("_masked" if ray_mask is not None else "_range" if t_range is not None else "") + suffix


@pytest.mark.parametrize("t_range,ray_mask", list(itertools.product((None, T_RANGE), (None, True, MASKS))))
def test_closest_hit_and_occlusion_host(t_range, ray_mask):
    ds = scene()
    o = ds.trace_rays(RAYS, t_range=t_range, ray_mask=ray_mask)
    reached(ds, closest_symbol("srt_trace_rays", t_range, ray_mask, ""))
    assert o["hit_id"].shape == (N,) and o["t"].shape == (N,) and o["bary"].shape == (N, 3) and "stats" in o
    for skip in (None, np.zeros(N, np.int32)):
        ds = scene()
        assert ds.occluded(RAYS, skip, t_range=t_range, ray_mask=ray_mask).shape == (N,)
        reached(ds, closest_symbol("srt_occluded", t_range, ray_mask, ""))


@pytest.mark.parametrize("t_range,ray_mask", list(itertools.product((None, 0x1000), (None, 0, 0x2000))))
def test_closest_hit_and_occlusion_device(t_range, ray_mask):
    ds = scene()
    ds.trace_rays_device(N, 0x100, hit_id=0x200, count=True, t_range=t_range, ray_mask=ray_mask)
    reached(ds, closest_symbol("srt_trace_rays", t_range, ray_mask, "_device"))
    ds = scene()
    ds.occluded_device(N, 0x100, 0x300, t_range=t_range, ray_mask=ray_mask)
    reached(ds, closest_symbol("srt_occluded", t_range, ray_mask, "_device"))


@pytest.mark.parametrize("t_range", [None, T_RANGE])
def test_multi_and_surface(t_range):
    ds = scene()
    o = ds.trace_rays_multi(RAYS, 4, t_range=t_range)
    reached(ds, "srt_trace_rays_multi")
    assert o["n_hits"].shape == (N,) and o["hit_id"].shape == (N, 4) and o["bary"].shape == (N, 4, 3)
    ds = scene()
    ds.trace_rays_multi_device(N, 0x100, 4, t_range=None if t_range is None else 0x1000)
    reached(ds, "srt_trace_rays_multi_device")
    ds = scene()
    o = ds.surface_rays(RAYS, t_range=t_range, smooth=True, count=True)
    reached(ds, "srt_surface_rays")
    assert o["hit_id"].shape == (N,) and o["obj"].shape == (N,) and o["normal"].shape == (N, 3) and o["bounce"].shape == (N, 6) and "stats" in o
    ds = scene()
    ds.surface_rays_device(N, 0x100, obj=0x200, t_range=None if t_range is None else 0x1000)
    reached(ds, "srt_surface_rays_device")
    ds = scene()
    o = ds.surface_hits(RAYS, np.zeros(N, np.int32), np.ones(N, np.float32), want=("point", "bounce"))
    reached(ds, "srt_surface_hits")
    assert set(o) == {"point", "bounce"} and o["point"].shape == (N, 3)
    ds = scene()
    ds.surface_hits_device(N, 0x100, 0x200, 0x300, normal=0x400)
    reached(ds, "srt_surface_hits_device")


def restored(call, symbol, flags):
    """call(ds, p) reaches `symbol` and leaves p.flags at `flags`, whether the library answers or raises."""
    ds, p = scene(), params(flags)
    out = call(ds, p)
    reached(ds, symbol)
    assert p.flags == flags
    ds, p = scene(fail=True), params(flags)
    with pytest.raises(Boom):
        call(ds, p)
    reached(ds, symbol)
    assert p.flags == flags
    return out


@pytest.mark.parametrize("t_range", [None, T_RANGE])
def test_shaded_rays(t_range):
    symbol = "srt_shade_rays" if t_range is None else "srt_shade_rays_range"
    for flags, count in itertools.product((0, abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_COUNT_WORK), (False, True)):
        o = restored(lambda ds, p: ds.shade_rays(RAYS, p, count=count, t_range=t_range), symbol, flags)
        assert o["hit_id"].shape == (N,) and o["rgb_linear"].shape == (N, 3) and o["rgb8"].dtype == np.uint8 and "stats" in o
    ds = scene()
    ds.shade_rays_device(N, 0x100, params(), rgb8=0x200, t_range=None if t_range is None else 0x1000)
    reached(ds, symbol + "_device")


def path_symbol(stem, shadow, visibility, ior, suffix):
    return stem + ("_refract" if ior is not None else "_masked" if visibility is not None else "_shadow" if shadow is not None else "") + suffix


PATH_CROSS = list(itertools.product((None, RULE), (None, VIS), (None, "table")))
SEG_KEYS = ("seg_hit_id", "seg_t", "seg_obj", "seg_rgb_linear", "seg_rays")


@pytest.mark.parametrize("shadow,visibility,ior", PATH_CROSS)
def test_path_calls_host(shadow, visibility, ior):
    table = None if ior is None else np.float32([0.0, 1.5])
    for count, smooth, flags in ((False, False, abi.SRT_FLAG_NO_TIMING), (True, False, 0), (False, True, abi.SRT_FLAG_COUNT_WORK), (True, True, 0)):
        o = restored(lambda ds, p: ds.shade_paths(RAYS, p, 2, np.float32([0.5, 0.25]), t_range=T_RANGE, count=count, smooth=smooth, shadow=shadow,
                                                  visibility=visibility, ior=table), path_symbol("srt_shade_paths", shadow, visibility, ior, ""), flags)
        assert o["rgb_linear"].shape == (N, 3) and o["rgb8"].shape == (N, 3) and o["seg_hit_id"].shape == (2, N) and o["seg_rays"].shape == (2, N, 6) and "stats" in o
        o = restored(lambda ds, p: ds.render_paths(p, 2, None, count=count, smooth=smooth, fill=7, shadow=shadow, visibility=visibility, ior=table),
                     path_symbol("srt_render_paths", shadow, visibility, ior, ""), flags)
        assert o["rgb_linear"].shape == (2, 2, 3) and o["seg_t"].shape == (2, 2, 2) and o["seg_rgb_linear"].shape == (2, 2, 2, 3)
        assert all((o[k] == 7).all() for k in ("rgb_linear", "rgb8") + SEG_KEYS)
    o = scene().shade_paths(RAYS, params(), 2, want=("rgb8", "seg_obj"), shadow=shadow, visibility=visibility, ior=table)
    assert set(o) == {"rgb8", "seg_obj", "stats"}


@pytest.mark.parametrize("shadow,visibility,ior", PATH_CROSS)
def test_path_calls_device(shadow, visibility, ior):
    for table in ((None,) if ior is None else (0, 0x3000)):      # (0: the _refract call without a table)
        ds = scene()
        ds.shade_paths_device(N, 0x100, params(), 2, reflectance=0x200, t_range=0x1000, rgb8=0x300, shadow=shadow, visibility=visibility, ior=table)
        reached(ds, path_symbol("srt_shade_paths", shadow, visibility, ior, "_device"))
        ds = scene()
        ds.render_paths_device(params(), 2, rgb_linear=0x300, seg_t=0x400, shadow=shadow, visibility=visibility, ior=table)
        reached(ds, path_symbol("srt_render_paths", shadow, visibility, ior, "_device"))
