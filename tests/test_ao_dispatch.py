"""No GPU, no library: which C symbol each of the four ambient-occlusion methods of lib.DeviceScene reaches, over the cross of their
optional arguments, with how many arguments -- the count the prototype of that symbol in include/srt.h has -- and what the srt_ao_desc,
the flags and the srt_visibility it is handed hold.  tests/test_query_dispatch.py's recorder, in a file of its own: the scene is made
without __init__ and its library records and answers 0."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from simple_raytracer_amd import abi, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K = 3, 40
VIS = (1, 2, 4)


def prototypes():
    """name -> number of parameters, from the header."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "srt.h")).read(), flags=re.S)
    hdr = re.sub(r"//[^\n]*", "", hdr)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"^int\s+(srt_[a-z_0-9]+)\s*\((.*?)\)\s*;", hdr, re.M | re.S)}


ARGC = prototypes()


def pointee(arg, ty):
    """The struct behind a byref() argument (None: NULL was passed)."""
    return None if arg is None else C.cast(arg, C.POINTER(ty)).contents


class Recorder:
    """Answers 0 and keeps, per call: the name, the argument count, the flags, and copies of the srt_ao_desc, srt_visibility and srt_ao_out."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            device, hits = name.endswith("_device"), "_hits" in name
            i_flags = 5 if hits else 4
            desc, vis = pointee(args[i_flags + 1], abi.AoDesc), pointee(args[i_flags + 2], abi.Visibility)
            out = pointee(args[-1] if device else args[-2], abi.AoOut)
            self.calls.append(dict(name=name, argc=len(args), flags=args[i_flags], t_range=None if hits else args[3],
                                   desc=(desc.n_dirs, bool(desc.dirs), desc.t_min, desc.t_max, desc.flags),
                                   vis=None if vis is None else (vis.primary, vis.bounce, vis.shadow),
                                   out=(bool(out.n_occluded), bool(out.ao), bool(out.occ_bits))))
            return 0
        return call


def scene():
    ds = lib.DeviceScene.__new__(lib.DeviceScene)
    ds.h, ds.flat, ds.L = None, None, Recorder()      # (h None: __del__ and close() have nothing to destroy)
    return ds


def reached(ds, symbol, smooth, count, skip_self, visibility, t_range, out=(True, True, True)):
    assert len(ds.L.calls) == 1, ds.L.calls
    c = ds.L.calls[0]
    assert c["name"] == symbol and c["argc"] == ARGC[symbol], (c, ARGC[symbol])
    assert c["flags"] == (abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0) | (abi.SRT_FLAG_COUNT_WORK if count else 0), c
    assert c["desc"] == (K, True, np.float32(0.25), np.float32(7.0), abi.SRT_AO_SKIP_SELF if skip_self else 0), c
    assert c["vis"] == visibility and bool(c["t_range"]) == (t_range is not None) and c["out"] == out, c


RAYS = np.zeros((N, 6), np.float32)
T_RANGE = np.tile(np.float32([0.0, 1.0]), (N, 1))
DIRS = lib.ao_directions(K)
CROSS = list(itertools.product((None, VIS), (False, True), (False, True), (False, True)))


@pytest.mark.parametrize("visibility,smooth,count,skip_self", CROSS)
def test_host_forms(visibility, smooth, count, skip_self):
    for t_range in (None, T_RANGE):
        ds = scene()
        o = ds.ao_rays(RAYS, DIRS, 0.25, 7.0, t_range=t_range, skip_self=skip_self, visibility=visibility, smooth=smooth, count=count)
        reached(ds, "srt_ao_rays", smooth, count, skip_self, visibility, t_range)
        assert o["hit_id"].shape == (N,) and o["t"].shape == (N,) and o["n_occluded"].shape == (N,) and o["n_occluded"].dtype == np.uint32
        assert o["ao"].shape == (N,) and o["ao"].dtype == np.float32 and o["occ_bits"].shape == (N, 2) and o["occ_bits"].dtype == np.uint32 and "stats" in o
    ds = scene()
    o = ds.ao_hits(RAYS, np.zeros(N, np.int32), np.ones(N, np.float32), DIRS, 0.25, 7.0, skip_self=skip_self, visibility=visibility, smooth=smooth, count=count)
    reached(ds, "srt_ao_hits", smooth, count, skip_self, visibility, None)
    assert set(o) == {"n_occluded", "ao", "occ_bits", "stats"} and o["occ_bits"].shape == (N, 2)
    ds = scene()
    o = ds.ao_rays(RAYS, DIRS, 0.25, 7.0, skip_self=skip_self, visibility=visibility, smooth=smooth, count=count, want=("t", "ao"))
    reached(ds, "srt_ao_rays", smooth, count, skip_self, visibility, None, out=(False, True, False))
    assert set(o) == {"t", "ao", "stats"}


@pytest.mark.parametrize("visibility,smooth,count,skip_self", CROSS)
def test_device_forms(visibility, smooth, count, skip_self):
    for t_range in (None, 0x1000):
        ds = scene()
        ds.ao_rays_device(N, 0x100, 0x200, K, 0.25, 7.0, t_range=t_range, skip_self=skip_self, visibility=visibility, smooth=smooth, count=count, hit_id=0x300,
                          n_occluded=0x400, ao=0x500, occ_bits=0x600)
        reached(ds, "srt_ao_rays_device", smooth, count, skip_self, visibility, t_range)
    ds = scene()
    ds.ao_hits_device(N, 0x100, 0x300, 0x310, 0x200, K, 0.25, 7.0, skip_self=skip_self, visibility=visibility, smooth=smooth, count=count, occ_bits=0x600)
    reached(ds, "srt_ao_hits_device", smooth, count, skip_self, visibility, None, out=(False, False, True))


def test_defaults():
    ds = scene()
    ds.ao_rays(RAYS, DIRS)
    c = ds.L.calls[0]
    assert c["desc"][2:] == (np.float32(1e-3), np.float32(np.inf), 0) and c["flags"] == 0 and c["vis"] is None
