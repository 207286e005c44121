"""CPU-only: the ABI surface of ambient occlusion in a frame (include/srt.h, "Ambient occlusion in a frame") -- the four entry points
declared, exported and listed, the mirrors of srt_ao_frame and srt_ao_frame_out with their sizes and offsets, the Python signatures, the
rotation table, and the argument errors that need no device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from simple_raytracer_amd import abi, build, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("srt_render_ao_device", "srt_render_ao", "srt_render_ao_hits_device", "srt_render_ao_hits")


@pytest.fixture(scope="module")
def L():
    build.build_all()
    return lib.load()


def header():
    return open(os.path.join(ROOT, "include", "srt.h")).read()


def struct_fields(hdr, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.S)
    return m.group(1)


def test_header_declares_and_library_exports_the_four_entry_points(L):
    hdr = header()
    declared = set(re.findall(r"^int\s+(srt_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared, name
        assert name in lib.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+SRT_ABI_VERSION\s+3\b", hdr) and L.srt_abi_version() == 3      # additive only
    assert int(re.search(r"#define\s+SRT_AO_ROT_MAX\s+(\d+)", hdr).group(1)) == abi.SRT_AO_ROT_MAX == 64
    # the frame block follows the ambient-occlusion block and says what it still leaves out
    assert hdr.index("typedef struct srt_ao_out") < hdr.index("Ambient occlusion in a frame:") < hdr.index("typedef struct srt_ao_frame {")
    section = hdr[hdr.index("Ambient occlusion in a frame:"):hdr.index("typedef struct srt_ao_frame {")]
    assert "weights per direction" in section[section.index("NOT HERE"):]


def test_the_struct_mirrors(L):
    hdr = header()
    body = struct_fields(hdr, "srt_ao_frame")
    assert re.findall(r"(\w+)\s*[,;]", body) == ["rot_w", "rot_h", "rot"] == [f[0] for f in abi.AoFrame._fields_]
    body = struct_fields(hdr, "srt_ao_frame_out")
    fields = re.findall(r"\*\s*(\w+);", body)
    assert fields == ["n_occluded", "ao", "occ_bits", "bent", "ao8"] == [f[0] for f in abi.AoFrameOut._fields_] == list(abi.AO_FRAME_FIELDS)
    # two uint32, then a pointer at 8; five pointers
    assert C.sizeof(abi.AoFrame) == 16 and abi.AoFrame.rot_w.offset == 0 and abi.AoFrame.rot_h.offset == 4 and abi.AoFrame.rot.offset == 8
    ptr = C.sizeof(C.c_void_p)
    assert C.sizeof(abi.AoFrameOut) == 5 * ptr
    assert [getattr(abi.AoFrameOut, k).offset for k in abi.AO_FRAME_FIELDS] == [0, ptr, 2 * ptr, 3 * ptr, 4 * ptr]
    # the first three fields are srt_ao_out's, in its order
    assert list(abi.AO_FRAME_FIELDS)[:3] == list(abi.AO_FIELDS)
    assert (abi.AO_FRAME_FIELDS["bent"], abi.AO_FRAME_FIELDS["ao8"]) == ((np.float32, 3), (np.uint8, 1))


def test_the_python_signatures():
    p = inspect.signature(lib.DeviceScene.render_ao).parameters
    assert list(p)[:4] == ["self", "params", "dirs", "rot"] and p["rot"].default is None
    assert p["t_min"].default == 1e-3 and p["t_max"].default == np.inf and p["skip_self"].default is False and p["visibility"].default is None
    assert p["smooth"].default is False and p["count"].default is False and p["fill"].default is None
    assert set(p["want"].default) == {"hit_id", "t", "n_occluded", "ao", "occ_bits", "bent", "ao8"}
    p = inspect.signature(lib.DeviceScene.render_ao_hits).parameters
    assert list(p)[:5] == ["self", "params", "hit_id", "t", "dirs"] and set(p["want"].default) == {"n_occluded", "ao", "occ_bits", "bent", "ao8"}
    for method in ("render_ao_device", "render_ao_hits_device"):
        p = inspect.signature(getattr(lib.DeviceScene, method)).parameters
        assert p["stream"].default == 0 and p["bent"].default == 0 and p["ao8"].default == 0 and p["rot"].default == 0 and p["visibility"].default is None, method


def test_the_rotation_table():
    for w, h in ((1, 1), (4, 4), (3, 5), (64, 64)):
        r = lib.ao_rotations(w, h)
        assert r.shape == (h, w, 2) and r.dtype == np.float32
        assert np.abs(np.sqrt((r.astype(np.float64) ** 2).sum(axis=2)) - 1.0).max() < 2e-7
        assert np.array_equal(r.view(np.uint32), lib.ao_rotations(w, h).view(np.uint32))      # deterministic
    r = lib.ao_rotations(3, 5).astype(np.float64).reshape(-1, 2)
    k = np.arange(15)
    angle = 2.0 * np.pi * (((k + 0.5) * 0.6180339887498949) % 1.0)      # entry k = iy * w + ix, row-major
    assert np.allclose(r[:, 0], np.cos(angle), atol=1e-7) and np.allclose(r[:, 1], np.sin(angle), atol=1e-7)
    assert len({tuple(v) for v in lib.ao_rotations(4, 4).reshape(-1, 2).view(np.uint32).tolist()}) == 16, "sixteen different turns"


def test_a_null_handle_is_refused_without_device_work(L):
    hit = np.zeros(16, np.int32); t = np.ones(16, np.float32)
    dirs = lib.ao_directions(4)
    desc = abi.AoDesc(4, dirs.ctypes.data, 1e-3, 1.0, 0)
    rot = lib.ao_rotations(2, 2)
    frame = abi.AoFrame(2, 2, rot.ctypes.data)
    p = abi.make_params(4, 4, abi.light_staircase(np.float32([0, 0, 0]), 1))
    cnt = np.full(16, 7, np.uint32)
    out = abi.AoFrameOut(cnt.ctypes.data, None, None, None, None)
    hp, tp = hit.ctypes.data_as(C.POINTER(C.c_int32)), t.ctypes.data_as(C.POINTER(C.c_float))
    for fr in (None, C.byref(frame)):
        for o in (None, C.byref(out)):
            assert L.srt_render_ao(None, C.byref(p), 0, C.byref(desc), fr, None, None, None, o, None) == abi.SRT_ERR_ARG
            assert L.srt_render_ao_device(None, C.byref(p), 0, C.byref(desc), fr, None, None, None, None, o) == abi.SRT_ERR_ARG
            assert L.srt_render_ao_hits(None, C.byref(p), hp, tp, 0, C.byref(desc), fr, None, o, None) == abi.SRT_ERR_ARG
            assert L.srt_render_ao_hits_device(None, C.byref(p), hit.ctypes.data, t.ctypes.data, 0, C.byref(desc), fr, None, None, o) == abi.SRT_ERR_ARG
    assert cnt[0] == 7
