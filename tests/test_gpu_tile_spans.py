"""GPU (-m gpu): the tile spans (simple_raytracer_amd/csrc/srt_tile_spans.h) on the device.

The fused frame's trace launch starts workgroups only for the tiles inside the spans of the frame's table, and the shading launch fills
the tiles outside with background.  Every case renders the frame twice into sentinel-filled pinned buffers -- as shipped (variant 0)
and with the table off and the full grid launched (variant 64) -- and asks for the same bits in hit_id, t, rgb_linear and rgb8 and the
same hit_rays from srt_sync; where a golden frame or the oracle is at hand, for those too.  At the reference's focal length of 400 a
96x54 frame lies wholly inside every golden scene, so every case also runs at focal 40, where the scenes have background all round
and the table does exclude tiles.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import pose_ref
import refit_ref
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FULL_GRID = 64 << 8                    # srt_params.flags bits 8..15: variant 64, the table off
SIZES = [(96, 54), (100, 52)]


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, host
    build.build_host()
    return host.Transformation


def with_flags(p, extra):
    q = abi.Params.from_buffer_copy(p)
    q.flags = p.flags | extra
    return q


def same_bits(a, b, what):
    assert np.array_equal(a["hit_id"], b["hit_id"]), f"{what}: hit_id"
    for k in ("t", "rgb_linear"):
        assert np.array_equal(gf.bits(a[k]), gf.bits(b[k])), f"{what}: {k}"
    assert np.array_equal(a["rgb8"], b["rgb8"]), f"{what}: rgb8"
    assert a["stats"]["hit_rays"] == b["stats"]["hit_rays"], f"{what}: hit_rays {a['stats']['hit_rays']} != {b['stats']['hit_rays']}"


def shipped_and_full(srt, ds, p, what):
    """The frame as shipped and on the full grid, compared; returns the shipped frame."""
    o, pipe = gf.render_pinned(srt, ds, p)
    f, pipe_f = gf.render_pinned(srt, ds, with_flags(p, FULL_GRID))
    assert pipe == pipe_f, f"{what}: variant 64 took other kernels ({pipe} / {pipe_f})"
    same_bits(o, f, what)
    assert o["stats"]["hit_rays"] == int((o["hit_id"] >= 0).sum()), what
    return o


@pytest.mark.parametrize("name", ["cube", "cube_ground", "cubes4_a40", "spheres6", "ground_bunny"])
def test_shipped_equals_full_grid(srt, name):
    g = gu.GoldenScene(name)
    ds = srt.DeviceScene(g.flat)
    excluded_somewhere = False
    for (W, H) in SIZES:
        for focal in (400.0, 40.0):
            for L in (1, 4, 8):                        # 8: the unfused pipeline, which keeps its full grid
                for hint in (0, abi.SRT_FLAG_FRAMES_IN_FLIGHT):      # four waves per tile / the half-tile form
                    p = g.params(W, H, L, focal=focal, flags=hint)
                    o = shipped_and_full(srt, ds, p, f"{name} {W}x{H} focal {focal} L={L} flags={hint}")
                    if focal == 400.0 and g.out(W, H, L, "hit_id") is not None:
                        assert np.array_equal(o["hit_id"], g.out(W, H, L, "hit_id")), "golden hit ids"
                        assert np.array_equal(gf.bits(o["t"]), gf.bits(g.out(W, H, L, "t"))), "golden t"
                    tiles = np.zeros(((H + 7) // 8 * 8, (W + 7) // 8 * 8), bool); tiles[:H, :W] = o["hit_id"] >= 0
                    tiles = tiles.reshape((H + 7) // 8, 8, (W + 7) // 8, 8).any(axis=(1, 3))
                    gy, gx = tiles.shape
                    pad = np.zeros((gy + 4, gx + 4), bool); pad[2:-2, 2:-2] = tiles
                    near = np.zeros_like(tiles)           # tiles within two tiles of a tile with a hit
                    for dy in range(5):
                        for dx in range(5):
                            near |= pad[dy:dy + gy, dx:dx + gx]
                    excluded_somewhere |= bool((~near).any())
    assert excluded_somewhere, "no frame of this scene had background: the table excluded nothing"
    ds.close()


def moved(flat, T, k, dx, dy, dz):
    mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1))
    mats[k] = T.changeObjPosition(dx, dy, dz)
    return mats


def test_nothing_in_view_and_everything_in_view(srt, oracle, T):
    """An object pushed wholly off the frame: no live tile row (one tile stays, srt_tile_spans.h).  An object that holds the origin:
    every tile stays.  Both created from the moved scene, so the table is made from these boxes."""
    g = gu.GoldenScene("cube")
    r = int(g.flat.obj_root[0])
    c = 0.5 * (g.flat.node_min.reshape(-1, 3)[r] + g.flat.node_max.reshape(-1, 3)[r])
    for what, d in (("off the frame", (50000.0, 0.0, 0.0)), ("around the origin", tuple(float(-x) for x in c))):
        want = pose_ref.pose_flat(g.flat, moved(g.flat, T, 0, *d))
        ds = srt.DeviceScene(want)
        for (W, H) in SIZES:
            for hint in (0, abi.SRT_FLAG_FRAMES_IN_FLIGHT):
                p = g.params(W, H, 2, focal=40.0, flags=hint)
                o = shipped_and_full(srt, ds, p, f"{what} {W}x{H}")
                gf.compare_exact(srt, o, oracle.render(want, p, pow="device"), gf.owned(p), want, p, what)
                assert (o["stats"]["hit_rays"] == 0) == (what == "off the frame")
        ds.close()


def stale_setup(srt, T):
    g = gu.GoldenScene("cube")
    p = g.params(96, 54, 2, focal=40.0)
    r = int(g.flat.obj_root[0])
    z = 0.5 * float(g.flat.node_min.reshape(-1, 3)[r][2] + g.flat.node_max.reshape(-1, 3)[r][2])
    mats = moved(g.flat, T, 0, 30.0 * z / 40.0, 0.0, 0.0)            # 30 pixels to the right at the cube's depth
    return g, p, mats


def check_moved(srt, oracle, ds, want, p, first, what):
    """The frame after the boxes changed on the device only: the oracle's frame of the moved scene, with hits where the table of the
    FIRST frame excluded (or the case tests nothing)."""
    o, _ = gf.render_pinned(srt, ds, p)
    gf.compare_exact(srt, o, oracle.render(want, p, pow="device"), gf.owned(p), want, p, what)
    cols0 = np.nonzero((first["hit_id"] >= 0).any(axis=0))[0]; cols1 = np.nonzero((o["hit_id"] >= 0).any(axis=0))[0]
    assert cols1.max() > cols0.max() + 16, f"{what}: the object did not leave the first frame's spans ({cols0.max()} -> {cols1.max()})"


def test_pose_makes_the_table_invalid(srt, oracle, T):
    g, p, mats = stale_setup(srt, T)
    ds = srt.DeviceScene(g.flat); ds.set_pose_source()
    first = shipped_and_full(srt, ds, p, "before the pose")
    ds.pose(mats)
    check_moved(srt, oracle, ds, pose_ref.pose_flat(g.flat, mats), p, first, "after srt_scene_pose")
    # the next upload from the host brings the table back, for the uploaded boxes
    ds.update(g.flat)
    again = shipped_and_full(srt, ds, p, "after srt_scene_update")
    same_bits(again, first, "the created scene again")
    ds.close()


def test_pose_through_another_handle_makes_the_table_invalid(srt, oracle, T):
    g, p, mats = stale_setup(srt, T)
    ds = srt.DeviceScene(g.flat); ds.set_pose_source()
    other = ds.share()
    first = shipped_and_full(srt, other, p, "shared handle before the pose")
    ds.pose(mats); ds.sync()
    check_moved(srt, oracle, other, pose_ref.pose_flat(g.flat, mats), p, first, "shared handle, posed through the first")
    other.close(); ds.close()


def test_refit_device_makes_the_table_invalid(srt, oracle, T):
    g, p, mats = stale_setup(srt, T)
    ds = srt.DeviceScene(g.flat); ds.refit_prepare()
    first = shipped_and_full(srt, ds, p, "before the refit")
    pts = np.ascontiguousarray(pose_ref.transform_objects(g.flat, mats), np.float32).reshape(-1, 4)      # n_tris x 3 points of 4 floats, visit order
    L = srt.load()
    n = pts.size * 4
    ptr = L.srt_host_alloc(n)                       # pinned host memory: the device reads it in place
    assert ptr
    try:
        np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=np.float32)[:] = pts.reshape(-1)
        ds.refit_device(points=ptr, stride=4); ds.sync()
        check_moved(srt, oracle, ds, refit_ref.refit_flat(g.flat, pts.reshape(-1, 3, 4)), p, first, "after srt_scene_refit_device")
    finally:
        ds.close()
        L.srt_host_free(ptr)


def test_shares_of_a_split_keep_the_full_grid(srt, oracle):
    """Scanline blocks of a two-way split and column tiles: no table (the kernels' tile arithmetic is the share's), the frames are the
    oracle's and the full grid's."""
    g = gu.GoldenScene("cube")
    ds = srt.DeviceScene(g.flat)
    for kw in (dict(block_rows=8, block_first=0, block_stride=2), dict(block_rows=8, block_first=1, block_stride=2),
               dict(block_rows=8, block_first=1, block_stride=2, block_cols=8)):
        for hint in (0, abi.SRT_FLAG_FRAMES_IN_FLIGHT):
            p = g.params(100, 52, 2, focal=40.0, flags=hint, **kw)
            o = shipped_and_full(srt, ds, p, str(kw))
            c = oracle.render(g.flat, p, pow="device")
            gf.compare_exact(srt, o, c, gf.owned(p), g.flat, p, str(kw))
    ds.close()


def test_captured_frames_replay_the_eager_frames_and_follow_the_scene():
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py): the table travels in the captured kernel nodes, and a
    replay after srt_scene_update or srt_scene_pose has moved the object renders the moved scene (the oracle's frame)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "tile_spans_graph_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tile spans graph case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
