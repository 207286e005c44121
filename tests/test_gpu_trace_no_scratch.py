"""The fused trace kernel without scratch (k_trace_nq at seven waves per SIMD, and its batch form): the frames are what they were.
Smallest shapes that reach the changed code: two scenes with a ground slab (shadow rays that walk another object's tree), partial tiles
on both edges (37 x 29) and whole ones (64 x 40), 1, 4 and 7 light samples (7 is the last fused count; from 2 on the sample-chunk loop
divides items by the sample count and its LDS masks hold more than one sample).  Yardsticks: the oracle at the bars of
tests/test_gpu_parity.py (hit ids equal, t bit for bit, colours under that file's rules), and variant 11 -- the same body built for five
waves per SIMD -- bit for bit."""
import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
from simple_raytracer_amd import abi
from test_gpu_parity import TOL_LINEAR, bits, check_rgb8, strict

pytestmark = pytest.mark.gpu

FUSED = "k_trace_nq+k_shade_tile"
V_FUSED_5_WAVES = 11
OUTPUTS = ("hit_id", "t", "rgb_linear", "rgb8")


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


_scenes = {}
_oracle_frames = {}


def device_scene(srt, name):
    if name not in _scenes:
        g = gu.GoldenScene(name)
        _scenes[name] = (g, srt.DeviceScene(g.flat))
    return _scenes[name]


def oracle_frame(oracle, g, name, W, H, L):
    """The oracle's frame, computed once per shape and left unchanged."""
    key = (name, W, H, L)
    if key not in _oracle_frames:
        c = oracle.render(g.flat, g.params(W, H, L))
        for k in OUTPUTS:
            c[k].setflags(write=False)
        _oracle_frames[key] = c
    return _oracle_frames[key]


def same_bits(a, b, what):
    assert np.array_equal(a["hit_id"], b["hit_id"]), f"{what}: hit ids differ"
    assert np.array_equal(a["rgb8"], b["rgb8"]), f"{what}: rgb8 differs"
    for k in ("t", "rgb_linear"):
        assert np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k} differs"


@pytest.mark.parametrize("L", [1, 4, 7])
@pytest.mark.parametrize("W,H", [(37, 29), (64, 40)])
@pytest.mark.parametrize("name", ["cube_ground", "ground_bunny"])
def test_fused_frames_match_the_oracle_and_the_five_wave_build(srt, oracle, name, W, H, L):
    g, ds = device_scene(srt, name)
    p = g.params(W, H, L)
    o = ds.render(p)
    assert ds.pipeline == FUSED
    c = oracle_frame(oracle, g, name, W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    assert np.array_equal(o["hit_id"], c["hit_id"])
    assert np.array_equal(bits(o["t"]), bits(c["t"]))
    assert np.abs(o["rgb_linear"] - c["rgb_linear"]).max() < TOL_LINEAR
    check_rgb8(o["rgb8"], c["rgb8"])
    strict(srt, oracle, o, g.flat, p, f"{name} {W}x{H} L{L}")
    five = ds.render(g.params(W, H, L, flags=V_FUSED_5_WAVES << 8))
    assert ds.pipeline == FUSED
    same_bits(o, five, f"{name} {W}x{H} L{L} against variant 11")


def test_batch_of_a_half_split_is_the_frame_by_frame_result(srt):
    """k_trace_nq_batch: two frames (two light positions) of one half of cube_ground at 64 x 40 -- scanline blocks of 8 rows dealt to
    two owners, the first owner's 24 rows; a batch launches frames of ONE size together -- in ONE srt_render_device_batch call against
    the same two frames rendered one by one."""
    L_ = srt.load()
    g, ds = device_scene(srt, "cube_ground")
    W, H = 64, 40
    params = []
    for k in range(2):
        light = g.light.copy(); light[0] += 40.0 * k
        params.append(abi.make_params(W, H, abi.light_staircase(light, 4), block_rows=8, block_first=0, block_stride=2))
    handles = [ds.share() for _ in params]
    frames = [gf.PinnedFrame(L_, h.rows(p), h.cols(p)) for h, p in zip(handles, params)]
    try:
        srt.FrameBatch(handles, params, *[[f.ptrs[k] for f in frames] for k in range(4)]).render()
        for h in handles:
            h.sync()
            assert h.pipeline == FUSED + " (batched)"
        for k, (f, p) in enumerate(zip(frames, params)):
            f.check_untouched(gf.owned(p), f"frame {k}")
            one = ds.render(p)
            assert ds.pipeline == FUSED
            assert (one["hit_id"] >= 0).any()
            same_bits(f.out(), one, f"frame {k} of the batch")
    finally:
        for f in frames:
            f.free()
        for h in handles:
            h.close()


def test_frame_edge_five_rows_of_an_8x8_frame(srt, oracle):
    """One tile whose last three rows are outside the call (rows = 5): the oracle's five rows, nothing written beyond them."""
    g, ds = device_scene(srt, "cube_ground")
    p = g.params(8, 8, 4, block_rows=5, block_first=0, block_stride=10 ** 6)
    assert ds.rows(p) == 5
    o, pipeline = gf.render_pinned(srt, ds, p)
    assert pipeline == FUSED
    c = oracle.render(g.flat, p)
    assert np.array_equal(o["hit_id"], c["hit_id"])
    assert np.array_equal(bits(o["t"]), bits(c["t"]))
    assert np.abs(o["rgb_linear"] - c["rgb_linear"]).max() < TOL_LINEAR
    check_rgb8(o["rgb8"], c["rgb8"])
    strict(srt, oracle, o, g.flat, p, "8x8, five rows")
    five, _ = gf.render_pinned(srt, ds, g.params(8, 8, 4, block_rows=5, block_first=0, block_stride=10 ** 6, flags=V_FUSED_5_WAVES << 8))
    same_bits(o, five, "8x8, five rows against variant 11")
