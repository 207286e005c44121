"""The fused trace kernel's half-tile form (k_trace_nq_half: two waves of 8x4 pixels per 8x8 tile, srt_kernels.h): the frames are what
the four-wave form makes of them.  Smallest shapes that reach what the form changes: two scenes with a ground slab (shadow rays that
walk another object's tree); 37 x 29 (tiles cut on both edges, one live column and one live row in the last half), 36 x 28 (the bottom
half of the last tile row and the right quadrants of the last column have no live pixel: a wave without rays, a wave with one empty
quadrant) and 64 x 40 (whole tiles); 1, 4 and 7 light samples (7 is the last fused count; from 2 on the shadow rounds divide items by
the sample count -- by the 2^20 scale at 32 pixels per wave -- and a wave's LDS masks hold more than one sample).  Yardsticks: the
oracle at the bars of tests/test_gpu_parity.py (hit ids equal, t bit for bit, colours under that file's rules) and the four-wave form
under variant 59, bit for bit.  The dispatcher ships the half-tile form for frames in flight on several streams
(SRT_FLAG_FRAMES_IN_FLIGHT: the shipped render of these tests carries the hint) and the four-wave form for a frame alone; variant 13
forces the half-tile form, so it is pinned whichever form variant 0 picks for a frame."""
import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
from simple_raytracer_amd import abi
from test_gpu_parity import TOL_LINEAR, bits, check_rgb8, strict

pytestmark = pytest.mark.gpu

FUSED = "k_trace_nq+k_shade_tile"
IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
V_FUSED_HALF = 13           # the half-tile form, forced
V_FUSED_HALF_TINY = 14      # ... with a 160-entry node queue: the stackless overflow walk
V_FUSED_FOUR_WAVES = 59     # shipped choice with four waves of 4x4 pixels per tile
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


def at_the_oracles_bars(srt, oracle, o, c, flat, p, what):
    assert np.array_equal(o["hit_id"], c["hit_id"]), f"{what}: hit ids differ"
    assert np.array_equal(bits(o["t"]), bits(c["t"])), f"{what}: t differs"
    assert np.abs(o["rgb_linear"] - c["rgb_linear"]).max() < TOL_LINEAR, what
    check_rgb8(o["rgb8"], c["rgb8"])
    strict(srt, oracle, o, flat, p, what)


@pytest.mark.parametrize("L", [1, 4, 7])
@pytest.mark.parametrize("W,H", [(37, 29), (36, 28), (64, 40)])
@pytest.mark.parametrize("name", ["cube_ground", "ground_bunny"])
def test_frames_match_the_oracle_and_the_four_wave_form(srt, oracle, name, W, H, L):
    g, ds = device_scene(srt, name)
    p = g.params(W, H, L, flags=IN_FLIGHT)
    o = ds.render(p)
    assert ds.pipeline == FUSED
    c = oracle_frame(oracle, g, name, W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    at_the_oracles_bars(srt, oracle, o, c, g.flat, g.params(W, H, L), f"{name} {W}x{H} L{L}")      # (the hint is not the oracle's)
    four = ds.render(g.params(W, H, L, flags=V_FUSED_FOUR_WAVES << 8))
    assert ds.pipeline == FUSED
    same_bits(o, four, f"{name} {W}x{H} L{L} against variant 59")
    half = ds.render(g.params(W, H, L, flags=V_FUSED_HALF << 8))
    assert ds.pipeline == FUSED
    same_bits(half, four, f"{name} {W}x{H} L{L}, variant 13 against variant 59")
    alone = ds.render(g.params(W, H, L))
    assert ds.pipeline == FUSED
    same_bits(alone, four, f"{name} {W}x{H} L{L}, without the in-flight hint against variant 59")


def test_frame_edge_five_rows_of_an_8x8_frame(srt, oracle):
    """One tile whose last three rows are outside the call (rows = 5): wave 1 owns one live row.  The oracle's five rows, nothing
    written beyond them."""
    g, ds = device_scene(srt, "cube_ground")
    kw = dict(block_rows=5, block_first=0, block_stride=10 ** 6)
    p = g.params(8, 8, 4, **kw)
    assert ds.rows(p) == 5
    c = oracle.render(g.flat, p)
    four, _ = gf.render_pinned(srt, ds, g.params(8, 8, 4, flags=V_FUSED_FOUR_WAVES << 8, **kw))
    for what, flags in (("shipped, frames in flight", IN_FLIGHT), ("shipped, a frame alone", 0), ("variant 13", V_FUSED_HALF << 8)):
        o, pipeline = gf.render_pinned(srt, ds, g.params(8, 8, 4, flags=flags, **kw))      # (render_pinned: check_untouched beyond the owned rows)
        assert pipeline == FUSED
        at_the_oracles_bars(srt, oracle, o, c, g.flat, p, f"8x8, five rows, {what}")
        same_bits(o, four, f"8x8, five rows, {what} against variant 59")


@pytest.mark.parametrize("L", [1, 4])
def test_overflow_walk_with_32_rays_per_wave(srt, L):
    """The half-tile body with a 160-entry node queue (variant 14): 32 rays x 2 children fill it in the bunny's tree, and the wave
    finishes those subtrees by the stackless walk -- the shipped frame, bit for bit."""
    g, ds = device_scene(srt, "ground_bunny")
    o = ds.render(g.params(64, 40, L, flags=IN_FLIGHT))
    assert ds.pipeline == FUSED
    assert (o["hit_id"] >= 0).any()
    tiny = ds.render(g.params(64, 40, L, flags=V_FUSED_HALF_TINY << 8))
    assert ds.pipeline == FUSED
    same_bits(tiny, o, f"ground_bunny 64x40 L{L}, variant 14 against the shipped frame")


def test_batch_and_single_render_of_a_frame_agree(srt):
    """The batch call keeps the four-wave kernel (k_trace_nq_batch): two frames (two light positions) of one half of cube_ground at
    64 x 40 in ONE srt_render_device_batch call against the same two frames rendered one by one."""
    L_ = srt.load()
    g, ds = device_scene(srt, "cube_ground")
    W, H = 64, 40
    params, lights = [], []
    for k in range(2):
        light = g.light.copy(); light[0] += 40.0 * k
        lights.append(light)
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
            for what, flags in (("a frame alone", 0), ("frames in flight", IN_FLIGHT)):
                one = ds.render(abi.make_params(W, H, abi.light_staircase(lights[k], 4), block_rows=8, block_first=0, block_stride=2, flags=flags))
                assert ds.pipeline == FUSED
                assert (one["hit_id"] >= 0).any()
                same_bits(f.out(), one, f"frame {k} of the batch against the single render, {what}")
    finally:
        for f in frames:
            f.free()
        for h in handles:
            h.close()
