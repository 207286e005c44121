"""The half-tile trace kernel built for eight waves per SIMD (k_trace_nq_half8 and k_trace_nq_half8_spans, srt_kernels.h: the half-tile body
without packed f32 operations, 384 node-queue entries a wave), which plan_frame ships for frames in flight.  The same rays, merged the same
way, so every output has the bits of the other builds: the shipped choice with SRT_FLAG_FRAMES_IN_FLIGHT (eight waves, 384 entries) and
variant 66 (eight waves, 256 entries) against variant 59 -- four waves of 4x4 pixels per tile on the full grid -- and against variant 65,
the seven-wave build with its 512 entries, in hit_id, t, rgb_linear and rgb8, and once more on the pixels a shadow ray decides (those
whose colour changes when a shadowed sample counts in full, shadow_div = 1).  Against the oracle at the bars of tests/test_gpu_parity.py.

Scenes by how a half-tile wave gets its roots, as tests/test_gpu_trace_half_seven.py (its scenes, views and oracle frames are shared):
  cubes4_a40   4 objects: root masks, ONE root group (six objects at a time with 384 entries)
  soup12       12 objects: the roots are queued from the masks in two groups of six (three groups of four with 256 entries)
  soup40       40 objects: no root masks, every wave tests the roots itself.  The shipped choice renders this soup with the packet kernels, so
               0, 59, 65 and 66 never reach a trace kernel here: the builds are forced instead, as tests/test_gpu_trace_half_seven.py does --
               variant 30 (eight waves) against 11 (four waves per tile) and 13 (seven waves)
  grid40       tests/half_eight_scenes.py: forty small squares side by side, boxes that overlap little -- no root masks either, and the shipped
               choice does take the trace kernel and its tile spans: 0, 66 and 30 against 59 and 65
  fans         tests/half_eight_scenes.py: six stacked squares of 32 triangles each, 7 nodes an object, 42 in the scene, and every ray
               of the 16 x 16 frame passes every one.  A wave queues 2 x 32 x 6 = 384 root children, its first pop of 64 asks for 128
               more -- 320 + 128 = 448 > 384 -- and the stackless walk finishes the subtrees in the closest-hit phase; the seven-wave
               build's 512 entries hold the 448 (tests/test_trace_half_eight_queue.py counts this on the host mirror's tree)
Shapes: 37 x 29 (tiles cut on both edges) and 64 x 40 (whole tiles); 1 and 4 light samples.  Eager here; captured into a graph, replayed,
and replayed after srt_scene_update in tests/trace_half_eight_graph_case.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import half_eight_scenes as he
import test_gpu_trace_half_seven as seven
from simple_raytracer_amd import abi
from test_gpu_parity import bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
V_FUSED_5_WAVES = 11        # four waves per tile, forced whatever the scene prefers
V_FUSED_HALF = 13           # the half-tile form's seven-wave build, forced
V_FUSED_HALF_TINY = 14      # the half-tile form with a 160-entry queue
V_FUSED_HALF_8_WAVES = 30   # the half-tile form's eight-wave build, forced
V_FOUR_WAVES = 59           # four waves per tile where the half-tile form would run
V_SEVEN_WAVES = 65          # the half-tile form's seven-wave build, 512 entries
V_EIGHT_WAVES_256 = 66      # the eight-wave build with 256 entries

srt = seven.srt


def with_shadow_div(p, div):
    q = abi.Params.from_buffer_copy(p)
    q._lights = p._lights
    q.shadow_div = div
    return q


def check_builds(srt, oracle, name, ds, flat, params, W, H, L, shadows_expected, four_waves=V_FOUR_WAVES, seven_waves_v=V_SEVEN_WAVES,
                 eight_waves=(0, V_EIGHT_WAVES_256, V_FUSED_HALF_8_WAVES)):
    c = seven.oracle_frame(oracle, name, flat, params(W, H, L), W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    four = ds.render(params(W, H, L, flags=IN_FLIGHT | four_waves << 8))
    assert ds.pipeline == seven.FUSED
    # the pixels a shadow ray decides: with shadow_div = 1 a shadowed sample counts like a lit one
    flat_lit = ds.render(with_shadow_div(params(W, H, L, flags=IN_FLIGHT | four_waves << 8), 1.0))
    shadowed = (bits(four["rgb_linear"]) != bits(flat_lit["rgb_linear"])).any(-1)
    assert not shadows_expected or (shadowed.any() and not shadowed.all()), f"{name}: {int(shadowed.sum())} of {shadowed.size} pixels depend on a shadow ray"
    seven_waves = ds.render(params(W, H, L, flags=IN_FLIGHT | seven_waves_v << 8))
    assert ds.pipeline == seven.FUSED
    seven.same_bits(seven_waves, four, f"{name} {W}x{H} L{L}, the seven-wave build against four waves per tile")
    for v in eight_waves:
        p = params(W, H, L, flags=IN_FLIGHT | v << 8)
        o = ds.render(p)
        assert ds.pipeline == seven.FUSED
        for other, what in ((four, f"variant {four_waves}"), (seven_waves, "the seven-wave build")):
            seven.same_bits(o, other, f"{name} {W}x{H} L{L}, variant {v} against {what}")
            assert np.array_equal(bits(o["rgb_linear"][shadowed]), bits(other["rgb_linear"][shadowed])) and np.array_equal(o["rgb8"][shadowed], other["rgb8"][shadowed]), \
                f"{name} {W}x{H} L{L}, variant {v} against {what}: shadow-dependent pixels"
        if v == eight_waves[0]:      # (the other builds' frames have these bits)
            seven.at_the_oracles_bars(srt, oracle, o, c, flat, params(W, H, L), f"{name} {W}x{H} L{L}, the shipped eight-wave build")


@pytest.mark.parametrize("L", seven.LIGHTS)
@pytest.mark.parametrize("W,H", seven.SHAPES)
@pytest.mark.parametrize("name", ["cubes4_a40", "soup12", "soup40"])
def test_eight_wave_builds_match_four_waves_seven_waves_and_the_oracle(srt, oracle, name, W, H, L):
    flat, params, ds = seven.scene(srt, name)
    if name == "soup40":
        check_builds(srt, oracle, name, ds, flat, params, W, H, L, False, V_FUSED_5_WAVES, V_FUSED_HALF, (V_FUSED_HALF_8_WAVES,))
    else:
        check_builds(srt, oracle, name, ds, flat, params, W, H, L, shadows_expected=name == "cubes4_a40")


@pytest.fixture(scope="module")
def grid40(srt):
    flat, _ = he.grid40_scene()
    ds = srt.DeviceScene(flat)
    yield flat, ds
    ds.close()


@pytest.mark.parametrize("L", seven.LIGHTS)
@pytest.mark.parametrize("W,H", seven.SHAPES)
def test_forty_objects_without_root_masks_through_the_shipped_choice(srt, oracle, grid40, W, H, L):
    flat, ds = grid40
    check_builds(srt, oracle, "grid40", ds, flat, he.grid40_params, W, H, L, shadows_expected=True)
    c = seven.oracle_frame(oracle, "grid40", flat, he.grid40_params(W, H, L), W, H, L)
    assert len(np.unique(flat.tri_obj[c["hit_id"][c["hit_id"] >= 0]])) == 40 and (c["hit_id"] < 0).any(), "every object is seen, and some background"


@pytest.fixture(scope="module")
def fans(srt):
    flat, _ = he.flat_scene()
    ds = srt.DeviceScene(flat)
    yield flat, ds
    ds.close()


@pytest.mark.parametrize("L", seven.LIGHTS)
def test_a_queue_of_384_entries_overflows_in_the_closest_hit_phase(srt, oracle, fans, L):
    """42 nodes, every one passed by every ray: 384 root children queued, 448 entries wanted at the first pop (docstring above).  Variant
    14's 160 entries overflow as well, the seven-wave build's 512 do not: the frames are the same."""
    flat, ds = fans
    check_builds(srt, oracle, "fans", ds, flat, lambda W, H, L, flags=0: he.params(L, flags), he.W, he.H, L, shadows_expected=True,
                 eight_waves=(0, V_EIGHT_WAVES_256, V_FUSED_HALF_8_WAVES, V_FUSED_HALF_TINY))
    c = seven.oracle_frame(oracle, "fans", flat, he.params(L), he.W, he.H, L)
    assert (c["hit_id"] >= 0).all(), "every ray hits: every wave of the frame walks all six objects"


def test_captured_frames_replay_and_follow_the_scene():
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py): eager, captured, replayed and replayed after
    srt_scene_update, through the spans kernels of the eight-wave and the seven-wave builds."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "trace_half_eight_graph_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "trace half eight graph case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
