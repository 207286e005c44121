"""The whole-frame form of the one-wave trace kernel and its shading launch (k_trace_nq_whole8_spans, k_shade_tile_whole_spans,
srt_kernels.h), which plan_frame ships for 1 .. 4 light samples under SRT_FLAG_FRAMES_IN_FLIGHT: the general frame's parameters as
constants, one batch of argument loads in front of the set-up, and triangle loops over pairs of named records.  The same rays and the same
tests in the same order, so every output has the bits of variant 68 (the general frame's kernels kept in their place), of variant 59 (four
waves of 4x4 pixels per tile on the full grid) and, at the bars of tests/test_gpu_parity.py, of the oracle -- in hit_id, t, rgb_linear and
rgb8, and once more on the pixels a shadow ray decides.

Scenes: the 2-, 4-, 6-, 12- and 40-object scenes, the overflow scene (fans, which is the 6-object one) and the ledge of
tests/test_gpu_trace_wave8.py, and tests/whole_scenes.py: leaves of 1, 2, 3 and 8 triangles in one batch, and a leaf whose first, or only
whose last, triangle shadows.  37 x 29, 64 x 40 and 40 x 36 (fans and the ledge at the one shape their views are made for); 1 and 4 light
samples.  Eager here; captured, replayed and replayed after srt_scene_update in tests/trace_whole_graph_case.py, with the frames that must
keep their kernels."""
import os
import subprocess
import sys

import numpy as np
import pytest

import half_eight_scenes as he
import test_gpu_trace_half_eight as eight
import test_gpu_trace_half_seven as seven
import test_gpu_trace_wave8 as wave8
import wave8_scenes as w8
import whole_scenes as ws
from simple_raytracer_amd import abi
from test_gpu_parity import bits
from test_gpu_trace_wave8 import fans, golden_scenes, grid40, ledge, soup12      # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

srt = seven.srt


def check_whole(srt, oracle, name, ds, flat, params, W, H, L, shadows_expected):
    """Variant 0 under the hint (the whole-frame kernels) against 68, 59 and the oracle; returns the oracle's frame."""
    c = seven.oracle_frame(oracle, f"whole {name}", flat, params(W, H, L), W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    four = ds.render(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_FOUR_WAVES << 8))
    assert ds.pipeline == seven.FUSED
    flat_lit = ds.render(eight.with_shadow_div(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_FOUR_WAVES << 8), 1.0))
    shadowed = (bits(four["rgb_linear"]) != bits(flat_lit["rgb_linear"])).any(-1)      # the pixels a shadow ray decides
    assert not shadows_expected or (shadowed.any() and not shadowed.all()), f"{name}: {int(shadowed.sum())} of {shadowed.size} pixels depend on a shadow ray"
    general = ds.render(params(W, H, L, flags=w8.IN_FLIGHT | ws.V_GENERAL << 8))
    assert ds.pipeline == seven.FUSED
    o = ds.render(params(W, H, L, flags=w8.IN_FLIGHT))
    assert ds.pipeline == seven.FUSED
    for other, what in ((general, "variant 68"), (four, "variant 59")):
        seven.same_bits(o, other, f"{name} {W}x{H} L{L}, variant 0 against {what}")
        assert np.array_equal(bits(o["rgb_linear"][shadowed]), bits(other["rgb_linear"][shadowed])) and np.array_equal(o["rgb8"][shadowed], other["rgb8"][shadowed]), \
            f"{name} {W}x{H} L{L} against {what}: shadow-dependent pixels"
    seven.at_the_oracles_bars(srt, oracle, o, c, flat, params(W, H, L), f"{name} {W}x{H} L{L}, variant 0")
    return c


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
@pytest.mark.parametrize("name", ["ground_bunny", "cube_ground"])
def test_two_objects(srt, oracle, golden_scenes, name, W, H, L):
    g, ds = golden_scenes(name)
    params = lambda W, H, L, flags=0: g.params(W, H, L, focal=float(W), flags=flags)
    c = check_whole(srt, oracle, name, ds, g.flat, params, W, H, L, shadows_expected=True)
    assert seven.a_tile_with_hits_in_both_halves(c["hit_id"]) and (c["hit_id"] < 0).any()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_four_objects(srt, oracle, W, H, L):
    flat, params, ds = seven.scene(srt, "cubes4_a40")
    check_whole(srt, oracle, "cubes4_a40", ds, flat, params, W, H, L, shadows_expected=True)


@pytest.mark.parametrize("L", w8.LIGHTS)
def test_six_objects_and_the_queue_overflows(srt, oracle, fans, L):
    flat, ds = fans
    c = check_whole(srt, oracle, "fans", ds, flat, lambda W, H, L, flags=0: he.params(L, flags), he.W, he.H, L, shadows_expected=True)
    assert (c["hit_id"] >= 0).all()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_twelve_objects(srt, oracle, soup12, W, H, L):
    flat, light, ds = soup12
    focal = {(37, 29): 9.25, (64, 40): 8.0, (40, 36): 9.25}[(W, H)]
    params = lambda W, H, L, flags=0: abi.make_params(W, H, abi.light_staircase(light, L), focal=focal, flags=flags)
    check_whole(srt, oracle, "soup12", ds, flat, params, W, H, L, shadows_expected=False)


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_forty_objects(srt, oracle, grid40, W, H, L):
    flat, ds = grid40
    check_whole(srt, oracle, "grid40", ds, flat, he.grid40_params, W, H, L, shadows_expected=True)


@pytest.mark.parametrize("L", w8.LIGHTS)
def test_the_ledge(srt, oracle, ledge, L):
    flat, ds = ledge
    check_whole(srt, oracle, "ledge", ds, flat, w8.ledge_params, w8.LEDGE_W, w8.LEDGE_H, L, shadows_expected=True)


@pytest.fixture(scope="module")
def leaf_scenes(srt):
    held = {}
    def get(name):
        if name not in held:
            flat = ws.leaves_scene() if name == "leaves" else ws.blind_scene(0 if name == "blind_first" else 7)
            held[name] = (flat, srt.DeviceScene(flat))
        return held[name]
    yield get
    for _, ds in held.values():
        ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_leaves_of_one_two_three_and_eight_triangles_in_one_batch(srt, oracle, leaf_scenes, W, H, L):
    """Every object is seen, so every count wins somewhere; they overlap, so the pairs of a batch hold different counts."""
    flat, ds = leaf_scenes("leaves")
    c = check_whole(srt, oracle, "leaves", ds, flat, ws.params, W, H, L, shadows_expected=True)
    seen = np.unique(np.asarray(flat.tri_obj)[c["hit_id"][c["hit_id"] >= 0]])
    assert list(seen) == [0, 1, 2, 3, 4], seen


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
@pytest.mark.parametrize("name", ["blind_first", "blind_last"])
def test_the_first_or_only_the_last_triangle_of_a_leaf_shadows(srt, oracle, leaf_scenes, name, W, H, L):
    flat, ds = leaf_scenes(name)
    check_whole(srt, oracle, name, ds, flat, ws.params, W, H, L, shadows_expected=True)


def test_captured_frames_and_the_frames_that_keep_their_kernels():
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py)."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "trace_whole_graph_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "trace whole graph case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
