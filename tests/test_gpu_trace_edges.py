"""GPU (-m gpu): the trace kernels of frames in flight at the edges of their index arithmetic -- the shapes, views and scenes of
tests/edge_frames.py, whose properties tests/test_edge_frames_ref.py pins on the CPU.

Every frame is rendered through gpu_frames.render_pinned: sentinel-filled pinned buffers with a guard row, so a store outside the frame
fails the case.  Per (scene, shape) and 1, 4, 5 and 7 light samples, eight builds:

    IN_FLIGHT                the whole-frame kernels (k_trace_nq_whole8_spans, k_shade_tile_whole_spans) at 1 and 4; two waves a tile at 5 and 7
    IN_FLIGHT, variant 68    k_trace_nq_wave8_spans, the general frame's one-wave workgroups
    IN_FLIGHT, variant 32    ... in the adjacent dispatch order
    IN_FLIGHT, variant 67    k_trace_nq_half8_spans, two waves a tile
    variant 31               the one-wave workgroups without the hint, at every sample count
    0                        four waves of 4x4 pixels per tile, over the spans
    IN_FLIGHT, variant 64    the shipped kernels on the full grid, no table
    IN_FLIGHT, variant 59    four waves per tile on the full grid

every one the fused pipeline, every frame with the bits of the variant-64 frame in hit_id, t, rgb_linear and rgb8 and its hit_rays
(tests/test_gpu_tile_spans.py's bar), and the IN_FLIGHT and variant-68 frames the oracle's with the device's pow (gpu_frames.compare_exact).
The captured launches -- the whole padded grid, the table from tile row 0, the epoch word -- in tests/trace_edges_graph_case.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edge_frames as ef
import golden_util as gu
import gpu_frames as gf
from test_gpu_tile_spans import same_bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FUSED = "k_trace_nq+k_shade_tile"
IN_FLIGHT = ef.IN_FLIGHT
V_FULL_GRID, V_GENERAL = 64, 68
FULL = IN_FLIGHT | V_FULL_GRID << 8
BUILDS = [(IN_FLIGHT, "the hint"), (IN_FLIGHT | V_GENERAL << 8, "variant 68"), (IN_FLIGHT | 32 << 8, "variant 32"), (IN_FLIGHT | 67 << 8, "variant 67"),
          (31 << 8, "variant 31"), (0, "four waves"), (IN_FLIGHT | 59 << 8, "variant 59")]
AT_THE_ORACLE = (IN_FLIGHT, IN_FLIGHT | V_GENERAL << 8)

_oracle_frames = {}


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def held(srt):
    """key -> (flat scene, device scene), built once: a golden scene's name, "offset", or an object count."""
    scenes = {}
    def get(key):
        if key not in scenes:
            flat = ef.offset_scene()[0] if key == "offset" else ef.object_grid(key)[0] if isinstance(key, int) else gu.GoldenScene(key).flat
            scenes[key] = (flat, srt.DeviceScene(flat))
        return scenes[key]
    yield get
    for _, ds in scenes.values():
        ds.close()


def oracle_frame(oracle, key, flat, p, W, H, L):
    """The oracle's frame with the device's pow, computed once per (scene, shape, L) and left unchanged."""
    k = (key, W, H, L)
    if k not in _oracle_frames:
        c = oracle.render(flat, p, pow="device")
        for name in ("hit_id", "t", "rgb_linear", "rgb8"):
            c[name].setflags(write=False)
        _oracle_frames[k] = c
    return _oracle_frames[k]


def check_case(srt, oracle, key, flat, ds, view, W, H, lights=ef.LIGHTS):
    """Every build of the frame against the full grid's, two of them against the oracle; returns {L: the hinted frame}."""
    out = {}
    for L in lights:
        what = f"{key} {W}x{H} L{L}"
        full, pipe = gf.render_pinned(srt, ds, view(L, FULL))
        assert pipe == FUSED, (what, pipe)
        for flags, name in BUILDS:
            p = view(L, flags)
            o, pipe = gf.render_pinned(srt, ds, p)
            assert pipe == FUSED, (what, name, pipe)
            same_bits(o, full, f"{what}, {name} against the full grid")
            if flags in AT_THE_ORACLE:
                gf.compare_exact(srt, o, oracle_frame(oracle, key, flat, p, W, H, L), gf.owned(p), flat, p, f"{what}, {name}")
            if flags == IN_FLIGHT:
                out[L] = o
    return out


@pytest.mark.parametrize("W,H", ef.SHAPES)
@pytest.mark.parametrize("name", ef.GOLDEN)
def test_golden_scenes_at_every_edge_shape(srt, oracle, held, name, W, H):
    flat, ds = held(name)
    o = check_case(srt, oracle, name, flat, ds, ef.edge_view(name, W, H), W, H)
    assert (o[1]["hit_id"] >= 0).any() or (name, (W, H)) in ef.NO_HIT_POSSIBLE


@pytest.mark.parametrize("W,H", ef.OFFSET_SHAPES)
def test_a_span_that_starts_inside_a_group_of_eight_and_ends_in_the_next(srt, oracle, held, W, H):
    flat, ds = held("offset")
    o = check_case(srt, oracle, "offset", flat, ds, ef.offset_view(W, H), W, H)
    x0, n = ef.OFFSET_SPANS[(W, H)]
    cols = np.flatnonzero((o[1]["hit_id"] >= 0).any(axis=0))
    assert cols.min() // 8 == x0 and cols.max() // 8 == x0 + n - 1, "hits in the first and in the last tile of the span"


@pytest.mark.parametrize("W,H", ef.GRID_SHAPES)
@pytest.mark.parametrize("n", ef.OBJECT_COUNTS)
def test_object_counts_on_both_sides_of_every_bound(srt, oracle, held, n, W, H):
    flat, ds = held(n)
    view = ef.grid_view(n, W, H)
    o = check_case(srt, oracle, f"grid{n}", flat, ds, view, W, H)
    seen = np.unique(flat.tri_obj[o[1]["hit_id"][o[1]["hit_id"] >= 0]])
    assert list(seen) == list(range(n)), f"objects seen: {seen}"
    if n > 1:      # the pixels whose shadow ray the last object stops: the oracle's bits, in every build (they all have the hinted frame's)
        c = oracle_frame(oracle, f"grid{n}", flat, view(1), W, H, 1)
        by_last = ef.shadowed_by_last(oracle, n, W, H, c)
        assert by_last.any()
        assert np.array_equal(o[1]["hit_id"][by_last], c["hit_id"][by_last])
        assert gf.int_shininess_only(flat), "compare_exact has asked for rgb_linear bit for bit"
        assert np.array_equal(gf.bits(o[1]["rgb_linear"][by_last]), gf.bits(c["rgb_linear"][by_last])) and np.array_equal(o[1]["rgb8"][by_last], c["rgb8"][by_last]), \
            "the pixels the last object shadows"
        lit, _ = gf.render_pinned(srt, ds, _with_shadow_div(view(1, IN_FLIGHT), 1.0))
        assert (gf.bits(lit["rgb_linear"][by_last]) != gf.bits(o[1]["rgb_linear"][by_last])).any(-1).all(), "... depend on their shadow ray on the device too"


def _with_shadow_div(p, div):
    q = type(p).from_buffer_copy(p)
    q._lights = p._lights
    q.shadow_div = div
    return q


def test_one_handle_through_the_edges(srt, oracle):
    """One device scene, a frame of one pixel, then the widest, then a small one, then nine tiles across: the workspaces only grow, and
    the shadow words of the larger frame are still there when the smaller one is traced."""
    name = "cube_ground"
    flat = gu.GoldenScene(name).flat
    ds = srt.DeviceScene(flat)
    try:
        for (W, H) in ((1, 1), (129, 9), (9, 3), (65, 12)):
            p = ef.edge_view(name, W, H)(1, IN_FLIGHT)
            o, pipe = gf.render_pinned(srt, ds, p)
            assert pipe == FUSED
            gf.compare_exact(srt, o, oracle_frame(oracle, name, flat, p, W, H, 1), gf.owned(p), flat, p, f"{name} {W}x{H} on a handle that has rendered other sizes")
    finally:
        ds.close()


@pytest.mark.parametrize("scene", ["cubes4_a40", "grid32", "grid33"])
def test_captured_frames_at_the_edges_replay_and_follow_the_scene(scene):
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py), one per scene; it stops at its first failure."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "trace_edges_graph_case.py"), scene], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and f"trace edges graph case {scene}: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
