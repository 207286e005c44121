"""The eight-wave trace build over the tile spans as workgroups of ONE wave (k_trace_nq_wave8_spans, srt_kernels.h), which plan_frame ships
for frames in flight: a wave owns half a tile, tests the roots of its own 32 rays and waits for nobody.  The same rays, merged the same way,
so every output has the bits of the other builds: the shipped choice with SRT_FLAG_FRAMES_IN_FLIGHT and variant 31 (the same kernel without
the hint) against variant 67 -- the two-wave workgroups in its place, k_trace_nq_half8_spans -- and variant 59, four waves of 4x4 pixels per
tile on the full grid, and with them variant 32 (a tile's halves next to each other in dispatch order, where the shipped order has them eight workgroups apart), in hit_id, t, rgb_linear and rgb8, and once more on the pixels a shadow ray decides (those whose colour changes when
a shadowed sample counts in full, shadow_div = 1).  Against the oracle at the bars of tests/test_gpu_parity.py.

Scenes by how a wave gets its roots (tests/test_gpu_trace_half_seven.py and tests/half_eight_scenes.py, shared):
  cubes4_a40     4 objects: the wave's own root pass, ONE group (six objects at a time with 384 entries)
  soup12         12 objects: two groups of six
  grid40         40 objects, more than 32: the queue path (every root queued as a node), and the shipped choice takes the trace kernel
  fans           six objects, every ray passes every node: 384 root children queued, 448 wanted at the first pop -- the stackless walk
  ground_bunny, cube_ground   the headline's scenes, two objects: one root pass of 32 rays x 2 objects fills the wave
  ledge          tests/wave8_scenes.py: a strip of tiles inside the spans whose one half holds hits and whose other half passes no root
Shapes: 37 x 29 (tiles cut on both edges), 64 x 40 (whole tiles) and 40 x 36 (rows % 8 == 4: the last tile row's lower halves have no live
pixel and their waves leave at once); 1 and 4 light samples.  Eager here; captured into a graph, replayed, and replayed after srt_scene_update in tests/trace_wave8_graph_case.py."""
import ctypes
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import half_eight_scenes as he
import test_gpu_trace_half_eight as eight
import test_gpu_trace_half_seven as seven
import test_tile_spans as ts
import wave8_scenes as w8
from simple_raytracer_amd import abi, build
from test_gpu_parity import bits

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNEL = "k_trace_nq_wave8_spans<384, true, 16, true>"
WORKGROUPS_PER_CU = 32

srt = seven.srt
cli = ts.cli


def check_builds(srt, oracle, name, ds, flat, params, W, H, L, shadows_expected):
    """The one-wave workgroups (0 under the hint, 31 with and without it, 32: the other dispatch order) against 67, 59 and the oracle;
    returns the oracle's frame."""
    c = seven.oracle_frame(oracle, f"wave8 {name}", flat, params(W, H, L), W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    four = ds.render(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_FOUR_WAVES << 8))
    assert ds.pipeline == seven.FUSED
    # the pixels a shadow ray decides: with shadow_div = 1 a shadowed sample counts like a lit one
    flat_lit = ds.render(eight.with_shadow_div(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_FOUR_WAVES << 8), 1.0))
    shadowed = (bits(four["rgb_linear"]) != bits(flat_lit["rgb_linear"])).any(-1)
    assert not shadows_expected or (shadowed.any() and not shadowed.all()), f"{name}: {int(shadowed.sum())} of {shadowed.size} pixels depend on a shadow ray"
    two = ds.render(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_TWO_WAVES << 8))
    assert ds.pipeline == seven.FUSED
    seven.same_bits(two, four, f"{name} {W}x{H} L{L}, variant 67 against four waves per tile")
    for flags in (w8.IN_FLIGHT, w8.V_WAVE_8 << 8, w8.IN_FLIGHT | w8.V_WAVE_8 << 8, w8.IN_FLIGHT | w8.V_ADJACENT << 8):
        o = ds.render(params(W, H, L, flags=flags))
        assert ds.pipeline == seven.FUSED
        for other, what in ((two, "variant 67"), (four, "variant 59")):
            seven.same_bits(o, other, f"{name} {W}x{H} L{L}, flags {flags:#x} against {what}")
            assert np.array_equal(bits(o["rgb_linear"][shadowed]), bits(other["rgb_linear"][shadowed])) and np.array_equal(o["rgb8"][shadowed], other["rgb8"][shadowed]), \
                f"{name} {W}x{H} L{L}, flags {flags:#x} against {what}: shadow-dependent pixels"
        if not flags & w8.IN_FLIGHT or flags == w8.IN_FLIGHT:      # (0 and 31 each once: the third frame has their bits)
            seven.at_the_oracles_bars(srt, oracle, o, c, flat, params(W, H, L), f"{name} {W}x{H} L{L}, flags {flags:#x}")
    return c


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_a_waves_own_root_pass_in_one_group(srt, oracle, W, H, L):
    flat, params, ds = seven.scene(srt, "cubes4_a40")
    c = check_builds(srt, oracle, "cubes4_a40", ds, flat, params, W, H, L, shadows_expected=True)
    assert seven.a_tile_with_hits_in_both_halves(c["hit_id"])


@pytest.fixture(scope="module")
def soup12(srt):
    flat, light = seven.soup12()
    ds = srt.DeviceScene(flat)
    yield flat, light, ds
    ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_a_waves_own_root_pass_in_two_groups(srt, oracle, soup12, W, H, L):
    """Views as wide as tests/test_gpu_trace_half_seven.py gives this sparse soup (a handful of hit pixels on three objects; every ray
    passes all twelve root boxes, which is what the case is for); 40 x 36 takes the focal length of 37 x 29."""
    flat, light, ds = soup12
    focal = {(37, 29): 9.25, (64, 40): 8.0, (40, 36): 9.25}[(W, H)]
    params = lambda W, H, L, flags=0: abi.make_params(W, H, abi.light_staircase(light, L), focal=focal, flags=flags)
    check_builds(srt, oracle, "soup12", ds, flat, params, W, H, L, shadows_expected=False)


@pytest.fixture(scope="module")
def golden_scenes(srt):
    held = {}
    def get(name):
        if name not in held:
            g = gu.GoldenScene(name)
            held[name] = (g, srt.DeviceScene(g.flat))
        return held[name]
    yield get
    for _, ds in held.values():
        ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
@pytest.mark.parametrize("name", ["ground_bunny", "cube_ground"])
def test_the_headline_scenes_two_objects_fill_a_root_pass(srt, oracle, golden_scenes, name, W, H, L):
    """At a focal length of the frame's width: the slab under the object, sky above it, background beside it."""
    g, ds = golden_scenes(name)
    params = lambda W, H, L, flags=0: g.params(W, H, L, focal=float(W), flags=flags)
    c = check_builds(srt, oracle, name, ds, g.flat, params, W, H, L, shadows_expected=True)
    assert seven.a_tile_with_hits_in_both_halves(c["hit_id"]) and (c["hit_id"] < 0).any()


@pytest.fixture(scope="module")
def grid40(srt):
    flat, _ = he.grid40_scene()
    ds = srt.DeviceScene(flat)
    yield flat, ds
    ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
@pytest.mark.parametrize("W,H", w8.SHAPES)
def test_forty_objects_keep_the_queue_path(srt, oracle, grid40, W, H, L):
    flat, ds = grid40
    c = check_builds(srt, oracle, "grid40", ds, flat, he.grid40_params, W, H, L, shadows_expected=True)
    assert len(np.unique(flat.tri_obj[c["hit_id"][c["hit_id"] >= 0]])) == 40 and (c["hit_id"] < 0).any(), "every object is seen, and some background"


@pytest.fixture(scope="module")
def fans(srt):
    flat, _ = he.flat_scene()
    ds = srt.DeviceScene(flat)
    yield flat, ds
    ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
def test_a_queue_of_384_entries_overflows_behind_the_waves_own_root_pass(srt, oracle, fans, L):
    """42 nodes, every one passed by every ray: the wave's own root pass queues the 384 root children the masks queued, and the first pop
    wants 448 (tests/test_trace_half_eight_queue.py counts this on the host mirror's tree)."""
    flat, ds = fans
    c = check_builds(srt, oracle, "fans", ds, flat, lambda W, H, L, flags=0: he.params(L, flags), he.W, he.H, L, shadows_expected=True)
    assert (c["hit_id"] >= 0).all(), "every ray hits: every wave of the frame walks all six objects"


@pytest.fixture(scope="module")
def ledge(srt):
    flat, _ = w8.ledge_scene()
    ds = srt.DeviceScene(flat)
    yield flat, ds
    ds.close()


@pytest.mark.parametrize("L", w8.LIGHTS)
def test_a_strip_of_half_tiles_inside_the_spans_is_written_by_the_waves_miss_path(srt, oracle, cli, ledge, L):
    """The CPU first: by the table tools/tile_spans_cli.cpp makes, the reference's slab test and the oracle's frame, tile row 3 of the
    ledge has eight tiles inside the spans whose lower half passes no root box while the upper half holds hits, and tile row 0 the same
    with the halves exchanged.  Then the builds."""
    flat, ds = ledge
    W, H = w8.LEDGE_W, w8.LEDGE_H
    c = check_builds(srt, oracle, "ledge", ds, flat, w8.ledge_params, W, H, L, shadows_expected=True)
    (kept,) = ts.run_cases(cli, [(*ts.root_boxes(flat), W, H, w8.LEDGE_FOCAL)])
    assert kept is not None, "the ledge has a span table"
    miss = w8.miss_path_half_tiles(ts, flat, kept, c["hit_id"], W, H, w8.LEDGE_FOCAL)
    assert miss[3, 1, :].all() and miss[0, 0, :].all(), "the strips: lower halves of tile row 3, upper halves of tile row 0"
    assert not miss[3, 0, :].any() and not miss[0, 1, :].any()


def test_thirty_two_workgroups_are_resident_on_a_cu(srt, tmp_path):
    """hipModuleOccupancyMaxActiveBlocksPerMultiprocessor on the library's own code object, through the HIP runtime the library has loaded:
    32 workgroups of 64 threads for the one-wave kernel (64 VGPRs at most and four LDS granules); the two-wave one's figure is printed
    beside it."""
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {r["short"]: r for r in kr.read(build.LIB_HIP, str(tmp_path / "co"), False)}
    hip = ctypes.CDLL(build.LIB_HIP)      # (symbols of the libraries it depends on are found through it: the one HIP runtime of the process)
    for f in ("hipModuleLoad", "hipModuleGetFunction", "hipModuleOccupancyMaxActiveBlocksPerMultiprocessor", "hipModuleUnload"):
        getattr(hip, f).restype = ctypes.c_int
    ds = srt.DeviceScene(he.flat_scene()[0])      # (the device is initialised and current)
    module, fn, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_int(0)
    assert hip.hipModuleLoad(ctypes.byref(module), str(tmp_path / "co" / "k.co").encode()) == 0
    try:
        for kernel, threads, want in ((KERNEL, 64, WORKGROUPS_PER_CU), ("k_trace_nq_half8_spans<384, true, 16>", 128, None)):
            assert hip.hipModuleGetFunction(ctypes.byref(fn), module, rows[kernel]["name"].encode()) == 0, kernel
            assert hip.hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(ctypes.byref(n), fn, ctypes.c_int(threads), ctypes.c_size_t(0)) == 0
            print(f"{kernel}: {n.value} workgroups of {threads} threads per CU")
            assert want is None or n.value == want, f"{kernel}: {n.value} workgroups per CU, not {want}"
    finally:
        hip.hipModuleUnload(module)
        ds.close()


def test_captured_frames_replay_and_follow_the_scene():
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py): eager, captured, replayed and replayed after
    srt_scene_update, through the one-wave workgroups on the whole grid."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "trace_wave8_graph_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "trace wave8 graph case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
