"""The half-tile trace kernel with the closest-hit phase's dir[] and best[] laid over the shadow phase's LDS (HalfTileLds, srt_kernels.h):
what tests/test_gpu_trace_half_tile.py (two-object ground scenes) does not reach and the overlay or the half-tile body can get wrong.
Variant 13 (the build plan_frame ships for frames in flight) and variant 19 (the six-wave build of the same body) against variant 11,
the four-wave fused kernel forced whatever the scene prefers, bit for bit -- a ray whose direction or best key were overwritten by the
shadow phase's rays, or a root mask by the closest-hit phase, changes a hit id, a t or a shadow bit -- and against the oracle at the bars
of tests/test_gpu_parity.py.  Scenes by how a half-tile wave gets its roots:
  3 .. 8 objects     cubes4_a40: root masks with several bits, the union-box test, ONE root group at 32 rays per wave
  9 .. 32 objects    a 12-object soup: the roots are queued from the masks in two groups of eight (512 / 64 = 8 at 32 rays per wave)
  more than 32       the 40-object soup of test_gpu_parity's many-objects test (one empty and one one-triangle object): there are no root
                     masks, every half-tile wave tests the roots itself, in five groups
and variants 15 (1024-entry queue) and 16 (32 shadow rays in flight: ShadowLds<32, 32>) on ground_bunny, which take the overlay too.
Shapes: 37 x 29 (tiles cut on both edges) and 64 x 40 (whole tiles); 1 and 4 light samples (4: a wave's masks hold several samples)."""
import numpy as np
import pytest

import golden_util as gu
from simple_raytracer_amd import abi
from test_gpu_parity import TOL_LINEAR, bits, check_rgb8, strict

pytestmark = pytest.mark.gpu

FUSED = "k_trace_nq+k_shade_tile"
V_FUSED_5_WAVES = 11        # the four-wave fused kernel, forced
V_FUSED_HALF = 13           # the half-tile form as shipped for frames in flight, forced
V_FUSED_HALF_1024 = 15      # ... with a 1024-entry node queue
V_FUSED_HALF_32_RAYS = 16   # ... with 32 shadow rays in flight per wave
V_FUSED_HALF_6_WAVES = 19   # ... built for six waves per SIMD
OUTPUTS = ("hit_id", "t", "rgb_linear", "rgb8")
SHAPES = [(37, 29), (64, 40)]
LIGHTS = [1, 4]


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def soup12():
    import scenes
    from simple_raytracer_amd import host
    recipe, meshes = scenes.soup(600, n_objects=12)
    flat = host.build_flat_scene(recipe, meshes)
    assert flat.n_objects == 12
    return flat, recipe.light


def soup40():
    """The scene of test_gpu_parity.test_many_objects_empty_objects_and_no_lights."""
    import scenes
    from simple_raytracer_amd import host
    recipe, meshes = scenes.soup(4000, n_objects=38)
    meshes["none"] = np.zeros((0, 3, 4), np.float32)
    meshes["one"] = np.array([[[-30, -30, 200, 1], [30, -30, 200, 1], [0, 40, 210, 1]]], np.float32)
    recipe.load("empty.obj", "none"); recipe.bvh("empty.obj")
    recipe.load("single.obj", "one"); recipe.color("single.obj", (0.2, 0.9, 0.9)); recipe.bvh("single.obj")
    flat = host.build_flat_scene(recipe, meshes)
    assert flat.n_objects == 40
    return flat, recipe.light


def focal(name, W, H):
    """The focal length is in pixels, so a small frame at the reference's 400 is a narrow cone down the z axis, which misses the cubes
    and the sparse soup: each scene keeps the view of a frame of the width it is rendered at elsewhere, scaled to W.  The 12-object soup
    is 600 triangles of ~8 units over 4000 x 4000 x 1000 -- about one hit pixel per thousand whatever the view (every ray still passes
    all twelve root boxes, which is what the case is for) -- so its two views are wide ones in which the oracle has hits on three
    objects."""
    if name == "soup12":
        return {(37, 29): 9.25, (64, 40): 8.0}[(W, H)]
    return 400.0 * W / {"cubes4_a40": 150, "soup40": 203, "ground_bunny": 400}[name]


_scenes = {}
_oracle_frames = {}


def scene(srt, name):
    """name -> (flat scene, params(W, H, L, flags), device scene), built once."""
    if name not in _scenes:
        if name in ("soup12", "soup40"):
            flat, light = soup12() if name == "soup12" else soup40()
        else:
            g = gu.GoldenScene(name)
            flat, light = g.flat, g.light
        params = lambda W, H, L, flags=0: abi.make_params(W, H, abi.light_staircase(light, L), focal=focal(name, W, H), flags=flags)
        _scenes[name] = (flat, params, srt.DeviceScene(flat))
    return _scenes[name]


def oracle_frame(oracle, name, flat, p, W, H, L):
    """The oracle's frame, computed once per scene and shape and left unchanged."""
    key = (name, W, H, L)
    if key not in _oracle_frames:
        c = oracle.render(flat, p)
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


def a_tile_with_hits_in_both_halves(hit_id):
    """Some 8x8 tile has hit pixels in rows 0..3 and in rows 4..7: both waves of its workgroup pass through both phases."""
    hit = np.asarray(hit_id) >= 0
    H, W = hit.shape
    padded = np.zeros(((H + 7) // 8 * 8, (W + 7) // 8 * 8), bool)
    padded[:H, :W] = hit
    halves = padded.reshape(padded.shape[0] // 8, 2, 4, padded.shape[1] // 8, 8).any(axis=(2, 4))      # (tile row, half, tile column)
    return bool((halves[:, 0] & halves[:, 1]).any())


def check_variants(srt, oracle, name, W, H, L, variants):
    flat, params, ds = scene(srt, name)
    p = params(W, H, L)
    c = oracle_frame(oracle, name, flat, p, W, H, L)
    assert (c["hit_id"] >= 0).any(), "the shape must put hit pixels (and their shadow rays) through the kernel"
    if name in ("ground_bunny", "cubes4_a40"):
        assert a_tile_with_hits_in_both_halves(c["hit_id"])
    four = ds.render(params(W, H, L, flags=V_FUSED_5_WAVES << 8))
    assert ds.pipeline == FUSED
    for v in variants:
        o = ds.render(params(W, H, L, flags=v << 8))
        assert ds.pipeline == FUSED
        same_bits(o, four, f"{name} {W}x{H} L{L}, variant {v} against variant 11")
        at_the_oracles_bars(srt, oracle, o, c, flat, p, f"{name} {W}x{H} L{L} variant {v}")


@pytest.mark.parametrize("L", LIGHTS)
@pytest.mark.parametrize("W,H", SHAPES)
@pytest.mark.parametrize("name", ["cubes4_a40", "soup12", "soup40"])
def test_overlay_builds_match_the_four_wave_kernel_and_the_oracle(srt, oracle, name, W, H, L):
    check_variants(srt, oracle, name, W, H, L, (V_FUSED_HALF, V_FUSED_HALF_6_WAVES))


@pytest.mark.parametrize("L", LIGHTS)
def test_wide_queue_and_32_ray_builds_take_the_overlay(srt, oracle, L):
    check_variants(srt, oracle, "ground_bunny", 64, 40, L, (V_FUSED_HALF_1024, V_FUSED_HALF_32_RAYS))
