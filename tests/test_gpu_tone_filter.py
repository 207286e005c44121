"""GPU (-m gpu): the tone map as a filter (quant_tone, simple_raytracer_amd/csrc/srt_device.h).  store_pixel decides a channel's 8-bit
value from an f32 evaluation of 255 * (c / (c + reinhard))^gamma wherever a margin allows and runs the exact functions -- tone1 / quant1 /
pow_like_host, unchanged, what srt_kat_tonemap runs -- where it does not.  The yardstick is srt_kat_tonemap throughout:

  1. sweeps on the device (srt_kat_tone_filter_sweep): every float at the default literals, 1e-4 .. 1e4 at seven other pairs -- no decided
     value differs, no result differs, and the largest deviation of the filter's 255 * tone from the exact one stays below a quarter of
     the margin the filter allowed for it (the margin's safety factor over what is observed: at least 4);
  2. special values (srt_kat_tone_filter): q is srt_kat_tonemap's, the filter's candidate too where it decided, and nothing is decided
     where the filter must not decide;
  3. the filter does decide: at most 2 % of 2^22 sums uniform in [0, 3) are left to the exact functions;
  4. frames: the rgb8 of every pipeline that shades is srt_kat_tonemap of the frame's own rgb_linear followed by the black -> background
     rule, and is the rgb8 of the same frame under variant 63 (every channel by the exact functions).
     (srt_render_ao is not among them: its kernels write ao8, a plain scale of a count, and are byte-identical to the parent's.)"""
import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import ray_query_ref as rq
import shade_query_ref as sq
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu

V_EXACT_TONE = 63
IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
POS_INF_BITS, NEG_ZERO_BITS, NEG_INF_BITS = 0x7F800000, 0x80000000, 0xFF800000
DEFAULTS = (0.5, 1.1)
PAIRS = [(0.5, 2.2), (0.5, 0.45), (1.0, 1.0), (0.25, 2.0), (0.5, 64.0), (2.0, 1.1), (1e-3, 1.1)]


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


# ---- 1. sweeps ---------------------------------------------------------------------------------------------------------------------------
def check_sweep(r, n, what):
    print(what, r, f"undecided share {r['undecided'] / r['values']:.3e}")
    assert r["values"] == n, (what, r)
    assert r["decided_different"] == 0, (what, r)
    assert r["results_different"] == 0, (what, r)
    assert r["max_deviation_over_margin"] <= 0.25, (what, r)      # the shipped margin is at least 4 x what is observed


def test_every_non_negative_float_at_the_default_literals(srt):
    r = srt.kat_tone_filter_sweep(0, POS_INF_BITS, *DEFAULTS)
    check_sweep(r, POS_INF_BITS + 1, "0 .. +inf")
    assert r["undecided"] < r["values"]


def test_every_negative_float_at_the_default_literals(srt):
    r = srt.kat_tone_filter_sweep(NEG_ZERO_BITS, 0xFFFFFFFF, *DEFAULTS)      # -0 .. -inf and the NaNs with the sign bit
    check_sweep(r, 0x80000000, "-0 .. -inf, NaNs")
    # no negative value, -0 included, is the filter's to decide -- but for c in (-reinhard, 0) the sum is positive and log2 c is NaN: nothing
    assert r["undecided"] == r["values"], r


@pytest.mark.parametrize("reinhard,gamma", PAIRS)
def test_one_e_minus_four_to_one_e_four_at_other_literals(srt, reinhard, gamma):
    lo, hi = f32_bits(1e-4), f32_bits(1e4)
    check_sweep(srt.kat_tone_filter_sweep(lo, hi, reinhard, gamma), hi - lo + 1, f"reinhard {reinhard} gamma {gamma}")


# ---- 2. special values -------------------------------------------------------------------------------------------------------------------
def specials(reinhard):
    f = np.float32
    around = lambda x: [np.nextafter(f(x), f(0)), f(x), np.nextafter(f(x), f(np.inf))]
    v = [f(0.0), -f(0.0), np.uint32(1).view(f), np.uint32(0x007FFFFF).view(f), np.uint32(0x00800000).view(f)] + around(1e-30) + around(1e30)
    v += [-f(reinhard), f(-1.0), f(np.nan), f(np.inf), f(-np.inf), np.finfo(f).max, f(1.0), f(0.25), f(3.0)]
    return np.array(v, np.float32)


def against_the_yardstick(srt, lin, reinhard, gamma, what):
    n = lin.size
    pad = np.concatenate([lin, np.zeros((-n) % 3, np.float32)])
    _, want = srt.kat_tonemap(pad, reinhard, gamma)
    want = want.reshape(-1)[:n]
    q, qf, dec = srt.kat_tone_filter(lin, reinhard, gamma)
    bad = np.flatnonzero(q != want)
    assert bad.size == 0, (what, lin[bad][:8], q[bad][:8], want[bad][:8])
    bad = np.flatnonzero(dec & (qf != want))
    assert bad.size == 0, (what, "decided and different", lin[bad][:8], qf[bad][:8], want[bad][:8])
    assert np.all(qf[~dec] == -1)
    return q, dec


def test_specials_at_the_default_literals(srt):
    lin = specials(DEFAULTS[0])
    q, dec = against_the_yardstick(srt, lin, *DEFAULTS, "specials")
    by = lambda x: dec[np.flatnonzero(lin.view(np.uint32) == np.float32(x).view(np.uint32))[0]]
    assert by(0.0) and q[0] == 0                      # +0 with reinhard > 0: certain
    for x in (-0.0, -1.0, -0.5, np.nan, np.inf, -np.inf, np.finfo(np.float32).max, 1e30, np.uint32(1).view(np.float32), np.uint32(0x007FFFFF).view(np.float32)):
        assert not by(x), x
    assert by(1.0) and by(0.25) and by(3.0)           # ordinary sums are the filter's


@pytest.mark.parametrize("reinhard,gamma", [(0.0, 1.1), (0.5, 0.0), (0.5, -1.1), (0.5, 1e4), (0.5, np.nan)])
def test_literals_the_filter_does_not_take(srt, reinhard, gamma):
    """reinhard 0: the quotient is exactly 1 and the value exactly 255 (the clamp).  gamma outside (0, 1e4): outside the filter's range."""
    lin = np.concatenate([specials(0.5), np.random.default_rng(5).uniform(0.0, 3.0, 4096).astype(np.float32)])
    _, dec = against_the_yardstick(srt, lin, reinhard, gamma, f"reinhard {reinhard} gamma {gamma}")
    assert not dec.any(), lin[dec][:8]


# ---- 3. the filter decides ---------------------------------------------------------------------------------------------------------------
def test_ordinary_sums_are_decided(srt):
    lin = np.random.default_rng(20240229).uniform(0.0, 3.0, 1 << 22).astype(np.float32)
    _, dec = against_the_yardstick(srt, lin, *DEFAULTS, "uniform sums")
    share = 1.0 - dec.mean()
    print(f"undecided share of 2^22 uniform sums in [0, 3): {share:.4%}")
    assert share <= 0.02, share


# ---- 4. frames ---------------------------------------------------------------------------------------------------------------------------
_scenes = {}


def device_scene(srt, name):
    if name not in _scenes:
        g = gu.GoldenScene(name)
        _scenes[name] = (g, srt.DeviceScene(g.flat))
    return _scenes[name]


def composed(srt, lin, p):
    """srt_kat_tonemap of a frame's rgb_linear, then black -> background."""
    _, q = srt.kat_tonemap(np.ascontiguousarray(lin, np.float32).reshape(-1, 3), p.reinhard, p.gamma)
    q = q.copy()
    q[np.all(q == 0, axis=1)] = np.int32(tuple(p.background[:3]))
    return q.astype(np.uint8).reshape(lin.shape)


def check_frame(srt, o, p, exact, what):
    assert np.array_equal(o["rgb8"], composed(srt, o["rgb_linear"], p)), f"{what}: rgb8 is not srt_kat_tonemap of the frame's rgb_linear"
    if exact is not None:
        assert np.array_equal(gf.bits(o["rgb_linear"]), gf.bits(exact["rgb_linear"])), f"{what}: rgb_linear differs from variant 63's"
        assert np.array_equal(o["rgb8"], exact["rgb8"]), f"{what}: rgb8 differs from variant 63's"


@pytest.mark.parametrize("L", [1, 4, 16])
@pytest.mark.parametrize("W,H", [(64, 48), (203, 117)])
@pytest.mark.parametrize("name", ["cube_ground", "ground_bunny", "texquad"])
def test_frames_of_every_pipeline_that_shades(srt, name, W, H, L):
    g, ds = device_scene(srt, name)
    exact = ds.render(g.params(W, H, L, flags=V_EXACT_TONE << 8))
    shipped = ds.render(g.params(W, H, L))
    assert (exact["hit_id"] >= 0).any() and np.array_equal(exact["hit_id"], shipped["hit_id"])
    check_frame(srt, exact, g.params(W, H, L), None, f"{name} {W}x{H} L{L}, variant 63")
    for what, flags in (("shipped", 0), ("frames in flight", IN_FLIGHT), ("variant 44", 44 << 8), ("variant 1", 1 << 8), ("variant 28", 28 << 8)):
        p = g.params(W, H, L, flags=flags)
        check_frame(srt, ds.render(p), p, exact, f"{name} {W}x{H} L{L}, {what}")
    # spp = 4: k_resolve tone-maps the mean of the sub-frames
    p4 = g.params(W, H, L, spp=4)
    check_frame(srt, ds.render(p4), p4, ds.render(g.params(W, H, L, spp=4, flags=V_EXACT_TONE << 8)), f"{name} {W}x{H} L{L}, spp 4")
    # a batch of three frames (three light positions) in one call
    L_ = srt.load()
    params = []
    for k in range(3):
        light = g.light.copy(); light[0] += 40.0 * k
        params.append(abi.make_params(W, H, abi.light_staircase(light, L)))
    handles = [ds.share() for _ in params]
    frames = [gf.PinnedFrame(L_, h.rows(q), h.cols(q)) for h, q in zip(handles, params)]
    try:
        srt.FrameBatch(handles, params, *[[f.ptrs[k] for f in frames] for k in range(4)]).render()
        for k, (h, f, q) in enumerate(zip(handles, frames, params)):
            h.sync()
            light = g.light.copy(); light[0] += 40.0 * k
            one = ds.render(abi.make_params(W, H, abi.light_staircase(light, L), flags=V_EXACT_TONE << 8))
            check_frame(srt, f.out(), q, one, f"{name} {W}x{H} L{L}, frame {k} of a batch")
    finally:
        for f in frames:
            f.free()
        for h in handles:
            h.close()


def test_shaded_rays_and_paths(srt):
    """srt_shade_rays and srt_render_paths (mirror depth 2, and the refracting and Fresnel kernels) on cube_ground at 64 x 48."""
    g, ds = device_scene(srt, "cube_ground")
    W, H = 64, 48
    for L in (1, 4):
        lights = abi.light_staircase(g.light, L)
        q = sq.shade_params(lights)
        o = ds.shade_rays(rq.frame_rays(W, H, rq.SHEAR, 120.0), q)
        assert (o["hit_id"] >= 0).any()
        check_frame(srt, o, q, None, f"srt_shade_rays L{L}")
        p = g.params(W, H, L)
        n_obj = ds.flat.n_objects
        half, ior = np.full(n_obj, 0.5, np.float32), np.full(n_obj, 1.5, np.float32)
        for what, kw in (("mirror", {}), ("refract", dict(ior=ior)), ("fresnel", dict(ior=ior, fresnel=srt.schlick_f0(ior)))):
            o = ds.render_paths(p, 2, half, 1e-3, want=("rgb_linear", "rgb8", "seg_hit_id"), **kw)
            assert (o["seg_hit_id"][0] >= 0).any()
            check_frame(srt, o, p, None, f"srt_render_paths {what} L{L}")
