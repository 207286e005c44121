"""CPU: the yardstick of the Fresnel split (tests/fresnel_ref.py) against what it extends, its one formula against Schlick's polynomial in
float64, and the input conditions of every frame case tests/test_gpu_fresnel.py uses.  Under a table with which nothing splits it is
refract_ref.shade_paths bit for bit; F at x = 1 is f0 exactly, F does not increase over x in [0, 1] and agrees with float64 to the five
roundings it contains; every frame case has side rays that hit beside a next segment that hits, side rays that hit beside one that misses,
side rays that miss beside one that hits, and totally reflected hits."""
import numpy as np
import pytest

import fresnel_ref as fr
import refract_ref as rf
import shade_path_ref as sp
import surface_ref as sf
from simple_raytracer_amd import lib

bits = sf.bits
F32 = np.float32


@pytest.mark.parametrize("table", ["negative", "nan", "mirrors_only"])
def test_a_table_under_which_nothing_splits_is_the_refracting_yardstick(oracle, table):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    ior = rf.case_ior(flat)
    f0 = {"negative": np.full(flat.n_objects, -1.0, np.float32), "nan": np.full(flat.n_objects, np.nan, np.float32),
          "mirrors_only": np.where(ior > 0, F32(-0.5), F32(0.04)).astype(np.float32)}[table]      # (f0 >= 0 only where ior does not transmit)
    assert not fr.splits(ior, f0).any()
    segs, _, sides = fr.trace(oracle, flat, rays, lights, rf.DEPTHS[name], ior, f0, bounce_t_min=rf.BOUNCE_T_MIN, colours=rf.case_colours(oracle, name),
                              cands=rf.case_memo(oracle, name), walks=rf.case_trace(oracle, name))
    got = fr.shade_paths_of(oracle, flat, segs, sides, rf.DEPTHS[name], None, refl)
    sp.assert_same(got, rf.case_reference(oracle, name), f"f0 {table}")
    assert (got["side_hit_id"] == -1).all() and np.isposinf(got["side_t"]).all() and not got["side_rgb_linear"].any() and not bits(got["fresnel"]).any()


def test_the_mix_without_a_side_hit_is_the_mirror_mix():
    """The mix on random rows: with no side hit anywhere it is shade_path_ref.mix bit for bit, whatever F says."""
    rng = np.random.default_rng(11)
    depth, n = 4, 500
    hit = np.where(rng.random((depth, n)) < 0.8, 5, -1).astype(np.int32)
    obj = rng.integers(0, 4, (depth, n)).astype(np.int32)
    lin = rng.uniform(0, 300, (depth, n, 3)).astype(np.float32)
    refl = np.float32(sp.REFLECTANCE)
    F = rng.uniform(0, 1, (depth, n)).astype(np.float32)
    got = fr.mix(hit, obj, lin, np.full((depth, n), -1, np.int32), lin, F, refl)
    assert np.array_equal(bits(got), bits(sp.mix(hit, obj, lin, refl)))
    # and a side hit changes it where the path is going
    side = np.where(rng.random((depth, n)) < 0.5, 7, -1).astype(np.int32)
    side[depth - 1] = -1
    assert (bits(fr.mix(hit, obj, lin, side, lin, F, refl)) != bits(got)).any()


def test_the_weight_at_x_1_is_f0_exactly():
    f0 = np.concatenate([np.float32([0.0, 0.04, 1.0, -0.0, 1e-45, 0.5, 0.999]), np.random.default_rng(3).uniform(0, 1, 1000).astype(np.float32)])
    # entering with dv = -1: x = 1;  leaving with k = 1: x = sqrt(1) = 1
    for entering, dv, k in ((True, -1.0, 0.5), (False, -0.3, 1.0)):
        F = fr.schlick(f0, np.full(f0.size, entering), np.full(f0.size, dv, np.float32), np.full(f0.size, k, np.float32))
        assert np.array_equal(bits(F), bits((f0 + F32(0.0)).astype(np.float32)))       # (f0 + (1 - f0) * 0: -0.0 + 0.0 is +0.0)
        assert np.array_equal(F, f0)


def test_the_weight_does_not_increase_and_agrees_with_float64():
    """x over [0, 1] in float32 steps of 2^-12, and every f0 of a grid over [0, 1].  Against float64: F = f0 + (1 - f0) * (1 - x)^5 holds
    five roundings behind m = 1 - x, which is exact here (x is a multiple of 2^-12 in [0, 1]): m2, m4, m5, (1 - f0) * m5 and the sum, each
    at most half an ulp of a value <= 1, that is 2^-25, and carried on through factors <= 1 except m2's error, which m4 doubles: 6 * 2^-25
    bounds the five together with the half ulp of 1 - f0 times m5 <= 1.  The leaving side adds sqrtf's rounding of x, |dF/dx| <= 5: 11 * 2^-25."""
    x = (np.arange(4097, dtype=np.float64) / 4096.0).astype(np.float32)
    for f0 in np.float32([0.0, 0.02, 0.04, 0.2, 0.5, 0.9, 1.0]):
        # entering: x = -dv
        F = fr.schlick(np.full(x.size, f0), np.ones(x.size, bool), -x, np.zeros(x.size, np.float32))
        assert (np.diff(F.astype(np.float64)) <= 0).all(), f"F increases with x at f0 = {f0}"
        want = np.float64(f0) + (1.0 - np.float64(f0)) * (1.0 - x.astype(np.float64)) ** 5
        assert np.abs(F.astype(np.float64) - want).max() <= 6 * 2.0 ** -25, (f0, np.abs(F - want).max())
        assert F[0] == F32(1.0) and F[-1] == f0
    # leaving: x = sqrtf(k); 1 - x rounds too now (half an ulp of a value <= 1, times |dF/dm| <= 5, is inside the 5 * 2^-25 added for x)
    k = np.linspace(0.0, 1.0, 4097).astype(np.float32)
    F = fr.schlick(np.full(k.size, 0.04, np.float32), np.zeros(k.size, bool), np.zeros(k.size, np.float32), k)
    want = 0.04 + (1.0 - np.float64(np.float32(0.04))) * (1.0 - np.sqrt(k.astype(np.float64))) ** 5
    assert np.abs(F.astype(np.float64) - (want - 0.04 + np.float64(np.float32(0.04)))).max() <= 11 * 2.0 ** -25
    assert (np.diff(F.astype(np.float64)) <= 0).all()


def test_schlick_f0():
    assert lib.schlick_f0(1.5) == F32(0.04) and lib.schlick_f0(1.5).dtype == np.float32
    table = np.float32([0.0, 1.5, -2.0, np.nan, 1.0, 2.0])
    got = lib.schlick_f0(table)
    assert np.array_equal(bits(got), bits(fr.schlick_f0(table)))
    assert got[0] == -1 and got[2] == -1 and got[3] == -1 and got[4] == 0 and got[5] == F32(1.0 / 9.0)
    assert np.array_equal(fr.splits(table, got), [False, True, False, False, True, True])


# segment 1 of the cases' walks: (both branches hit, the side ray alone, the next segment alone), as counted when the cases were chosen
COUNTED = {"cubes4_a40": (409, 119, 79), "cube_ground": (209, 84, 514), "ground_bunny": (422, 440, 306)}


@pytest.mark.parametrize("name", list(fr.DEPTHS))
def test_frame_cases_meet_their_input_conditions(oracle, name):
    segs, kinds, sides = fr.case_walks(oracle, name)
    c = fr.condition(segs, kinds, sides)
    print(name, c, [int((k == rf.TIR).sum()) for k in kinds])
    assert (c[1]["both"], c[1]["side_only"], c[1]["next_only"]) == COUNTED[name], (name, c[1])
    # the last segment takes no side ray, and a side ray is only ever taken at a hit
    assert not sides[fr.DEPTHS[name] - 1][0].any() if len(sides) == fr.DEPTHS[name] else True
    for (walked, F, s), seg in zip(sides, segs):
        assert not (walked & (seg.hit < 0)).any() and not F[~walked].any()
    if name == "cubes4_a40":
        assert int((kinds[1] == rf.TIR).sum()) == 145 and c[1]["neither"] == 2, (c[1], int((kinds[1] == rf.TIR).sum()))
