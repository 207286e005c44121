"""CPU: the yardstick of mirror paths (tests/shade_path_ref.py) against the yardsticks it is made of.  Depth 1 is shade_range_ref.shade bit
for bit; the rows at depth D are the first D rows at a larger depth; the float32 mix agrees with a float64 evaluation within float32
rounding; and every frame case of tests/test_gpu_shade_paths.py meets its input condition on the yardstick alone."""
import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import shade_path_ref as sp
import shade_query_ref as sq
import shade_range_ref as sr
import surface_ref as sf

bits = sf.bits


@pytest.fixture(scope="module")
def small(oracle):
    """cubes4_a40's frame case thinned to every 7th ray, at depth 3 and depth 2."""
    flat, rays, lights, refl = sp.frame_case("cubes4_a40")
    rays = np.ascontiguousarray(rays[::7])
    return flat, rays, lights, refl, sp.shade_paths(oracle, flat, rays, lights, 3, refl, sp.BOUNCE_T_MIN)


def test_depth_1_is_the_shaded_query(oracle, small):
    flat, rays, lights, refl, _ = small
    tr = np.tile(np.float32([0.5, 400.0]), (rays.shape[0], 1))
    for t_range in (None, tr):
        hit, t, lin, rgb8 = sr.shade(oracle, flat, rays, lights, t_range=t_range)
        o = sp.shade_paths(oracle, flat, rays, lights, 1, refl, sp.BOUNCE_T_MIN, t_range=t_range)
        assert np.array_equal(o["seg_hit_id"][0], hit) and np.array_equal(bits(o["seg_t"][0]), bits(t))
        assert np.array_equal(bits(o["seg_rgb_linear"][0]), bits(lin)) and np.array_equal(bits(o["rgb_linear"]), bits(lin)) and np.array_equal(o["rgb8"], rgb8)
        assert np.array_equal(bits(o["seg_rays"][0]), bits(rays))
        assert np.array_equal(o["seg_obj"][0], np.where(hit >= 0, flat.tri_obj[np.maximum(hit, 0)], -1))


def test_prefix_property(oracle, small):
    flat, rays, lights, refl, deep = small
    two = sp.shade_paths(oracle, flat, rays, lights, 2, refl, sp.BOUNCE_T_MIN)
    sp.assert_same(two, {k: deep[k][:2] for k in sp.SEG_KEYS}, "depth 2 of depth 3", sp.SEG_KEYS)
    assert (deep["seg_hit_id"][1] >= 0).any() and np.any(bits(two["rgb_linear"]) != bits(deep["seg_rgb_linear"][0]))


def test_the_mix_against_float64(small):
    *_, refl, ref = small
    want = sp.mix(ref["seg_hit_id"], ref["seg_obj"], ref["seg_rgb_linear"], refl, dtype=np.float64)
    # depth terms, each a product of at most depth + 1 rounded factors and one rounded add: (2 * depth + 2) * depth half-ulps of the largest sum
    depth = ref["seg_hit_id"].shape[0]
    tol = (2 * depth + 2) * depth * 2.0 ** -24 * float(np.abs(ref["seg_rgb_linear"]).max())
    assert np.abs(ref["rgb_linear"].astype(np.float64) - want).max() <= tol
    # a NULL table and a zero table: segment 0 alone
    for table in (None, np.zeros_like(refl)):
        assert np.array_equal(bits(sp.mix(ref["seg_hit_id"], ref["seg_obj"], ref["seg_rgb_linear"], table)), bits(ref["seg_rgb_linear"][0]))


@pytest.mark.parametrize("name", list(sp.FRAMES))
def test_frame_cases_meet_their_input_condition(oracle, name):
    sp.condition(sp.frame_reference(oracle, name))
