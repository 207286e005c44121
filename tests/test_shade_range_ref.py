"""CPU-only: the yardstick of the shaded query with a t interval (tests/shade_range_ref.py) holds on the oracle itself.  With no
interval, and with each of the four identity intervals, the composition -- winner from ray_range_ref, one single-triangle 1 x 1 frame per
(hit, light), shadow bits from ray_range_ref.occluded, the float32 sum, oracle.tonemap -- equals shade_query_ref.oracle_shade, the
oracle's full-scene 1 x 1 frame, bit for bit in hit id, t, rgb_linear and rgb8.  It passes without srt_shade_rays_range: it is what the
GPU tests of that call compare against."""
import dataclasses
import functools

import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import shade_query_ref as sq
import shade_range_ref as sr
from shade_range_ref import look_at
from simple_raytracer_amd import abi

INF, NAN = np.float32(np.inf), np.float32(np.nan)
IDENTITIES = {"NULL": None, "(0, inf)": (0.0, INF), "(-inf, inf)": (-INF, INF), "(NaN, NaN)": (NAN, NAN)}
W, H = 8, 6                       # 48 rays a case


def with_shininess(flat, sh):
    m = flat.obj_material.reshape(-1, 3).copy()
    m[:, 2] = sh
    return dataclasses.replace(flat, obj_material=m)


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (flat scene, flags, rays, light): cameras chosen so that the 48 rays hold hits, misses, hits with sample 0 in shadow and
    lit hits (asserted below)."""
    F = abi.SRT_FLAG_SMOOTH_NORMALS
    if name.startswith("cube_ground"):
        g = gu.GoldenScene("cube_ground")
        flat = {"cube_ground": g.flat, "cube_ground sh 15": with_shininess(g.flat, 15.0), "cube_ground sh 7.5": with_shininess(g.flat, 7.5)}[name]
        return flat, 0, rq.frame_rays(W, H, look_at((-600.0, -250.0, 120.0), (-80.0, 105.0, 390.0)), 7.0), g.light
    if name == "cubes4_a40":
        g = gu.GoldenScene(name)
        return g.flat, 0, rq.frame_rays(W, H, rq.SHEAR, rq.FOCAL[name] * W / rq.FRAME_W), rq.SHADOW_LIGHT[name]
    g = gu.GoldenScene("texquad")
    flags = F if name == "texquad smooth" else 0
    return sq.texquad_with_normals(g), flags, rq.frame_rays(W, H, rq.SHEAR, rq.FOCAL["texquad"] * W / rq.FRAME_W), g.light


CASES = ("cube_ground", "cubes4_a40", "texquad flat", "texquad smooth", "cube_ground sh 15", "cube_ground sh 7.5")


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), (what, "hit ids")
    assert np.array_equal(sq.bits(a[1]), sq.bits(b[1])), (what, "t")
    assert np.array_equal(sq.bits(a[2]), sq.bits(b[2])), (what, "rgb_linear")
    assert np.array_equal(a[3], b[3]), (what, "rgb8")


@pytest.mark.parametrize("n_lights", [1, 4])
@pytest.mark.parametrize("name", CASES)
def test_composition_is_the_full_scene_frame(oracle, name, n_lights):
    flat, flags, rays, light = case(name)
    n = rays.shape[0]
    lights = abi.light_staircase(np.asarray(light, np.float32), n_lights)
    want = sq.oracle_shade(oracle, flat, rays, lights, flags=flags)
    hit = want[0]
    in_shadow, lit = sq.shadow_share(oracle, flat, rays[hit >= 0], lights[0])
    print(name, n_lights, "hits", int((hit >= 0).sum()), "of", n, "sample 0 in shadow", int(in_shadow.sum()), "lit", int(lit.sum()))
    assert 0 < (hit >= 0).sum() < n and in_shadow.any() and lit.any()
    if name.startswith("texquad"):
        assert (flat.tri_tex[hit[hit >= 0]] >= 0).any()
    for what, pair in IDENTITIES.items():
        tr = None if pair is None else np.tile(np.array(pair, np.float32), (n, 1))
        same(sr.shade(oracle, flat, rays, lights, t_range=tr, flags=flags), want, f"{name} {n_lights} lights {what}")
    # the identities hold ray by ray: all of them in one batch
    tr = np.array([p for p in IDENTITIES.values() if p is not None], np.float32)[np.arange(n) % 3]
    same(sr.shade(oracle, flat, rays, lights, t_range=tr, flags=flags), want, f"{name} mixed identities")


def test_other_literals(oracle):
    flat, flags, rays, light = case("cube_ground")
    lights = abi.light_staircase(np.asarray(light, np.float32), 4)
    want = sq.oracle_shade(oracle, flat, rays, lights, **sq.OTHER_LITERALS)
    assert not np.array_equal(want[3], sq.oracle_shade(oracle, flat, rays, lights)[3])
    same(sr.shade(oracle, flat, rays, lights, **sq.OTHER_LITERALS), want, "other literals")


def test_shininess_cases_differ(oracle):
    """The two shininess scenes are two scenes: the non-integer exponent reaches the oracle's pow."""
    lights = abi.light_staircase(np.asarray(case("cube_ground")[3], np.float32), 1)
    a = sr.shade(oracle, case("cube_ground sh 15")[0], case("cube_ground")[2], lights)
    b = sr.shade(oracle, case("cube_ground sh 7.5")[0], case("cube_ground")[2], lights)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(sq.bits(a[2]), sq.bits(b[2]))


def test_an_interval_changes_the_colour(oracle):
    """Behind the first hit lies another surface with another colour: the yardstick follows the interval (a composition that ignored it
    would pass the identities all the same)."""
    flat, flags, rays, light = case("cube_ground")
    lights = abi.light_staircase(np.asarray(light, np.float32), 4)
    h0, t0, lin0, _ = sr.shade(oracle, flat, rays, lights)
    tr = np.stack([np.nextafter(t0, INF), np.full(t0.shape, INF)], axis=1).astype(np.float32)
    h1, t1, lin1, rgb8 = sr.shade(oracle, flat, rays, lights, t_range=tr)
    both = (h0 >= 0) & (h1 >= 0)
    assert both.sum() >= 5 and (h1[both] != h0[both]).all() and (t1[both] > t0[both]).all()
    assert np.any(sq.bits(lin1[both]) != sq.bits(lin0[both]), axis=1).any()
    gone = (h0 >= 0) & (h1 < 0)
    assert (lin1[h1 < 0] == 0).all() and (rgb8[h1 < 0] == np.array(abi.REFERENCE_BACKGROUND, np.uint8)).all() and np.isposinf(t1[h1 < 0]).all()
    print("second hits", int(both.sum()), "hits with nothing behind", int(gone.sum()))
