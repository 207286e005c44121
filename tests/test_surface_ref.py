"""CPU: tests/surface_ref.py -- the yardstick of srt_surface_rays / srt_surface_hits -- tied to the oracle, not to the code under test.

What shading is given for a hit is what the oracle's own frame shades it with: for every hit ray of a small camera-mode frame, Phong by
the oracle's leaf function on (the ray, the hit's points, each light, surface_ref's colour, surface_ref's material, t), summed over the
lights in light order with float32 adds, is the oracle's rgb_linear of that ray without shadow division, bit for bit -- so the colour
(the texel included) and the material are the ones softShadow reads.  The oracle's Phong derives the face normal from the points itself;
surface_ref's numpy restatement of it is held to unit length and to a float64 normal.  The reflection formula is held to its identities."""
import functools

import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import shade_query_ref as sq
import surface_ref as sf
from shade_range_ref import look_at

W, H, N_LIGHTS = 24, 16, 3
bits = sf.bits
ULP1 = float(np.spacing(np.float32(1.0)))


def frame_of(name):
    """(flat, rays, lights) of the 24 x 16 camera-mode frame of a scene."""
    g = gu.GoldenScene(name)
    if name == "cube_ground":
        rays = rq.frame_rays(W, H, look_at((-40.0, -400.0, 330.0), (-80.0, 105.0, 390.0)), 30.0)
    else:
        rays = rq.frame_rays(W, H, rq.SHEAR, rq.FOCAL[name] * W / rq.FRAME_W)
    return g.flat, rays, sq.lights_for(name, g.light, N_LIGHTS)


@functools.lru_cache(maxsize=None)
def shaded(name):
    """The oracle's answer for the frame's rays (shadow_div 1: a shadowed sample is added as it is) and surface_ref's rows for its hits."""
    from oracle import pyoracle
    flat, rays, lights = frame_of(name)
    hit, t, lin, _ = sq.oracle_shade(pyoracle, flat, rays, lights, shadow_div=1.0)
    return flat, rays, lights, hit, t, lin, sf.surface(pyoracle, flat, rays, hit, t)


@pytest.mark.parametrize("name", ["texquad", "cubes4_a40", "cube_ground"])
def test_colour_and_material_are_what_the_oracle_shades_with(oracle, name):
    flat, rays, lights, hit, t, lin, s = shaded(name)
    sel = np.flatnonzero(hit >= 0)
    assert sel.size >= W * H // 10, (name, sel.size)
    assert np.array_equal(s["obj"][sel], flat.tri_obj[hit[sel]]) and (s["obj"][hit < 0] == -1).all()
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 12)[hit[sel]]
    acc = np.zeros((sel.size, 3), np.float32)
    for l in range(N_LIGHTS):
        rows = np.zeros((sel.size, 28), np.float32)
        rows[:, 0:6] = rays[sel]; rows[:, 6:18] = pts; rows[:, 18:21] = lights[l]
        rows[:, 21:24] = s["color"][sel]; rows[:, 24:27] = s["material"][sel]; rows[:, 27] = t[sel]
        acc = (acc + oracle.phong(rows, pow="device")).astype(np.float32)
    bad = np.any(bits(acc) != bits(lin[sel]), axis=1)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {sel.size} hits shade differently, first at ray {int(sel[np.flatnonzero(bad)[0]])}"
    # the point is the one Phong and the shadow ray start from: o + d * t
    assert np.array_equal(bits(s["point"][sel]), bits(rq.shadow_rays(rays[sel], t[sel], lights[0])[:, 0:3]))
    assert np.array_equal(bits(s["bounce"][:, 0:3]), bits(s["point"]))
    for k in ("point", "normal", "color", "material", "bounce"):
        assert (bits(s[k][hit < 0]) == 0).all(), k


def test_the_texel_path_is_taken_on_texquad(oracle):
    flat, rays, lights, hit, t, lin, s = shaded("texquad")
    sel = np.flatnonzero(hit >= 0)
    textured = flat.tri_tex[hit[sel]] >= 0
    own = np.asarray(flat.obj_color, np.float32).reshape(-1, 3)[flat.tri_obj[hit[sel]]]
    differs = np.any(bits(s["color"][sel]) != bits(own), axis=1)
    assert (textured & differs).any(), "no textured hit with a colour other than its object's"
    assert not (differs & ~textured).any()
    assert len({tuple(c) for c in bits(s["color"][sel][textured]).tolist()}) > 4, "the texels of the frame are (almost) one colour"


@pytest.mark.parametrize("name", ["texquad", "cubes4_a40", "cube_ground", "ground_bunny"])
def test_face_normal_is_unit_and_agrees_with_float64(name):
    flat = gu.GoldenScene(name).flat
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 12)
    N = sf.face_normal(pts)
    length = np.sqrt((N.astype(np.float64) ** 2).sum(1))
    assert np.abs(length - 1.0).max() <= 2 * ULP1, np.abs(length - 1.0).max() / ULP1
    p = pts.astype(np.float64)
    c = np.cross(p[:, 4:7] - p[:, 0:3], p[:, 8:11] - p[:, 0:3])
    c /= np.linalg.norm(c, axis=1, keepdims=True)
    assert np.abs(N - c).max() <= 1e-6, np.abs(N - c).max()


def test_reflection_identities():
    rng = np.random.default_rng(7)
    d = rng.standard_normal((500, 3)).astype(np.float32) * np.float32(30.0)
    N = rng.standard_normal((500, 3)).astype(np.float32)
    N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(bits(sf.reflect(d, N)), bits(sf.reflect(d, -N)))                # no orientation needed
    # d perpendicular to N: r == d;  d parallel to N: r == -d  (axis normals, exactly representable components)
    for axis in range(3):
        n = np.zeros((1, 3), np.float32); n[0, axis] = 1.0
        perp = np.float32([[1.5, -2.25, 7.0]]); perp[0, axis] = 0.0
        assert np.array_equal(bits(sf.reflect(perp, n)), bits(perp))
        for c in (3.0, -0.75, 1024.5):
            par = n * np.float32(c)
            assert np.array_equal(sf.reflect(par, n), -par) and np.array_equal(sf.reflect(par, -n), -par)
    # the mirror keeps the tangential part and flips the normal part: |r| == |d| up to rounding
    r = sf.reflect(d, N).astype(np.float64)
    assert np.allclose(np.linalg.norm(r, axis=1), np.linalg.norm(d.astype(np.float64), axis=1), rtol=1e-5)
