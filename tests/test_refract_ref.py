"""CPU: the yardstick of refracting paths (tests/refract_ref.py) against what it extends, its one formula against physics, and the input
conditions of every frame case tests/test_gpu_refract.py uses.  With a table of no positive entry it is shade_path_ref.shade_paths bit for
bit; refract_dir obeys Snell's law in float64; every frame case has mirror hits and entering hits at segment 0 and, at some later
segment, rays that enter, rays that leave and rays that are totally reflected."""
import numpy as np
import pytest

import refract_ref as rf
import shade_path_ref as sp
import surface_ref as sf

bits = sf.bits


@pytest.mark.parametrize("table", ["zeros", "negative", "nan"])
def test_a_table_without_a_positive_entry_is_the_mirror_yardstick(oracle, table):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    ior = {"zeros": np.zeros(flat.n_objects, np.float32), "negative": np.full(flat.n_objects, -1.5, np.float32),
           "nan": np.full(flat.n_objects, np.nan, np.float32)}[table]
    got = rf.shade_paths(oracle, flat, rays, lights, sp.DEPTH, ior, refl, sp.BOUNCE_T_MIN, colours=rf.case_colours(oracle, name), cands=rf.case_memo(oracle, name))
    sp.assert_same(got, sp.frame_reference(oracle, name), f"ior {table}")


def test_refract_dir_obeys_snells_law():
    """Against physics, in float64, not against the formula.  The quantities compared are sines and cosines of unit vectors, so 1e-4 is
    both absolute and relative to 1; the length is compared relative to |d|.  The float32 evaluation errs by about 0.5 / sqrt(k) * 4 * 2^-24
    in a component of the unit vector: 4e-6 at k = 1e-3, a 25th of the bound."""
    rng = np.random.default_rng(20250311)
    m = 10000
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    N = unit(rng.normal(size=(m, 3))).astype(np.float32)
    d = (unit(rng.normal(size=(m, 3))) * rng.uniform(0.1, 500.0, size=(m, 1))).astype(np.float32)
    n = rng.uniform(1.05, 2.5, size=m).astype(np.float32)
    r, entering, k = rf.refract_parts(d, N, n)
    assert entering.sum() > m // 4 and (~entering).sum() > m // 4
    # total internal reflection: the mirrored direction, bit for bit, and only when leaving
    tir = k < 0
    assert tir.sum() > 100 and not (tir & entering).any()
    assert np.array_equal(bits(r[tir]), bits(sf.reflect(d[tir], N[tir])))
    ok = k >= np.float32(1e-3)
    assert ok.sum() > m // 2
    rf.assert_snell(d[ok], N[ok], r[ok], n[ok], entering[ok])


# (enter, leave, tir) at segments 1, 2, 3 of the cases' primary walks, as counted when the cases were chosen
COUNTED = {"cubes4_a40": ((80, 529, 145), (409, 148, 75), (74, 411, 73)),
           "cube_ground": ((562, 245, 209),),
           "ground_bunny": ((690, 478, 255), (42, 397, 525))}


@pytest.mark.parametrize("name", list(rf.DEPTHS))
def test_frame_cases_meet_their_input_conditions(oracle, name):
    segs, kinds = rf.case_walks(oracle, name)
    c = rf.condition(segs, kinds)
    print(name, c)
    assert c[0]["mirror"] >= 100, c[0]
    for b, want in enumerate(COUNTED[name], start=1):
        assert (c[b]["enter"], c[b]["leave"], c[b]["tir"]) == want, (name, b, c[b], want)
