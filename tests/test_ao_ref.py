"""CPU-only: the yardstick of the ambient-occlusion queries (tests/ao_ref.py) on its own -- the frame of the definition, the
concatenation identity, and the input conditions of the cases tests/test_gpu_ao.py compares the device with."""
import numpy as np
import pytest

import ao_ref as ar
import shadow_rule_ref as sh

F64 = np.float64
K = ar.N_DIRS


def deviation(T, B, Nf):
    """The largest deviation of (T, B, Nf) from an orthonormal triple: |dot - delta| over the six products."""
    dot = lambda a, b: (a * b).sum(axis=1)
    return max(np.abs(dot(T, T) - 1).max(), np.abs(dot(B, B) - 1).max(), np.abs(dot(Nf, Nf) - 1).max(), np.abs(dot(T, B)).max(), np.abs(dot(T, Nf)).max(),
               np.abs(dot(B, Nf)).max())


# Measured on the yardstick, in float64, over the facing normals of every hit of the three lamp cases (the normals themselves are float32,
# unit to rounding, and that is what the figure shows: cube_ground 7.3e-8, cubes4_a40 1.3e-7, ground_bunny 2.4e-7 over the
# every-third-ray batch used here and 2.9e-7 over all its 2304 rays).  Allowed: 4 x the largest figure of these batches, rounded up to 2.5e-7.
MEASURED_DEVIATION = 2.5e-7


@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_the_frame_is_orthonormal_and_faces_the_ray(oracle, name):
    c = ar.case(oracle, name)
    d = c.rays[c.sel, 3:6]
    T, B, Nf = ar.frame(d.astype(F64), c.Nf.astype(F64), F64)      # (Nf of Nf: a facing normal is not flipped again)
    assert np.array_equal(Nf, c.Nf.astype(F64))
    dev = deviation(T, B, Nf)
    print(f"{name}: deviation from orthonormal {dev:.3g} over {c.sel.size} hits")
    assert dev <= 4 * MEASURED_DEVIATION, dev
    # right-handed: T x B = Nf
    assert np.abs(np.cross(T, B) - Nf).max() <= 4 * MEASURED_DEVIATION
    # Nf faces the ray, by the definition's own dot
    k = (d[:, 0] * c.Nf[:, 0] + d[:, 1] * c.Nf[:, 1]) + d[:, 2] * c.Nf[:, 2]
    assert (k <= 0).all() and (k < 0).any()
    # both orientations occur in the frame before the flip, or the flip is never exercised
    import surface_ref as sf
    N = sf.face_normal(np.asarray(c.flat.tri_points, np.float32).reshape(-1, 12)[c.hit[c.sel]])
    if name == "ground_bunny":
        assert (ar.frame(d, N)[2] != N).any(axis=1).any(), "no normal is flipped"


def test_the_frame_at_its_edges():
    one_up = np.nextafter(np.float32(-1.0), np.float32(0.0))       # one ulp above -1
    x = np.sqrt(np.float32(1.0) - one_up * one_up).astype(np.float32)
    N = np.float32([[0, 0, 1], [0, 0, -1], [1, 0, 0.0], [1, 0, -0.0], [0.6, 0.8, 0.0], [0.6, 0.8, -0.0], [0, 1, -0.0], [x, 0, one_up], [0, x, one_up]])
    d = -N                                                          # facing: nothing flips
    T, B, Nf = ar.frame(d, N)
    assert np.array_equal(Nf.view(np.uint32), N.view(np.uint32))
    assert np.isfinite(T).all() and np.isfinite(B).all()
    assert deviation(T.astype(F64), B.astype(F64), Nf.astype(F64)) <= 4 * MEASURED_DEVIATION
    assert np.abs(np.cross(T.astype(F64), B.astype(F64)) - Nf).max() <= 4 * MEASURED_DEVIATION
    # the poles and the sign of a zero z
    assert np.array_equal(T[0], [1, 0, 0]) and np.array_equal(B[0], [0, 1, 0])
    assert np.array_equal(T[1], [1, 0, 0]) and np.array_equal(B[1], [0, -1, 0])
    assert np.array_equal(T[2], [0, 0, -1]) and np.array_equal(T[3], [0, 0, 1])      # s = copysignf(1, z) follows the zero's sign
    # a back-facing normal is flipped, a NaN or zero dot flips nothing
    assert np.array_equal(ar.frame(np.float32([[0, 0, 1]]), np.float32([[0, 0, 1]]))[2], [[0, 0, -1]])
    assert np.array_equal(ar.frame(np.float32([[1, 0, 0]]), np.float32([[0, 0, 1]]))[2], [[0, 0, 1]])
    assert np.array_equal(ar.frame(np.float32([[np.nan, 0, 1]]), np.float32([[0, 0, 1]]))[2], [[0, 0, 1]])


def test_ao_rays_restate_the_association():
    rng = np.random.default_rng(5)
    N = rng.normal(size=(9, 3)); N = (N / np.linalg.norm(N, axis=1, keepdims=True)).astype(np.float32)
    T, B, Nf = ar.frame(-N, N)
    P = rng.uniform(-50, 50, (9, 3)).astype(np.float32)
    dirs = ar.directions(5)
    r = ar.ao_rays(P, T, B, Nf, dirs)
    assert r.shape == (9, 5, 6) and r.dtype == np.float32
    for i in range(9):
        for j in range(5):
            u, v, w = dirs[j]
            want = [np.float32(np.float32(np.float32(T[i, a] * u) + np.float32(B[i, a] * v)) + np.float32(Nf[i, a] * w)) for a in range(3)]
            assert np.array_equal(r[i, j, 3:6], np.float32(want)) and np.array_equal(r[i, j, 0:3], P[i])
    # the local z axis is the facing normal, and a unit table gives unit rays to rounding
    assert np.abs(ar.ao_rays(P, T, B, Nf, np.float32([[0, 0, 1]]))[:, 0, 3:6] - Nf).max() == 0
    assert np.abs(np.linalg.norm(r[..., 3:6].astype(F64), axis=2) - 1).max() < 1e-6


def test_pack_and_unpack():
    rng = np.random.default_rng(6)
    for k in (1, 31, 32, 33, 65, 130):
        b = rng.random((7, k)) < 0.4
        cnt, ao, words = ar.pack(b)
        assert words.shape == (7, (k + 31) // 32) and np.array_equal(ar.unpack(words, k), b) and np.array_equal(cnt, b.sum(axis=1))
        assert np.array_equal(ao, ((k - b.sum(axis=1)).astype(np.float32) / np.float32(k)))
        assert not ar.unpack(words, words.shape[1] * 32)[:, k:].any()      # bits >= n_dirs are 0


def test_a_table_is_the_concatenation_of_its_parts(oracle):
    flat, rays = ar.case_rays("cube_ground")
    rays = rays[400:520]
    dirs = ar.directions(40)
    whole = ar.Case(oracle, flat, rays, dirs).blocked(t_max=60.0)
    a, b = ar.Case(oracle, flat, rays, dirs[:7]).blocked(t_max=60.0), ar.Case(oracle, flat, rays, dirs[7:]).blocked(t_max=60.0)
    assert np.array_equal(np.concatenate([a, b], axis=1), whole) and 0 < whole.sum() < whole.size


# The rows with 0 < n_occluded < 16 at 16 cosine directions and t_min 1e-3, measured on the yardstick alone: {(t_max, skip_self): rows}.
# cube_ground and cubes4_a40 over all 1296 rays of their frames (1268 and 1038 hits), ground_bunny over every third of its 2304 rays (768
# rays, 692 hits; over all of them the figures are 359, 105 and 666 of 2074 hits, which costs the yardstick about 75 s).
PARTIAL = {"cube_ground": {(20.0, False): 137, (60.0, False): 453, (20.0, True): 137},
           "cubes4_a40": {(20.0, False): 242, (60.0, False): 242, (20.0, True): 242},
           "ground_bunny": {(20.0, False): 118, (60.0, False): 222, (20.0, True): 34}}


@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_the_input_conditions_of_the_gpu_cases(oracle, name):
    c = ar.case(oracle, name)
    assert np.array_equal(c.dirs.view(np.uint32), ar.directions(K).view(np.uint32))
    ref = {key: c.reference(t_max=key[0], skip_self=key[1]) for key in PARTIAL[name]}
    cond = {key: ar.conditions(r, K) for key, r in ref.items()}
    print(name, cond)
    near, far, skipped = ref[(20.0, False)], ref[(60.0, False)], ref[(20.0, True)]
    for key, want in PARTIAL[name].items():
        assert cond[key]["open"] > 0 and cond[key]["partial"] > 0, (key, cond[key])       # some row is fully open, some row is partial
        assert cond[key]["partial"] == want, (key, cond[key], want)
    assert (near["hit_id"] < 0).any() and (near["n_occluded"][near["hit_id"] < 0] == 0).all() and (near["ao"][near["hit_id"] < 0] == 1).all()
    if name != "cubes4_a40":      # (the four cubes stand closer to one another than either radius: every blocker is inside both)
        assert (near["n_occluded"] != far["n_occluded"]).any() and (near["n_occluded"] <= far["n_occluded"]).all()
    if name == "ground_bunny":    # the one case whose hit object blocks its own hemisphere: a concave mesh
        assert (near["n_occluded"] != skipped["n_occluded"]).any() and cond[(20.0, True)]["partial"] < cond[(20.0, False)]["partial"]
    else:
        assert np.array_equal(near["occ_bits"], skipped["occ_bits"])
