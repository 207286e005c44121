"""CPU-only: the yardstick of ambient occlusion in a frame (tests/render_ao_ref.py) on its own -- it is ao_ref on the frame's rays where no
rotation is given, a (1, 0) rotation changes nothing on finite tables, a real rotation does change rows, the bent sum is the sequential
sum it says it is -- and the input conditions of the cases tests/test_gpu_render_ao.py compares the device with."""
import numpy as np
import pytest

import ao_ref as ar
import render_ao_ref as ra
import render_paths_ref as rp

K = ra.N_DIRS
DIRS = ar.directions(K)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def frame_rows(ref):
    """ao_ref's flat rows of a frame-shaped result."""
    return {k: ref[k].reshape((-1,) + ref[k].shape[2:]) for k in ("hit_id", "t") + ar.FIELDS}


@pytest.mark.parametrize("name", ra.NAMES)
def test_without_a_rotation_it_is_ao_ref_on_the_frames_rays(oracle, name):
    flat, p = ra.case(name)
    rays, live = rp.frame_rays_owned(p)
    assert live.all()
    want = ar.ao(oracle, flat, rays.reshape(-1, 6), DIRS, t_max=60.0)
    got = ra.case_reference(oracle, name, 60.0, rotated=False)
    ar.assert_same(frame_rows(got), want, f"{name}, no rotation")
    # a 1 x 1 table holding (1, 0): 1 * u - 0 * v and 0 * u + 1 * v are u and v for finite u, v
    one = ra.render_ao(oracle, flat, p, DIRS, np.float32([[[1.0, 0.0]]]), t_max=60.0)
    ar.assert_same(frame_rows(one), want, f"{name}, the identity rotation")
    assert np.array_equal(bits(one["bent"]), bits(got["bent"])) and np.array_equal(one["ao8"], got["ao8"])
    assert np.array_equal(got["ao8"], (got["ao"].astype(np.float64) * 255.0 + 0.5).astype(np.int64).astype(np.uint8)), "ao8 rounds to nearest"
    assert (got["ao8"][got["hit_id"] < 0] == 255).all() and (bits(got["bent"][got["hit_id"] < 0]) == 0).all()


def test_the_rotated_table():
    d = ar.directions(16)
    c, s = ra.rotations(4, 4)[0, 0]        # entry 0: a turn by 0.309 of a circle, which moves a direction of radius r by 1.65 r
    r = ra.rotate(d, c, s)
    assert r.dtype == np.float32 and np.array_equal(bits(r[:, 2]), bits(d[:, 2]))
    want = np.stack([np.float64(c) * d[:, 0] - np.float64(s) * d[:, 1], np.float64(s) * d[:, 0] + np.float64(c) * d[:, 1]], axis=1)
    assert np.abs(r[:, :2] - want).max() < 3e-7 and np.abs(r[:, :2] - d[:, :2]).max() > 0.1
    assert np.array_equal(bits(ra.rotate(d, 1.0, 0.0)), bits(d))
    # entry (y % h, x % w) of the IMAGE pixel, whatever the share
    import shadow_rule_ref as sh
    _, _, lights, _ = sh.lamp_case("cube_ground")
    rot = ra.rotations(3, 5)
    whole = ra.rot_entry(rp.camera_params("cube_ground", lights, 37, 23), rot)
    assert whole[7, 4] == (7 % 5) * 3 + 4 % 3 and whole.shape == (23, 37)
    p = rp.camera_params("cube_ground", lights, 37, 23, block_rows=8, block_cols=8, block_stride=3, block_first=1)
    own = rp.owned(p)
    share = ra.rot_entry(p, rot)
    assert (share[own < 0] == -1).all() and (own < 0).any()
    assert np.array_equal(share[own >= 0], whole.reshape(-1)[own[own >= 0]])
    assert (share[own >= 0] != ra.rot_entry(rp.camera_params("cube_ground", lights, own.shape[1], own.shape[0]), rot)[own >= 0]).any(), "local pixels would index otherwise"


def test_the_bent_sum_is_sequential():
    rng = np.random.default_rng(11)
    w = (rng.standard_normal((5, 40, 3)) * np.float32(10.0) ** rng.integers(-3, 4, (5, 40, 1))).astype(np.float32)
    open_rows = np.zeros((5, 40), bool)
    got = ra.bent_sum(w, open_rows)
    for i in range(5):
        acc = np.zeros(3, np.float32)
        for j in range(40):
            acc = (acc + w[i, j]).astype(np.float32)
        assert np.array_equal(bits(got[i]), bits(acc)), "a fully open row: the sequential sum of the whole table"
    assert (bits(got) != bits(ra.bent_sum(w[:, ::-1], open_rows))).any(), "the order matters on these values"
    assert (bits(ra.bent_sum(w, ~open_rows)) == 0).all(), "a closed row: (+0, +0, +0)"
    half = np.arange(40)[None, :] % 2 == 0
    assert np.array_equal(bits(ra.bent_sum(w, np.broadcast_to(half, (5, 40)))), bits(ra.bent_sum(w[:, 1::2], np.zeros((5, 20), bool))))


@pytest.mark.parametrize("name", ra.NAMES)
def test_the_input_conditions_of_the_gpu_cases(oracle, name):
    """At both radii: pixels that hit and pixels that miss, rows partially blocked; the 4 x 4 rotation changes at least one row's bits."""
    for t_max in ra.RADII:
        plain, turned = ra.case_reference(oracle, name, t_max, rotated=False), ra.case_reference(oracle, name, t_max)
        for ref in (plain, turned):
            c = ra.conditions(ref, K)
            print(name, t_max, c)
            assert 0 < c["partial"] and 0 < c["hits"] < c["pixels"], c
        assert np.array_equal(plain["hit_id"], turned["hit_id"]) and np.array_equal(bits(plain["t"]), bits(turned["t"]))
        changed = int((plain["occ_bits"] != turned["occ_bits"]).any(axis=2).sum())
        print(name, t_max, "rows the rotation changes:", changed)
        assert changed > 0
        open_rows = (turned["n_occluded"] == 0) & (turned["hit_id"] >= 0)
        assert open_rows.any() and (bits(turned["bent"][open_rows]) != bits(plain["bent"][open_rows])).any(), "an open row's bent sum follows the turned table"
