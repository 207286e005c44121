"""CPU: the goniometer of tests/refract_edges.py reaches the cases it is built for, on the yardstick alone.  The rows looked at are the
ones the device evaluates: the rays of the batch whose segment 0 hits a transmitting sheet on the yardstick, with the normal shading uses
there (flat: the face normal; smooth: the interpolated one), through refract_ref.refract_steps.  Every count is printed, then asserted."""
import numpy as np
import pytest

import refract_edges as re
import refract_ref as rf
import surface_ref as sf

bits = sf.bits
TINY = np.finfo(np.float32).tiny


def denormal(a):
    return ((np.abs(a) > 0) & (np.abs(a) < TINY)).reshape(a.shape[0], -1).any(axis=1)


@pytest.fixture(scope="module")
def rows(oracle):
    return {smooth: re.first_hits(oracle, smooth) for smooth in (False, True)}


def test_the_scene_is_what_the_batch_assumes(oracle, rows):
    flat, (rays, kind, sheet, scale) = re.scene(), re.batch()
    assert flat.n_objects == 18 == re.IOR.size == re.REFLECTANCE.size and rays.shape[0] % 64 and rays.shape[0] > 257
    fn = sf.face_normal(np.asarray(flat.tri_points, np.float32).reshape(-1, 12))
    for k in range(re.N_SHEETS):
        want = np.float32([0.0, 0.0, re.sheet_normal_sign(k)])
        assert np.array_equal(bits(fn[2 * k:2 * k + 2]), bits(np.tile(want, (2, 1)))), (k, fn[2 * k:2 * k + 2])      # exactly (+0, +0, +-1)
    idx, _, _, _, _, obj = rows[False]
    # every ray aimed at a sheet hits that sheet first, at every length of d: the miss rows are not where the coverage hides
    assert np.array_equal(obj, sheet), np.flatnonzero(obj != sheet)
    assert set(np.unique(re.IOR[obj[idx]]).tolist()) == set(np.unique(re.IOR[re.IOR > 0]).tolist())
    for smooth in (False, True):
        i, p, d, N, n, _ = rows[smooth]
        # flat: the sheets' own normal; smooth: the (1, 0, 0) sheets and the tilted ones differ from it
        same = np.array_equal(bits(N), bits(np.stack([np.zeros(i.size), np.zeros(i.size), np.where(sheet[i] % 2 == 0, 1.0, -1.0)], axis=1).astype(np.float32)))
        assert same == (not smooth)


@pytest.mark.parametrize("smooth", [False, True])
def test_the_rows_reach_the_cases(rows, smooth):
    rays, kind, sheet, scale = re.batch()
    idx, p, d, N, n, _ = rows[smooth]
    k, out, c = p["k"], p["out"], p["c"]
    count = {}
    # the sweeps: k < 0 next to k >= 0
    for s in re.SWEPT:
        m = (kind[idx] == re.KIND_SWEEP) & (sheet[idx] == s)
        kk = k[m]
        assert m.sum() == re.SWEEP
        flips = int(((kk[:-1] >= 0) & (kk[1:] < 0)).sum() + ((kk[:-1] < 0) & (kk[1:] >= 0)).sum())
        count[f"sweep {s}: flips, distinct k"] = (flips, int(np.unique(kk).size))
        assert flips >= 1, (s, kk)
    count["k == 0"] = int((k == 0).sum())
    nan_k = np.isnan(k)
    mirrored = sf.reflect(d, N)
    nan_r = nan_k & np.isnan(out).any(axis=1)
    count["k NaN"], count["k NaN and r NaN"] = int(nan_k.sum()), int(nan_r.sum())
    count["k NaN, r NaN, the mirrored direction finite"] = int((nan_r & np.isfinite(mirrored).all(axis=1)).sum())
    plus0 = (c == 0) & ~np.signbit(c)
    count["c == +0"], count["c == +0 with finite L"] = int(plus0.sum()), int((plus0 & np.isfinite(p["L"])).sum())
    count["c == +0 and entering"] = int((plus0 & p["entering"]).sum())
    fin = np.isfinite(out).all(axis=1) & (out != 0).any(axis=1)
    count["r finite, not zero"], count["r infinite"] = int(fin.sum()), int(np.isinf(out).any(axis=1).sum())
    count["denormal in I or u"] = int((denormal(p["I"]) | denormal(p["u"])).sum())
    count["L == 0"], count["L == inf"] = int((p["L"] == 0).sum()), int(np.isinf(p["L"]).sum())
    tir = k < 0
    count["k < 0"] = int(tir.sum())
    for name, v in count.items():
        print(f"smooth {smooth}: {name}: {v}")
    assert count["k == 0"] >= 1 and count["k NaN and r NaN"] == count["k NaN"] >= 1 and count["k NaN, r NaN, the mirrored direction finite"] >= 1
    # c == +0: under the smooth build the (1, 0, 0) sheets give it with a finite L; under both builds an overflowed L gives it (I = 0)
    assert count["c == +0"] >= 1 and count["c == +0 and entering"] == 0 and (count["c == +0 with finite L"] >= 1) == smooth
    assert count["r finite, not zero"] >= 100 and count["r infinite"] >= 1 and count["denormal in I or u"] >= 1
    assert count["L == 0"] >= 1 and count["L == inf"] >= 1
    # total internal reflection is the mirrored direction, bit for bit
    assert tir.sum() >= 100 and np.array_equal(bits(out[tir]), bits(mirrored[tir]))
    # Snell's law in float64 where the formula refracts with room to spare, the inputs are finite and d . d neither under- nor overflows
    with np.errstate(invalid="ignore"):
        ok = (k >= np.float32(1e-3)) & np.isfinite(n) & np.isfinite(out).all(axis=1) & (scale[idx] >= 1e-18) & (scale[idx] <= 1e15)
    print(f"smooth {smooth}: rows held to Snell's law: {int(ok.sum())}")
    assert ok.sum() >= 200
    rf.assert_snell(d[ok], N[ok], out[ok], n[ok], p["entering"][ok])


def test_segments_follow(oracle):
    """Colours flow: the mirrors catch segment 1 of many rays and segment 2 of some, under both builds."""
    from simple_raytracer_amd import abi
    flat, rays = re.scene(), re.batch()[0]
    for smooth in (False, True):
        segs, kinds = rf.trace(oracle, flat, rays, np.zeros((0, 3), np.float32), re.DEPTH, re.IOR, bounce_t_min=re.BOUNCE_T_MIN,
                               flags=abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0)
        hits = [int((s.hit >= 0).sum()) for s in segs]
        c = rf.kind_counts(kinds)
        print(f"smooth {smooth}: hits per segment {hits}, kinds at segment 0 {c[0]}")
        assert len(hits) == 3 and hits[1] >= 100 and hits[2] >= 100
        assert min(c[0][w] for w in ("mirror", "enter", "leave", "tir")) >= 50, c[0]


def test_the_frame_sees_the_sheets(oracle):
    """The 16 x 16 frame of refract_edges.frame_params: column i looks at sheet i, so every ior is met, rays enter, leave and are
    totally reflected, and later segments hit."""
    import render_paths_ref as rpr
    flat = re.scene()
    rays, live = rpr.frame_rays_owned(re.frame_params(3))
    assert live.all()
    segs, kinds = rf.trace(oracle, flat, rays.reshape(-1, 6), np.zeros((0, 3), np.float32), re.DEPTH, re.IOR, bounce_t_min=re.BOUNCE_T_MIN)
    obj = segs[0].obj.reshape(16, 16)
    print("frame: objects per column", [sorted(set(obj[:, i].tolist())) for i in range(16)], "kinds", rf.kind_counts(kinds))
    assert all((obj[:, i] == i).all() for i in range(16))
    c = rf.kind_counts(kinds)[0]
    assert min(c[w] for w in ("mirror", "enter", "leave", "tir")) >= 8, c
    assert len(segs) == 3 and (segs[1].hit >= 0).sum() >= 32 and (segs[2].hit >= 0).sum() >= 32
