"""CPU-only: the goniometer of tests/ao_edges.py on the yardstick (tests/ao_ref.py) alone -- its rows reach the cases it names, every aimed
bit is decided by its own blocker, and a subtly wrong kernel would be seen: each VARIANT of the frame or of w below, swapped in for
ao_ref.frame / ao_ref.ao_rays while a Case is built, changes rows or flips aimed bits.  The counts were measured on the yardstick and are
asserted with ==, as PARTIAL is in tests/test_ao_ref.py.  The variants live here, not in ao_ref.py."""
import contextlib
import functools

import numpy as np
import pytest

import ao_edges as ae
import ao_ref as ar

F32, F64 = np.float32, np.float64
K = ae.K
COARSE = ("no_flip", "flip_ge", "s_ge", "swap_TB", "tz_no_s", "bz_pos", "b_neg", "frame_from_N")
ULP = ("b_assoc", "a_ulp", "fma_tx", "fma_by", "fma_w1", "fma_w2", "w_assoc", "k_single", "b_flush")
CASES = (("rays", False), ("rays", True), ("hits", False))


def fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64; the sum is rounded once more, to float32."""
    with np.errstate(all="ignore"):
        return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(np.float32)


def frame_variant(kind):
    """ao_ref.frame with one thing wrong (float32 only)."""
    def frame(d, N, dtype=np.float32):
        d, N = np.ascontiguousarray(d, np.float32).reshape(-1, 3), np.ascontiguousarray(N, np.float32).reshape(-1, 3)
        one = F32(1.0)
        with np.errstate(all="ignore"):
            if kind == "k_single":                          # one rounding: float64 products and sum
                k = (d.astype(F64) * N.astype(F64)).sum(axis=1).astype(np.float32)
            else:
                k = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
            flip = np.zeros(k.shape, bool) if kind == "no_flip" else (k >= 0) if kind == "flip_ge" else (k > 0)
            Nf = np.where(flip[:, None], -N, N).astype(np.float32)
            x, y, z = (N if kind == "frame_from_N" else Nf).T
            s = np.where(z >= 0, one, -one).astype(np.float32) if kind == "s_ge" else np.copysign(one, z).astype(np.float32)
            a = (-one) / (s + z)
            if kind == "a_ulp":
                a = np.nextafter(a, F32(0.0))
            b = x * (y * a) if kind == "b_assoc" else (x * y) * a
            if kind == "b_neg":
                b = -b
            if kind == "b_flush":
                b = np.where(np.abs(b) < F32(ae.TINY), b * F32(0.0), b)
            sxx = (s * x) * x
            tx = fma(sxx, a, np.full_like(a, one)) if kind == "fma_tx" else one + sxx * a
            by = fma(y * y, a, s) if kind == "fma_by" else s + (y * y) * a
            T = np.stack([tx, s * b, -x if kind == "tz_no_s" else (-s) * x], axis=1).astype(np.float32)
            B = np.stack([b, by, y if kind == "bz_pos" else -y], axis=1).astype(np.float32)
        return (B, T, Nf) if kind == "swap_TB" else (T, B, Nf)
    return frame


def rays_variant(kind):
    """ao_ref.ao_rays with its sum contracted or re-associated."""
    def ao_rays(P, T, B, Nf, dirs):
        P, T, B, Nf = (np.ascontiguousarray(a, np.float32).reshape(-1, 1, 3) for a in (P, T, B, Nf))
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(1, -1, 3)
        u, v, w_ = dirs[:, :, 0:1], dirs[:, :, 1:2], dirs[:, :, 2:3]
        full = lambda a: np.broadcast_to(a, np.broadcast_shapes(T.shape, dirs.shape))
        with np.errstate(all="ignore"):
            tu, bv, nw = T * u, B * v, Nf * w_
            if kind == "fma_w1":
                w = fma(full(T), full(u), full(bv)) + nw
            elif kind == "fma_w2":
                w = fma(full(Nf), full(w_), full(tu + bv))
            else:
                w = tu + (bv + nw)
        w = w.astype(np.float32)
        return np.concatenate([np.broadcast_to(P, w.shape), w], axis=2).astype(np.float32)
    return ao_rays


@contextlib.contextmanager
def swapped(kind):
    keep = ar.frame, ar.ao_rays
    if kind in ("fma_w1", "fma_w2", "w_assoc"):
        ar.ao_rays = rays_variant(kind)
    else:
        ar.frame = frame_variant(kind)
    try:
        yield
    finally:
        ar.frame, ar.ao_rays = keep


def make_case(oracle, key, dirs=ae.T16):
    g = ae.build()
    if key[0] == "rays":
        return ar.Case(oracle, g.flat, g.rays, dirs, smooth=key[1])
    return ar.Case(oracle, g.flat, g.hits.rays, dirs, smooth=key[1], hits=(g.hits.hit_id, g.hits.t))


def flush_bits(case):
    """The bits of ao_edges.flush()'s pairs on a Case of the hits batch at T_ODD."""
    f = ae.flush()
    return case.blocked(t_max=ae.FLUSH_T_MAX)[f.row, f.entry]


@functools.lru_cache(maxsize=None)
def flush_case(kind):
    from oracle import pyoracle
    if kind is None:
        return make_case(pyoracle, ("hits", True), ae.T_ODD)
    with swapped(kind):
        return make_case(pyoracle, ("hits", True), ae.T_ODD)


@functools.lru_cache(maxsize=None)
def effect(kind):
    """What a variant changes, per case of CASES: (rows whose occ_bits change, aimed pairs whose bit flips -- indices into aimed())."""
    from oracle import pyoracle
    a = ae.aimed()
    out = {}
    for key in CASES:
        base = ae.case(*key).blocked(t_max=ae.T_MAX)
        with swapped(kind):
            got = make_case(pyoracle, key).blocked(t_max=ae.T_MAX)
        mine = np.flatnonzero((a.source == key[0]) & (a.smooth == key[1]))
        flipped = mine[base[a.row[mine], a.entry[mine]] != got[a.row[mine], a.entry[mine]]]
        out[key] = (np.flatnonzero((base != got).any(axis=1)), flipped)
    return out


# ---- the conditions ---------------------------------------------------------------------------------------------------------------------
# {case: {class: (rows, rows with 0 < n_occluded < 16)}} at T16, t_max 16, measured on the yardstick.
ROWS = {
    ("rays", False): {"pole+": (32, 32), "pole-": (32, 32), "equator+0": (16, 16), "equator-0": (16, 15), "tilt+": (60, 60), "tilt-": (60, 60), "b_sub": (0, 0),
                      "b_zero": (0, 0), "nan": (0, 0), "general": (288, 285)},
    ("rays", True): {"pole+": (8, 8), "pole-": (8, 8), "equator+0": (16, 16), "equator-0": (16, 15), "tilt+": (60, 60), "tilt-": (60, 60), "b_sub": (16, 16),
                     "b_zero": (16, 16), "nan": (16, 0), "general": (288, 283)},
}
AIMED_PLANNED, AIMED_KEPT = 1650, 1351
AIMED_BY_CLASS = {"pole+": 19, "pole-": 27, "equator+0": 15, "equator-0": 30, "tilt+": 57, "tilt-": 112, "b_sub": 8, "b_zero": 8, "nan": 0, "general": 1075}
AIMED_BY_CASE = {("rays", False): 607, ("rays", True): 720, ("hits", False): 24}


def test_every_class_is_reached(oracle):
    g = ae.build()
    for key, want in ROWS.items():
        c = ae.case(*key)
        assert c.sel.size == g.rays.shape[0], "every main ray hits"
        cls = ae.classify(c.Nf)
        cnt = c.reference(t_max=ae.T_MAX)["n_occluded"].astype(np.int64)
        got = {name: (int((cls == k).sum()), int(((cls == k) & (cnt > 0) & (cnt < K)).sum())) for k, name in enumerate(ae.CLASSES)}
        print(key, got)
        assert got == want, (key, got)
        for name, (rows, partial) in got.items():
            if rows:       # (a NaN frame makes every AO ray NaN: all of them count or none does -- the rows are pinned, never partial)
                assert rows >= 8 and (partial >= 4 or name == "nan"), (key, name, rows, partial)
    flat, smooth = ROWS[("rays", False)], ROWS[("rays", True)]
    assert all(flat[n][0] >= 8 for n in ("pole+", "pole-", "equator+0", "equator-0", "tilt+", "tilt-", "general"))
    assert all(smooth[n][0] >= 8 for n in ("b_sub", "b_zero", "nan"))
    c = ae.case("rays", True)
    b, xy = ae.b_of(c.Nf)
    assert ((b != 0) & (np.abs(b) < ae.TINY)).sum() >= 1 and ((b == 0) & (xy != 0)).sum() >= 1
    kind = np.array(g.kinds)[g.cell]
    # the kinds that tell only under the smooth build: per-vertex normals differ from the face normal, zero and NaN normals give NaN
    plain = ae.case("rays", False)
    assert (c.Nf[kind == "per_vertex"].view(np.uint32) != plain.Nf[kind == "per_vertex"].view(np.uint32)).any(axis=1).all()
    assert np.isnan(c.Nf[kind == "zero"]).all() and np.isnan(c.Nf[kind == "nan"]).any(axis=1).all() and not np.isnan(plain.Nf).any()
    # the near-pole tilts: z one of +-1 with x or y != 0, and z just inside
    z = plain.Nf[kind == "tilt", 2]
    assert (np.abs(z) == 1).sum() >= 8 and (np.abs(z) < 1).sum() >= 8


def test_the_sweeps_and_the_zero_and_nan_dots(oracle):
    g, h = ae.build(), ae.hits_batch()
    c = ae.case("hits", False)
    pts = np.asarray(g.flat.tri_points, np.float32).reshape(-1, 12)
    import surface_ref as sf
    N = sf.face_normal(pts[h.hit_id])
    k = ae.dot_k(h.rays[:, 3:6], N)
    sweep = np.flatnonzero(h.kind == "sweep").reshape(4, ae.SWEEP)
    for rows in sweep:
        assert (k[rows] > 0).any() and (k[rows] <= 0).any() and (np.diff(h.rays[rows, 3].view(np.int32)) != 0).all()
        flipped = (c.Nf[rows].view(np.uint32) != N[rows].view(np.uint32)).any(axis=1)
        assert np.array_equal(flipped, k[rows] > 0) and 0 < flipped.sum() < ae.SWEEP
    kz = np.flatnonzero(h.kind == "k_zero")
    assert (k[kz] == 0).all() and np.signbit(k[kz]).any() and (~np.signbit(k[kz])).any()
    assert np.isnan(k[h.kind == "k_nan"]).all()
    assert (k[h.kind == "degenerate"] != k[h.kind == "degenerate"]).all(), "a zero-area or NaN triangle has a NaN face normal"


def test_every_aimed_bit_is_its_own_blockers(oracle):
    a = ae.aimed()
    got = {name: int((a.cls == k).sum()) for k, name in enumerate(ae.CLASSES)}
    by_case = {key: int(((a.source == key[0]) & (a.smooth == key[1])).sum()) for key in CASES}
    print("aimed pairs: planned", a.planned, "kept", a.row.size, got, by_case)
    assert a.row.size >= 512 and (a.planned, a.row.size) == (AIMED_PLANNED, AIMED_KEPT) and got == AIMED_BY_CLASS and by_case == AIMED_BY_CASE
    for key in CASES:
        mine = np.flatnonzero((a.source == key[0]) & (a.smooth == key[1]))
        assert mine.size
        full, cut = ae.blocked_without(ae.case(*key), a.row[mine], a.entry[mine], a.tri[mine])
        assert full.all() and not cut.any()
        assert (a.t[mine] > ae.T_MIN).all() and (a.t[mine] < ae.T_MAX).all()
    assert np.unique(a.entry).size == K, "every entry of T16 is aimed at"


# ---- the variants -----------------------------------------------------------------------------------------------------------------------
# rows changed over the three cases of CASES, measured
COARSE_ROWS = {"no_flip": 638, "flip_ge": 39, "s_ge": 22, "swap_TB": 1329, "tz_no_s": 485, "bz_pos": 953, "b_neg": 853, "frame_from_N": 637}
# aimed bits flipped over the three cases (k_single: rows of the sweeps; b_flush: bits of ao_edges.flush()), measured
ULP_FLIPS = {"b_assoc": 47, "a_ulp": 176, "fma_tx": 27, "fma_by": 19, "fma_w1": 106, "fma_w2": 199, "w_assoc": 250, "k_single": 7, "b_flush": 8}


@pytest.mark.parametrize("kind", COARSE)
def test_a_coarse_variant_changes_rows(oracle, kind):
    g, h = ae.build(), ae.hits_batch()
    eff = effect(kind)
    n = sum(v[0].size for v in eff.values())
    print(kind, "rows changed", {key: int(v[0].size) for key, v in eff.items()})
    assert n >= 8 and n == COARSE_ROWS[kind], (kind, n)
    if kind == "s_ge":
        for key in CASES:
            z = ae.case(*key).Nf[eff[key][0], 2]
            assert ((z == 0) & np.signbit(z)).all(), "only rows with z = -0 may change"
    if kind == "flip_ge":
        import surface_ref as sf
        N = sf.face_normal(np.asarray(g.flat.tri_points, np.float32).reshape(-1, 12)[h.hit_id])
        zero = np.flatnonzero(ae.dot_k(h.rays[:, 3:6], N) == 0)
        assert np.array_equal(eff[("hits", False)][0], zero) and eff[("rays", False)][0].size == 0
    if kind == "no_flip":
        rows = eff[("hits", False)][0]
        for c in range(4):
            sw = np.flatnonzero(h.kind == "sweep")[c * ae.SWEEP:(c + 1) * ae.SWEEP]
            assert np.isin(sw, rows).any(), f"sweep {c}"


@pytest.mark.parametrize("kind", ULP)
def test_an_ulp_variant_flips_bits(oracle, kind):
    h = ae.hits_batch()
    if kind == "b_flush":
        flips = int((flush_bits(flush_case(None)) != flush_bits(flush_case(kind))).sum())
    elif kind == "k_single":
        flips = int(np.isin(np.flatnonzero(h.kind == "sweep"), effect(kind)[("hits", False)][0]).sum())
    else:
        flips = sum(v[1].size for v in effect(kind).values())
    print(kind, "flips", flips, {key: (int(v[0].size), int(v[1].size)) for key, v in effect(kind).items()} if kind != "b_flush" else "")
    assert flips >= 4 and flips == ULP_FLIPS[kind], (kind, flips)


# ---- tables and intervals ---------------------------------------------------------------------------------------------------------------
def test_the_odd_table(oracle):
    assert ae.T_ODD.shape == (40, 3) and ae.T33.shape[0] == 33 and ae.T1024.shape[0] == 1024 and ae.T7.shape[0] == 7
    c = make_case(oracle, ("rays", False), ae.T_ODD)
    b = c.blocked(t_max=ae.T_MAX)
    fin = b[:, ae.ODD_FINITE]
    assert fin.any() and not fin.all() and fin.any(axis=0).sum() >= 8
    rest = np.setdiff1d(np.arange(40), ae.ODD_FINITE)
    print("T_ODD: rows blocked per entry that is zero or not finite", {int(j): (ae.T_ODD[j].tolist(), int(b[:, j].sum())) for j in rest})
    f = ae.flush()
    bits = flush_bits(flush_case(None))
    print("flush pairs: blocked", bits.astype(int).tolist())
    assert f.row.size == 8


def test_the_intervals_differ_where_they_must(oracle):
    g, a = ae.build(), ae.aimed()
    rows, chosen = ae.interval_batch()
    assert 8 <= rows.size <= 128
    c = ae.case("rays", False)
    r, e = int(a.row[chosen]), int(a.entry[chosen])
    assert r in rows
    got = {}
    for skip in (False, True):
        for name, t_min, t_max in ae.intervals():
            got[(name, skip)] = c.blocked(t_min=t_min, t_max=t_max, skip_self=skip)[rows]
    at = int(np.flatnonzero(rows == r)[0])
    for skip in (False, True):
        assert got[("t_max = t*", skip)][at, e] and not got[("t_max just below t*", skip)][at, e]
        assert got[("t_min = t*", skip)][at, e] and not got[("t_min just above t*", skip)][at, e]
        assert not got[("t_min > t_max", skip)].any()
        assert got[("(NaN, NaN)", skip)].sum() > got[("(NaN, 16)", skip)].sum() > 0      # NaN bounds bound nothing: blockers beyond 16 count too
        assert np.array_equal(got[("(NaN, NaN)", skip)] | True, got[("(-inf, +inf)", skip)] | True)
        assert (got[("(1e-3, NaN)", skip)] <= got[("(NaN, NaN)", skip)]).all()
    # t_min <= 0: the hit's own facet near t = 0 blocks, depending on rounding -- and not under SKIP_SELF, where its object is left out
    plain = c.blocked(t_min=ae.T_MIN, t_max=ae.T_MAX)[rows]
    assert (got[("t_min = 0", False)] != plain).any() and (got[("t_min = -1", False)] != plain).any()
    assert (got[("t_max = t*", True)] != got[("t_max = t*", False)]).any(), "SKIP_SELF must change rows: a coarse blocker shares the facet's object"
    print("intervals: bits set", {k: int(v.sum()) for k, v in got.items()})
