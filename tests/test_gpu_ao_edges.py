"""GPU (-m gpu): srt_ao_rays / srt_ao_hits on the goniometer of tests/ao_edges.py -- the poles, the signed zeros, the near-pole tilts,
subnormal and underflowing b, NaN normals, the flip of k one ulp at a time, zero and NaN dots, blockers aimed at single table entries, odd
and wide tables, the closed interval at a blocker's own t, hits a caller brings with an odd t -- bit for bit against tests/ao_ref.py
(tests/test_ao_edges_ref.py proves on the CPU that the rows reach these cases and that a wrong frame would be seen).  No tolerance anywhere.
Before and after the module a plain ao_rays of the main batch gives the yardstick's bits: the handle survives the NaN rows."""
import functools

import numpy as np
import pytest

import ao_edges as ae
import ao_ref as ar
import ray_range_ref as rr
from test_gpu_ao import check

pytestmark = pytest.mark.gpu
T_MAX = ae.T_MAX


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def ds(srt):
    g = ae.build()
    want = ae.case("rays", False).reference(t_max=T_MAX)
    scene = srt.DeviceScene(g.flat)
    check(scene.ao_rays(g.rays, ae.T16, t_max=T_MAX), want, "the main batch, before everything")
    yield scene
    check(scene.ao_rays(g.rays, ae.T16, t_max=T_MAX), want, "the main batch, after everything")
    scene.close()


@functools.lru_cache(maxsize=None)
def hits_case(smooth, table="T16"):
    from oracle import pyoracle
    h = ae.hits_batch()
    if table == "T16" and not smooth:
        return ae.case("hits", False)
    return ar.Case(pyoracle, ae.scene(), h.rays, getattr(ae, table), smooth=smooth, hits=(h.hit_id, h.t))


@functools.lru_cache(maxsize=None)
def main_case(smooth, table):
    from oracle import pyoracle
    return ar.Case(pyoracle, ae.scene(), ae.build().rays, getattr(ae, table), smooth=smooth)


def prefix(ref, k):
    """The rows of a table's first k entries: a table's row is the concatenation of its parts' rows."""
    cnt, ao, words = ar.pack(ar.unpack(ref["occ_bits"], ae.K)[:, :k])
    return dict(ref, n_occluded=cnt, ao=ao, occ_bits=words)


def check_aimed(o, source, smooth, k, what):
    """Every aimed bit of this build's pairs is set; a failure names the classes of the pairs that are clear."""
    a = ae.aimed()
    mine = np.flatnonzero((a.source == source) & (a.smooth == smooth) & (a.entry < k))
    assert mine.size
    got = ar.unpack(o["occ_bits"], k)[a.row[mine], a.entry[mine]]
    if not got.all():
        bad = mine[~got]
        by_class = {ae.CLASSES[c]: int((a.cls[bad] == c).sum()) for c in np.unique(a.cls[bad])}
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {mine.size} aimed bits are clear, by class {by_class}; first: row {a.row[i]}, entry {a.entry[i]}, "
                             f"class {ae.CLASSES[a.cls[i]]}, blocker {a.tri[i]}")


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("k", [16, 7])
def test_the_main_batch(ds, smooth, k):
    """All eight builds of k_query_ao (flat / smooth, counting or not, srt_ao_rays / srt_ao_hits) under both deals."""
    g = ae.build()
    c = ae.case("rays", smooth)
    table = ae.T16[:k]
    for skip in (False, True):
        want = prefix(c.reference(t_max=T_MAX, skip_self=skip), k)
        for count in (False, True):
            what = f"main batch, {k} directions, smooth {smooth}, skip_self {skip}, counting {count}"
            o = ds.ao_rays(g.rays, table, t_max=T_MAX, skip_self=skip, smooth=smooth, count=count)
            if not skip:
                check_aimed(o, "rays", smooth, k, what)
            check(o, want, what, n_dirs=k)
            h = ds.ao_hits(g.rays, o["hit_id"], o["t"], table, t_max=T_MAX, skip_self=skip, smooth=smooth, count=count)
            check(h, want, what + ", ao_hits", ar.FIELDS, n_dirs=k)


@pytest.mark.parametrize("smooth", [False, True])
def test_the_hits_batch(ds, smooth):
    """The sweeps across k = 0, zero and NaN dots, valid ids with odd t, the degenerate triangles: srt_ao_hits only."""
    h = ae.hits_batch()
    c = hits_case(smooth)
    for k in (16, 7):
        for skip in (False, True):
            want = prefix(c.reference(t_max=T_MAX, skip_self=skip), k)
            for count in (False, True):
                what = f"hits batch, {k} directions, smooth {smooth}, skip_self {skip}, counting {count}"
                o = ds.ao_hits(h.rays, h.hit_id, h.t, ae.T16[:k], t_max=T_MAX, skip_self=skip, smooth=smooth, count=count)
                if not smooth and not skip:
                    check_aimed(o, "hits", False, k, what)
                for kind in np.unique(h.kind):      # kind by kind first: a failure says which rows are off
                    at = np.flatnonzero(h.kind == kind)
                    ar.assert_same({f: o[f][at] for f in ar.FIELDS}, {f: want[f][at] for f in ar.FIELDS}, f"{what}, rows `{kind}`", ar.FIELDS)
                check(o, want, what, ar.FIELDS, n_dirs=k)


@pytest.mark.parametrize("smooth", [False, True])
def test_the_odd_table(ds, smooth):
    """T_ODD on the main batch at t_max 16, and on the hits batch at FLUSH_T_MAX, where the pairs of the subnormal flush live."""
    g, h = ae.build(), ae.hits_batch()
    want = main_case(smooth, "T_ODD").reference(t_max=T_MAX)
    o = ds.ao_rays(g.rays, ae.T_ODD, t_max=T_MAX, smooth=smooth)
    check(o, want, f"T_ODD, main batch, smooth {smooth}", n_dirs=40)
    check(ds.ao_hits(g.rays, o["hit_id"], o["t"], ae.T_ODD, t_max=T_MAX, smooth=smooth), want, f"T_ODD, main batch, smooth {smooth}, ao_hits", ar.FIELDS, n_dirs=40)
    c = hits_case(smooth, "T_ODD")
    o = ds.ao_hits(h.rays, h.hit_id, h.t, ae.T_ODD, t_max=ae.FLUSH_T_MAX, smooth=smooth)
    if smooth:      # the subnormal flush: a kernel that flushes b to zero sets these bits
        f = ae.flush()
        got = ar.unpack(o["occ_bits"], 40)[f.row, f.entry]
        assert not got.any(), f"the bits of the subnormal flush are set in {int(got.sum())} of {got.size} pairs: b = (x * y) * a lost its subnormal"
    check(o, c.reference(t_max=ae.FLUSH_T_MAX), f"T_ODD, hits batch, smooth {smooth}", ar.FIELDS, n_dirs=40)


def test_wide_tables(ds, oracle):
    """33 entries: a second word with one live bit; 1024 entries: sixteen chunks, the last one full, W = 32."""
    g = ae.build()
    rays = np.ascontiguousarray(g.rays[ae.small_batch()])
    assert rays.shape[0] == 70
    for name, n_dirs in (("T33", 33), ("T1024", 1024)):
        table = getattr(ae, name)
        want = ar.Case(oracle, g.flat, rays, table).reference(t_max=T_MAX)
        assert want["occ_bits"].shape == (70, (n_dirs + 31) // 32) and want["occ_bits"][:, -1].any()
        for count in (False, True):
            o = ds.ao_rays(rays, table, t_max=T_MAX, count=count)
            check(o, want, f"{name}, counting {count}", n_dirs=n_dirs)
            check(ds.ao_hits(rays, o["hit_id"], o["t"], table, t_max=T_MAX, count=count), want, f"{name}, counting {count}, ao_hits", ar.FIELDS, n_dirs=n_dirs)


def test_the_interval_at_a_blockers_own_t(ds):
    g, a = ae.build(), ae.aimed()
    rows, chosen = ae.interval_batch()
    rays = np.ascontiguousarray(g.rays[rows])
    c = ae.case("rays", False)
    at, e = int(np.flatnonzero(rows == a.row[chosen])[0]), int(a.entry[chosen])
    for skip in (False, True):
        for name, t_min, t_max in ae.intervals():
            want = {k: v[rows] for k, v in c.reference(t_min=t_min, t_max=t_max, skip_self=skip).items()}
            what = f"interval `{name}`, skip_self {skip}"
            o = ds.ao_rays(rays, ae.T16, t_min=float(t_min), t_max=float(t_max), skip_self=skip)
            if name in ("t_max = t*", "t_min = t*"):
                assert ar.unpack(o["occ_bits"], ae.K)[at, e], what + ": the interval is closed, the blocker at t* counts"
            if name in ("t_max just below t*", "t_min just above t*"):
                assert not ar.unpack(o["occ_bits"], ae.K)[at, e], what + ": the blocker at t* lies outside"
            check(o, want, what)
            check(ds.ao_hits(rays, o["hit_id"], o["t"], ae.T16, t_min=float(t_min), t_max=float(t_max), skip_self=skip), want, what + ", ao_hits", ar.FIELDS)


def test_a_nan_origin_component_goes_to_the_exact_slab_test(ds, oracle):
    """What the k_nan rows found: P = o + d * 0 with an infinite d.x has ONE NaN component, and the AO rays from it whose directions are
    normal floats reached the slab FILTER, whose v_min / v_max dropped the NaN axis and rejected boxes the reference's comparisons pass (a
    direction of length 1e-20 leaves only the triangle with a NaN vertex to answer NaN, and its box was rejected).  ray_rcp(o, d) now sends
    such rays to the exact form.  The same rays through srt_occluded and srt_trace_rays, against ray_range_ref."""
    g, h = ae.build(), ae.hits_batch()
    c = hits_case(False, "T_ODD")
    aor = np.ascontiguousarray(c.ao_rays[np.flatnonzero(h.kind == "k_nan")].reshape(-1, 6))
    nan_o = np.isnan(aor[:, 0:3])
    assert (nan_o.any(axis=1) & ~nan_o.all(axis=1)).all(), "one NaN component, not three"
    cand = rr.candidates(oracle, g.flat, aor)
    tr = np.tile(np.float32([ae.T_MIN, ae.FLUSH_T_MAX]), (aor.shape[0], 1))
    want, plain = rr.occluded(cand, g.flat, tr), rr.occluded(cand, g.flat)
    with np.errstate(invalid="ignore"):
        tiny = np.isfinite(aor[:, 3:6]).all(axis=1) & (np.abs(aor[:, 3:6]).max(axis=1) < 1e-15) & (np.abs(aor[:, 3:6]).min(axis=1) > 1e-30)
    assert want[tiny].sum() >= 4 and plain[tiny].sum() >= 4 and not want[tiny].all(), "rays that only the triangle with a NaN vertex answers"
    assert np.array_equal(ds.occluded(aor), plain), "srt_occluded"
    assert np.array_equal(ds.occluded(aor, t_range=tr), want), "srt_occluded_range"
    assert np.array_equal(ds.occluded(aor, t_range=tr, ray_mask=True), want), "srt_occluded_masked"
    hit, t = rr.closest(cand)
    ar.assert_same(ds.trace_rays(aor, want=("hit_id", "t")), {"hit_id": hit, "t": t}, "srt_trace_rays")
