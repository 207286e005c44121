"""GPU (-m gpu): srt_trace_rays_multi and its _device form (include/srt.h, RAY QUERIES, "The K nearest hits of a ray in one walk"),
pinned bit for bit by tests/ray_multi_ref.py: n_hits, ids, t as uint32, bary as uint32, and the padding of every row.
tests/test_ray_multi_ref.py shows on the CPU that the batches used here hold what they are for (ties up to 4 deep, +0 / -0 pairs,
rows of 7 without a tie, 40 hits on every ray of the stack)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import ray_multi_ref as rm
import ray_query_ref as rq
import ray_range_ref as rr
import tree_shapes as ts
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = np.float32(np.inf), np.float32(np.nan)
IDENTITIES = {"NULL": None, "(0, inf)": (0.0, INF), "(-inf, inf)": (-INF, INF), "(NaN, NaN)": (NAN, NAN)}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@functools.lru_cache(maxsize=None)
def reference(name):
    """Computed once and shared: the scene, its batch, the candidates and a mixed interval batch."""
    from oracle import pyoracle
    if name == "stack":
        flat, rays = rm.stack_scene(), rm.stack_rays()
    elif name in ts.FAMILIES:
        flat, rays = ts.family(name), ts.ray_batch(name)
    else:
        flat = gu.GoldenScene(name).flat
        rays = rq.unrelated_rays(flat, 257 if name == "cubes4_a40" else 200, seed=5)
    c = rr.candidates(pyoracle, flat, rays)
    return dict(flat=flat, rays=rays, c=c, tr=rr.mixed_intervals(c, 17)[0])


def check(oracle, flat, rays, c, o, k, tr, what, sel=None):
    """Every array of `o` against the yardstick at (k, tr); sel: the rays of the batch `o` was made from, in its order."""
    n_hits, hit, t = rm.multi(c, k, tr)
    bary = rm.multi_bary(oracle, flat, rays, hit, t) if "bary" in o else None
    if sel is not None:
        n_hits, hit, t = n_hits[sel], hit[sel], t[sel]
        bary = bary[sel] if bary is not None else None
    print(what, "rays", hit.shape[0], "k", k, "rows full / short / empty", int((n_hits >= k).sum()), int(((n_hits < k) & (n_hits > 0)).sum()), int((n_hits == 0).sum()))
    bad = o["n_hits"] != n_hits
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} n_hits differ, first at ray {int(np.flatnonzero(bad)[0])}: {o['n_hits'][bad][0]} for {n_hits[bad][0]}"
    bad = (o["hit_id"] != hit).any(1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows of ids differ, first at ray {int(np.flatnonzero(bad)[0])}: {o['hit_id'][bad][0]} for {hit[bad][0]}"
    assert np.array_equal(bits(o["t"]), bits(t)), f"{what}: t differs"
    if bary is not None:
        assert np.array_equal(bits(o["bary"]), bits(bary)), f"{what}: bary differs"
    assert o["stats"]["primary_rays"] == hit.shape[0] and o["stats"]["hit_rays"] == int((n_hits > 0).sum()), (what, o["stats"])
    return n_hits, hit, t


@pytest.mark.parametrize("k", range(1, 17))
def test_every_k_on_ties(srt, oracle, k):
    """364 rays with ties up to 4 deep and a mixed interval batch: every bucket edge, rows that are full, short and empty, ties that
    straddle the cut at k."""
    r = reference("ties")
    ds = srt.DeviceScene(r["flat"])
    n_hits, hit, t = check(oracle, r["flat"], r["rays"], r["c"], ds.trace_rays_multi(r["rays"], k, t_range=r["tr"]), k, r["tr"], "ties, intervals")
    check(oracle, r["flat"], r["rays"], r["c"], ds.trace_rays_multi(r["rays"], k), k, None, "ties, unbounded")
    ds.close()


def test_overflow_on_the_stack(srt, oracle):
    """40 hits on every ray, a leaf of 31 pushed in slices: the count is full, the rows hold the nearest 16, 8 and 1 in order; a segment
    that admits exactly 16, 17 and 15 layers."""
    r = reference("stack")
    flat, rays, c = r["flat"], r["rays"], r["c"]
    ds = srt.DeviceScene(flat)
    for k in (16, 8, 1):
        n_hits, hit, t = check(oracle, flat, rays, c, ds.trace_rays_multi(rays, k), k, None, "stack")
        assert (n_hits == 40).all() and (hit >= 0).all()
    for layers in (16, 17, 15):
        tr = rm.stack_segment(layers)
        n_hits, hit, t = check(oracle, flat, rays, c, ds.trace_rays_multi(rays, 16, t_range=tr), 16, tr, f"stack, {layers} layers")
        assert (n_hits == layers).all() and ((hit >= 0).sum(1) == min(layers, 16)).all()
    ds.close()


def test_signed_zeros(srt, oracle):
    """The frame of `ties`: over 2,000 rays whose hits are one +0 and one -0 -- lowest id first, each t with its own sign bit."""
    flat, rays = ts.family("ties"), ts.frame_rays()
    c = rr.candidates(oracle, flat, rays)
    pairs = rm.zero_pairs(c)
    assert pairs.sum() >= 2000
    ds = srt.DeviceScene(flat)
    for k in (2, 4):
        o = ds.trace_rays_multi(rays, k)
        n_hits, hit, t = check(oracle, flat, rays, c, o, k, None, "ties frame")
        got = o["hit_id"][pairs], bits(o["t"])[pairs]
        assert (got[0][:, 0] < got[0][:, 1]).all() and (np.sort(got[1][:, :2], axis=1) == np.array([0, 0x80000000], np.uint32)).all()
        assert len(np.unique(bits(t)[pairs][:, 0])) == 2, "both orders of the signs occur"
    ds.close()


def test_wave_and_workgroup_edges(srt, oracle):
    """The first 1, 63, 64, 65 and 257 rays of a batch, and the batch permuted: a ray's row depends on the ray alone."""
    r = reference("cubes4_a40")
    flat, rays, c, tr = r["flat"], r["rays"], r["c"], r["tr"]
    ds = srt.DeviceScene(flat)
    for m in (1, 63, 64, 65, 257):
        sel = np.arange(m)
        check(oracle, flat, rays, c, ds.trace_rays_multi(rays[:m], 4, t_range=tr[:m]), 4, tr, f"first {m}", sel)
        check(oracle, flat, rays, c, ds.trace_rays_multi(rays[:m], 4), 4, None, f"first {m}, unbounded", sel)
    perm = np.random.default_rng(3).permutation(rays.shape[0])
    check(oracle, flat, rays, c, ds.trace_rays_multi(rays[perm], 4, t_range=tr[perm]), 4, tr, "permuted", perm)
    ds.close()


@pytest.mark.parametrize("name", ["sliced", "shuffled", "comb255", "comb256", "roots33"])
def test_tree_shapes(srt, oracle, name):
    """k = 8 on the families' batches, with and without intervals.  On `sliced`, which has no ties, column j is also the j-th call of the
    next_up chain of range calls."""
    r = reference(name)
    flat, rays, c = r["flat"], r["rays"], r["c"]
    ds = srt.DeviceScene(flat)
    o = ds.trace_rays_multi(rays, 8)
    n_hits, hit, t = check(oracle, flat, rays, c, o, 8, None, name)
    check(oracle, flat, rays, c, ds.trace_rays_multi(rays, 8, t_range=r["tr"]), 8, r["tr"], name + ", intervals")
    if name == "sliced":
        assert n_hits.max() == 7
        lo = np.full(rays.shape[0], -INF, np.float32)
        for j in range(7):
            step = ds.trace_rays(rays, t_range=np.stack([lo, np.full_like(lo, INF)], axis=1))
            assert np.array_equal(step["hit_id"], o["hit_id"][:, j]) and np.array_equal(bits(step["t"]), bits(o["t"][:, j])), j
            assert np.array_equal(bits(step["bary"]), bits(o["bary"][:, j])), j
            lo = np.where(step["hit_id"] >= 0, rr.next_up(step["t"]), INF).astype(np.float32)      # (a finished ray stays finished: nothing is >= +inf but +inf, no hit)
    ds.close()


def test_column_0_is_the_range_call(srt, oracle):
    """ground_bunny, 200 rays and a zero-direction and an all-NaN ray: column 0 is trace_rays(t_range=...) bit for bit, for the four
    identity intervals and a mixed batch; the 200 also against the yardstick."""
    r = reference("ground_bunny")
    flat, c = r["flat"], r["c"]
    rays = np.concatenate([r["rays"], np.zeros((1, 6), np.float32), np.full((1, 6), NAN)]).astype(np.float32)
    rays[-2, 0:3] = r["rays"][0, 0:3]
    n = rays.shape[0]
    ds = srt.DeviceScene(flat)
    cases = {k: (None if p is None else np.tile(np.array(p, np.float32), (n, 1))) for k, p in IDENTITIES.items()}
    cases["mixed"] = np.concatenate([r["tr"], np.float32([[0.0, INF], [NAN, 1.0]])])
    for what, tr in cases.items():
        for k in (1, 5):
            o = ds.trace_rays_multi(rays, k, t_range=tr)
            want = ds.trace_rays(rays, t_range=tr)
            assert np.array_equal(o["hit_id"][:, 0], want["hit_id"]) and np.array_equal(bits(o["t"][:, 0]), bits(want["t"])), (what, k)
            assert np.array_equal(bits(o["bary"][:, 0]), bits(want["bary"])), (what, k)
            assert np.array_equal(o["n_hits"] > 0, want["hit_id"] >= 0) and o["stats"]["hit_rays"] == want["stats"]["hit_rays"], (what, k)
            part = {key: v[:200] for key, v in o.items() if key != "stats"}
            part["stats"] = dict(primary_rays=200, hit_rays=int((o["n_hits"][:200] > 0).sum()))
            check(oracle, flat, r["rays"], c, part, k, None if tr is None else tr[:200], f"ground_bunny {what}")
    ds.close()


def test_contract(srt, oracle):
    r = reference("cubes4_a40")
    flat, rays, c, tr = r["flat"], r["rays"], r["c"], r["tr"]
    n = rays.shape[0]
    g = gu.GoldenScene("cubes4_a40")
    ds = srt.DeviceScene(flat)
    p = g.params(121, 91, 3)
    golden = g.out(121, 91, 3, "hit_id")
    before = ds.render(p)
    assert golden is not None and np.array_equal(before["hit_id"], golden)
    # the walk is the unbounded call's: the same node and triangle tests, with and without an interval, at any k
    plain = ds.trace_rays(rays, count=True)["stats"]
    assert plain["node_tests_primary"] > 0 and plain["tri_tests_primary"] > 0
    for k, q in ((1, None), (4, tr), (16, tr)):
        o = ds.trace_rays_multi(rays, k, count=True, t_range=q)
        check(oracle, flat, rays, c, o, k, q, f"counting, k {k}")
        assert (o["stats"]["node_tests_primary"], o["stats"]["tri_tests_primary"]) == (plain["node_tests_primary"], plain["tri_tests_primary"]), (k, o["stats"], plain)
    o = ds.trace_rays_multi(rays, 4, t_range=tr)
    assert o["stats"]["node_tests_primary"] == 0 and o["stats"]["tri_tests_primary"] == 0
    # any output pointer may be NULL
    only = ds.trace_rays_multi(rays, 4, want=("n_hits",), t_range=tr)
    assert set(only) == {"n_hits", "stats"} and np.array_equal(only["n_hits"], o["n_hits"]) and only["stats"]["hit_rays"] == o["stats"]["hit_rays"]
    only = ds.trace_rays_multi(rays, 4, want=("t",), t_range=tr)
    assert set(only) == {"t", "stats"} and np.array_equal(bits(only["t"]), bits(o["t"]))
    none = ds.trace_rays_multi(rays, 4, want=(), t_range=tr)
    assert set(none) == {"stats"} and none["stats"]["hit_rays"] == o["stats"]["hit_rays"]
    # errors, all before anything is touched
    L = srt.load()
    f32p, i32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    r4 = np.ascontiguousarray(rays[:4]); out = np.full((4, 17), -7, np.int32); cnt = np.full(4, 77, np.uint32)
    args = lambda k, flags: (ds.h, 4, r4.ctypes.data_as(f32p), None, k, flags, cnt.ctypes.data_as(u32p), out.ctypes.data_as(i32p), None, None, None)
    assert L.srt_trace_rays_multi(*args(0, 0)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi(*args(17, 0)) == abi.SRT_ERR_LIMIT
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, 2 << 8, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT):
        assert L.srt_trace_rays_multi(*args(4, flags)) == abi.SRT_ERR_ARG, flags
        assert L.srt_trace_rays_multi_device(ds.h, 4, None, None, 4, flags, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi(ds.h, 4, None, None, 4, 0, cnt.ctypes.data_as(u32p), None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi_device(ds.h, 4, None, None, 4, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi_device(ds.h, 4, None, None, 0, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi_device(ds.h, 4, None, None, 17, 0, None, None, None, None, None) == abi.SRT_ERR_ARG      # (NULL rays come first)
    assert (out == -7).all() and (cnt == 77).all()
    with pytest.raises(srt.SrtError) as e:
        ds.trace_rays_multi(rays, 0)
    assert e.value.code == abi.SRT_ERR_ARG
    with pytest.raises(srt.SrtError) as e:
        ds.trace_rays_multi(rays, 17)
    assert e.value.code == abi.SRT_ERR_LIMIT
    # n = 0
    z = ds.trace_rays_multi(np.zeros((0, 6), np.float32), 4, t_range=np.zeros((0, 2), np.float32))
    assert z["hit_id"].shape == (0, 4) and z["n_hits"].shape == (0,) and z["stats"]["primary_rays"] == 0 and z["stats"]["hit_rays"] == 0
    assert L.srt_trace_rays_multi(ds.h, 0, None, None, 4, 0, None, None, None, None, None) == abi.SRT_OK
    assert L.srt_trace_rays_multi_device(ds.h, 0, None, None, 4, 0, None, None, None, None, None) == abi.SRT_OK
    # a second handle on the same records, and the scene renders its frame afterwards
    sh = ds.share()
    check(oracle, flat, rays, c, sh.trace_rays_multi(rays, 4, t_range=tr), 4, tr, "shared handle")
    sh.close()
    check(oracle, flat, rays, c, ds.trace_rays_multi(rays, 4, t_range=tr), 4, tr, "after the refused calls")
    after = ds.render(p)
    assert np.array_equal(after["hit_id"], golden) and np.array_equal(bits(after["t"]), bits(before["t"])) and np.array_equal(after["rgb8"], before["rgb8"])
    ds.close()


def test_device_entry_point():
    """Device pointers from torch tensors in a fresh process (torch initialises HIP first): float-aligned rays and t_range, a second
    stream, a shared handle, one call captured into a hipGraph and replayed twice."""
    p = subprocess.run([sys.executable, os.path.join(HERE, "ray_multi_device_case.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ray multi device case: ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
