"""GPU (-m gpu): ray queries with a t interval per ray -- srt_trace_rays_range / srt_occluded_range and their _device forms
(include/srt.h, RAY QUERIES, "A t interval per ray") -- pinned bit for bit by tests/ray_range_ref.py: the oracle's slab test on every
node, its triangle test on every triangle of the reached leaves, and the header's definition in numpy.  Every batch mixes its intervals
ray by ray, so that neighbouring lanes carry different bounds: a kernel that took the testing lane's interval instead of the owner's
would fail.  The golden scenes have leaves of at most 8 triangles; the sliced push of larger leaves is covered by
tests/test_gpu_tree_shapes.py, with the same interval batches (ray_range_ref.mixed_intervals)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import pose_ref
import ray_query_ref as rq
import ray_range_ref as rr
from ray_range_ref import mixed_intervals, want_bary
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = np.float32(np.inf), np.float32(np.nan)
IDENTITIES = {"NULL": None, "(0, inf)": (0.0, INF), "(-inf, inf)": (-INF, INF), "(NaN, NaN)": (NAN, NAN)}
SEGMENT_TARGET = (0.0, 15.0, 100.0)      # a point between the four cubes of cubes4_a40: things lie beyond it (SHADOW_LIGHT is outside the scene)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, host
    build.build_host()
    return host.Transformation


@functools.lru_cache(maxsize=None)
def reference(name, n, seed):
    """Computed once and shared: the scene, n unrelated rays, their candidates, a mixed interval batch, skipped objects, and what the
    yardstick says of them."""
    g = gu.GoldenScene(name)
    flat = g.flat
    from oracle import pyoracle
    rays = rq.unrelated_rays(flat, n, seed=seed)
    c = rr.candidates(pyoracle, flat, rays)
    tr, kind, hit0 = mixed_intervals(c, seed + 1)
    skip = np.random.default_rng(seed + 2).integers(-1, flat.n_objects, n).astype(np.int32)
    want_hit, want_t = rr.closest(c, tr)
    return dict(g=g, flat=flat, rays=rays, c=c, tr=tr, kind=kind, hit0=hit0, skip=skip, hit=want_hit, t=want_t,
                occ=rr.occluded(c, flat, tr, skip), occ_all=rr.occluded(c, flat, tr, None))


def check_closest(o, hit, t, what):
    bad = o["hit_id"] != hit
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(bits(o["t"]), bits(t)), f"{what}: t differs"


@pytest.mark.parametrize("name", ["cubes4_a40", "ground_bunny"])
def test_identities(srt, name):
    """NULL, (0, inf), (-inf, inf) and (NaN, NaN) give the unbounded calls' bits, on unrelated rays plus a zero-direction and a NaN ray."""
    r = reference(name, 200, 77)
    rays = np.concatenate([r["rays"], np.zeros((1, 6), np.float32), np.full((1, 6), NAN)]).astype(np.float32)
    rays[-2, 0:3] = r["rays"][0, 0:3]
    n = rays.shape[0]
    skip = np.concatenate([r["skip"], np.int32([-1, 0])]).astype(np.int32)
    ds = srt.DeviceScene(r["flat"])
    base = ds.trace_rays(rays)
    occ, occ_all = ds.occluded(rays, skip), ds.occluded(rays)
    assert 0.2 < (base["hit_id"] >= 0).mean() < 0.9 and 0 < occ_all.sum() < n
    for what, pair in IDENTITIES.items():
        tr = None if pair is None else np.tile(np.array(pair, np.float32), (n, 1))
        o = ds.trace_rays(rays, t_range=tr)
        check_closest(o, base["hit_id"], base["t"], what)
        assert np.array_equal(bits(o["bary"]), bits(base["bary"])), what
        assert o["stats"]["hit_rays"] == base["stats"]["hit_rays"] and o["stats"]["primary_rays"] == n
        assert np.array_equal(ds.occluded(rays, skip, t_range=tr), occ), what
        assert np.array_equal(ds.occluded(rays, t_range=tr), occ_all), what
    # the identities hold ray by ray: all four kinds in one batch
    tr = np.array([p for p in IDENTITIES.values() if p is not None], np.float32)[np.arange(n) % 3]
    check_closest(ds.trace_rays(rays, t_range=tr), base["hit_id"], base["t"], "mixed identities")
    assert np.array_equal(ds.occluded(rays, skip, t_range=tr), occ)
    ds.close()


@pytest.mark.parametrize("name,n", [("cubes4_a40", 257), ("cube", 130), ("ground_bunny", 200)])
def test_intervals_against_the_yardstick(srt, name, n):
    """Second hits, misses just below the first hit, closed single-point intervals, empty and random intervals, NaN bounds, in ONE
    batch; for cubes4_a40 also the first 1, 63, 64 and 65 rays of it (the wave and workgroup edges)."""
    r = reference(name, n, 5)
    kind, hit0, hit = r["kind"], r["hit0"], r["hit"]
    was_hit = hit0 >= 0
    second = (kind == 0) & was_hit
    # the batch says something: second hits exist and are other triangles, kind 1 misses, kind 2 keeps the id, kind 3 is empty
    assert (hit[second] >= 0).sum() * 2 >= second.sum() > 0 and (hit[second] != hit0[second]).all()
    assert (hit[(kind == 1) & was_hit] == -1).all() and np.array_equal(hit[(kind == 2) & was_hit], hit0[(kind == 2) & was_hit])
    assert (hit[kind == 3] == -1).all() and (r["occ_all"][kind == 3] == 0).all()
    assert 0 < (hit[kind >= 4] >= 0).sum() < (kind >= 4).sum()
    assert 0 < r["occ"].sum() < r["occ_all"].sum() < n
    ds = srt.DeviceScene(r["flat"])
    sizes = (1, 63, 64, 65, n) if name == "cubes4_a40" else (n,)
    for m in sizes:
        o = ds.trace_rays(r["rays"][:m], t_range=r["tr"][:m])
        check_closest(o, hit[:m], r["t"][:m], f"{name}, {m} rays")
        assert o["stats"]["primary_rays"] == m and o["stats"]["hit_rays"] == int((hit[:m] >= 0).sum())
        assert np.array_equal(ds.occluded(r["rays"][:m], r["skip"][:m], t_range=r["tr"][:m]), r["occ"][:m]), m
        assert np.array_equal(ds.occluded(r["rays"][:m], t_range=r["tr"][:m]), r["occ_all"][:m]), m
    # any output pointer may be NULL
    only = ds.trace_rays(r["rays"], want=("hit_id",), t_range=r["tr"])
    assert set(only) == {"hit_id", "stats"} and np.array_equal(only["hit_id"], hit)
    # the same batch in another order gives the same results in that order
    perm = np.random.default_rng(3).permutation(n)
    check_closest(ds.trace_rays(r["rays"][perm], t_range=r["tr"][perm]), hit[perm], r["t"][perm], "permuted")
    ds.close()


def test_bary_on_texquad(srt, oracle):
    """The barycentrics of a second hit are taken at o + d * t of THAT hit, on the scene whose shading reads them."""
    r = reference("texquad", 257, 9)
    flat = r["flat"]
    assert flat.n_textures >= 1 and (flat.tri_tex >= 0).any()
    second = (r["kind"] == 0) & (r["hit"] >= 0)
    assert second.sum() >= 5 and (r["hit"] >= 0).sum() >= 40
    ds = srt.DeviceScene(flat)
    o = ds.trace_rays(r["rays"], t_range=r["tr"])
    check_closest(o, r["hit"], r["t"], "texquad")
    assert np.array_equal(bits(o["bary"]), bits(want_bary(oracle, flat, r["rays"], r["hit"], r["t"])))
    ds.close()


def edge_rays(flat):
    """Axis-aligned rays from outside through points on every triangle's edges: the diagonal of a cube's face belongs to two triangles."""
    P = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)[..., :3]
    ext = np.float32((P.reshape(-1, 3).max(0) - P.reshape(-1, 3).min(0)).max())
    pts = np.concatenate([P[:, a] * np.float32(1 - f) + P[:, b] * np.float32(f) for a, b in ((0, 1), (1, 2), (2, 0)) for f in (0.25, 0.5, 0.75)])
    out = []
    for ax in range(3):
        for sg in (-1.0, 1.0):
            d = np.zeros(3, np.float32); d[ax] = sg
            o = pts.copy(); o[:, ax] -= np.float32(sg) * 2 * ext
            out.append(np.concatenate([o, np.tile(d, (pts.shape[0], 1))], axis=1))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


@pytest.mark.parametrize("name", ["cube", "cubes4_a0"])
def test_ties_go_to_the_lowest_id(srt, oracle, name):
    """Rays whose two nearest candidates have the same t bits (found on the CPU): under (t, t) both are in range, the lowest id wins."""
    flat = gu.GoldenScene(name).flat
    rays = edge_rays(flat)
    c = rr.candidates(oracle, flat, rays)
    hit, t = rr.closest(c)
    at_min = (c.t != -np.inf) & (bits(c.t + np.float32(0.0)) == bits(t + np.float32(0.0))[c.ray])
    tied = (np.bincount(c.ray[at_min], minlength=rays.shape[0]) >= 2) & (hit >= 0)
    print(name, "rays", rays.shape[0], "tied at the minimum", int(tied.sum()))
    assert tied.sum() >= 10
    lowest = np.full(rays.shape[0], np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lowest, c.ray[at_min], c.tri[at_min])
    assert np.array_equal(lowest[tied], hit[tied])
    tr = np.stack([t, t], axis=1).astype(np.float32)
    want_hit, want_t = rr.closest(c, tr)
    assert np.array_equal(want_hit, hit)
    ds = srt.DeviceScene(flat)
    check_closest(ds.trace_rays(rays, t_range=tr), hit, t, name + " (t, t)")
    check_closest(ds.trace_rays(rays), hit, t, name + " unbounded")
    ds.close()


def test_segments(srt, oracle, T):
    """Visibility as segments on cubes4_a40: from the hit points of a frame towards a point, d = target - so, range (0, 1), the hit
    object skipped; and from the same origins ON the surface with t_min = 1e-3 and nothing skipped.  Towards SHADOW_LIGHT (outside the
    scene) and towards a point between the cubes, where the unbounded call sees what lies beyond the target."""
    name = "cubes4_a40"
    flat = gu.GoldenScene(name).flat
    W, H, M, focal = rq.FRAME_W, rq.FRAME_H, rq.rigid(T, 4.0), rq.FOCAL[name]
    fr = oracle.render(flat, rq.camera_params(W, H, M, focal, rq.SHADOW_LIGHT[name]))
    hit, t = fr["hit_id"].reshape(-1), fr["t"].reshape(-1)
    sel = np.flatnonzero(hit >= 0)[::7]
    rays = rq.frame_rays(W, H, M, focal)[sel]
    skip = flat.tri_obj[hit[sel]].astype(np.int32)
    n = sel.size
    ds = srt.DeviceScene(flat)
    for target in (rq.SHADOW_LIGHT[name], SEGMENT_TARGET):
        sray = rq.shadow_rays(rays, t[sel], target)
        c = rr.candidates(oracle, flat, sray)
        seg, lifted = np.tile(np.float32([0.0, 1.0]), (n, 1)), np.tile(np.float32([1e-3, 1.0]), (n, 1))
        want_seg, want_unb = rr.occluded(c, flat, seg, skip), rr.occluded(c, flat, None, skip)
        want_lift, want_self = rr.occluded(c, flat, lifted, None), rr.occluded(c, flat, seg, None)
        print(target, "rays", n, "occluded: unbounded", int(want_unb.sum()), "segment", int(want_seg.sum()), "| nothing skipped: (0, 1)", int(want_self.sum()),
              "(1e-3, 1)", int(want_lift.sum()))
        assert (want_seg <= want_unb).all() and (want_lift <= want_self).all()
        assert 0 < want_lift.sum() < want_self.sum(), "t_min lets no ray off its own surface"
        if target is SEGMENT_TARGET:
            assert ((want_unb == 1) & (want_seg == 0)).sum() >= 100, "no ray is occluded unbounded and free as a segment: move the target"
            assert want_seg.sum() >= 100
        assert np.array_equal(ds.occluded(sray, skip, t_range=seg), want_seg)
        assert np.array_equal(ds.occluded(sray, skip), want_unb)
        assert np.array_equal(ds.occluded(sray, t_range=lifted), want_lift)
        assert np.array_equal(ds.occluded(sray, t_range=seg), want_self)
        # the closest hit inside the segment: what blocks it first
        want_hit, want_t = rr.closest(c, lifted)
        check_closest(ds.trace_rays(sray, t_range=lifted), want_hit, want_t, "closest hit inside the segment")
    ds.close()


def test_counting_build_counts_what_the_unbounded_call_counts(srt):
    """The interval prunes nothing: node and triangle tests of a range call equal the unbounded call's on the same rays."""
    for name in ("cubes4_a40", "ground_bunny"):
        r = reference(name, 257 if name == "cubes4_a40" else 200, 5)
        ds = srt.DeviceScene(r["flat"])
        a = ds.trace_rays(r["rays"], count=True)["stats"]
        o = ds.trace_rays(r["rays"], count=True, t_range=r["tr"])
        check_closest(o, r["hit"], r["t"], name + ", counting")
        b = o["stats"]
        assert a["node_tests_primary"] > 0 and a["tri_tests_primary"] > 0
        assert (b["node_tests_primary"], b["tri_tests_primary"]) == (a["node_tests_primary"], a["tri_tests_primary"]), (name, a, b)
        assert b["hit_rays"] == int((r["hit"] >= 0).sum()) and b["primary_rays"] == r["rays"].shape[0]
        plain = ds.trace_rays(r["rays"], t_range=r["tr"])["stats"]
        assert plain["node_tests_primary"] == 0 and plain["tri_tests_primary"] == 0 and plain["hit_rays"] == b["hit_rays"]
        ds.close()


def test_after_pose(srt, oracle, T):
    """One orbit step on ground_bunny: an interval batch reads the moved records, pinned by the yardstick on pose_ref's flat scene."""
    r = reference("ground_bunny", 200, 5)
    flat, rays = r["flat"], r["rays"]
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = np.tile(pose_ref.orbit_matrix(T, 3.0), (flat.n_objects, 1))
    moved = pose_ref.pose_flat(flat, mats)
    c = rr.candidates(oracle, moved, rays)
    tr, kind, hit0 = mixed_intervals(c, 21)
    want_hit, want_t = rr.closest(c, tr)
    assert not np.array_equal(hit0, rr.closest(r["c"])[0]), "the pose moves nothing these rays see"
    assert ((kind == 0) & (want_hit >= 0)).sum() >= 5
    before = ds.trace_rays(rays, t_range=tr)
    ds.pose(mats)                                             # asynchronous on the scene's own stream: the query is ordered behind it
    check_closest(ds.trace_rays(rays, t_range=tr), want_hit, want_t, "posed")
    assert np.array_equal(ds.occluded(rays, r["skip"], t_range=tr), rr.occluded(c, moved, tr, r["skip"]))
    assert not np.array_equal(before["hit_id"], want_hit)
    ds.close()


def test_edge_cases_and_argument_errors(srt):
    r = reference("cubes4_a40", 257, 5)
    ds = srt.DeviceScene(r["flat"])
    L = srt.load()
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    # n = 0
    o = ds.trace_rays(np.zeros((0, 6), np.float32), t_range=np.zeros((0, 2), np.float32))
    assert o["hit_id"].shape == (0,) and o["stats"]["primary_rays"] == 0 and o["stats"]["hit_rays"] == 0
    assert ds.occluded(np.zeros((0, 6), np.float32), t_range=np.zeros((0, 2), np.float32)).shape == (0,)
    assert L.srt_trace_rays_range(ds.h, 0, None, None, 0, None, None, None, None) == abi.SRT_OK
    assert L.srt_occluded_range(ds.h, 0, None, None, None, None) == abi.SRT_OK
    assert L.srt_trace_rays_range_device(ds.h, 0, None, None, 0, None, None, None, None) == abi.SRT_OK
    assert L.srt_occluded_range_device(ds.h, 0, None, None, None, None, None) == abi.SRT_OK
    # a NULL occluded leaves the call nothing to report
    r4, q4 = np.ascontiguousarray(r["rays"][:4]), np.ascontiguousarray(r["tr"][:4])
    assert L.srt_occluded_range(ds.h, 4, r4.ctypes.data_as(f32p), q4.ctypes.data_as(f32p), None, None) == abi.SRT_OK
    # a second handle on the same records
    sh = ds.share()
    check_closest(sh.trace_rays(r["rays"], t_range=r["tr"]), r["hit"], r["t"], "shared handle")
    sh.close()
    # argument errors, all before anything is touched (only what the host rejects)
    out = np.full(4, -7, np.int32); occ = np.full(4, 9, np.uint8)
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, 2 << 8, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT):
        assert L.srt_trace_rays_range(ds.h, 4, r4.ctypes.data_as(f32p), q4.ctypes.data_as(f32p), flags, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG, flags
        assert L.srt_trace_rays_range_device(ds.h, 4, None, None, flags, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_range(ds.h, 4, None, q4.ctypes.data_as(f32p), 0, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_range(ds.h, 4, None, q4.ctypes.data_as(f32p), None, occ.ctypes.data_as(u8p)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_range_device(ds.h, 4, None, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_range_device(ds.h, 4, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_range(None, 4, r4.ctypes.data_as(f32p), q4.ctypes.data_as(f32p), 0, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_range(None, 4, r4.ctypes.data_as(f32p), q4.ctypes.data_as(f32p), None, occ.ctypes.data_as(u8p)) == abi.SRT_ERR_ARG
    assert (out == -7).all() and (occ == 9).all()
    check_closest(ds.trace_rays(r["rays"], t_range=r["tr"]), r["hit"], r["t"], "after the refused calls")
    ds.close()


def run_case(mode):
    p = subprocess.run([sys.executable, os.path.join(HERE, "ray_range_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and f"ray range {mode} case: ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


def test_device_entry_points():
    """Device pointers from torch tensors on a second stream: the host forms' bits, the identities, a t_range pointer that is only
    float-aligned, a shared handle (own process: torch initialises HIP first)."""
    run_case("device")


def test_range_call_captured_into_a_hip_graph():
    """srt_trace_rays_range_device and srt_occluded_range_device captured once into a hipGraph and replayed once: the same bits."""
    run_case("graph")
