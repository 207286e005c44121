"""GPU (-m gpu): ray queries -- srt_trace_rays / srt_occluded and their _device forms (include/srt.h, RAY QUERIES) -- pinned bit for
bit by the oracle as it stands, through the two reductions of tests/ray_query_ref.py: a W x H camera-mode frame is W * H rays, a ray
is a 1 x 1 camera-mode frame, and two frames with shadow_div 1 and 2 read out which hit pixels are in shadow."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import pose_ref
import ray_query_ref as rq
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = rq.FRAME_W, rq.FRAME_H


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


def want_bary(oracle, flat, rays, hit, t):
    """oracle.barycentric on (tri_points[hit], o + d * t) for the hits, (0, 0, 0) for the misses."""
    out = np.zeros((rays.shape[0], 3), np.float32)
    sel = hit >= 0
    dt = rays[sel, 3:6] * t[sel, None]
    P = rays[sel, 0:3] + dt
    pts = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 12)[hit[sel]]
    out[sel] = oracle.barycentric(np.concatenate([pts, P], axis=1))
    return out


def check_against_frame(oracle, flat, rays, o, c, what):
    """A query result `o` over frame-shaped rays against the oracle's camera-mode frame `c`."""
    hit, t = c["hit_id"].reshape(-1), c["t"].reshape(-1)
    bad = o["hit_id"] != hit
    assert not bad.any(), f"{what}: {int(bad.sum())} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(bits(o["t"]), bits(t)), f"{what}: t differs"
    assert np.array_equal(bits(o["bary"]), bits(want_bary(oracle, flat, rays, hit, t))), f"{what}: barycentrics differ"
    assert o["stats"]["primary_rays"] == rays.shape[0] and o["stats"]["hit_rays"] == int((hit >= 0).sum()), (what, o["stats"])


@pytest.mark.parametrize("matrix", ["rigid", "shear"])
@pytest.mark.parametrize("name", ["ground_bunny", "cubes4_a40", "texquad"])
def test_frame_shaped_batches(srt, oracle, T, name, matrix):
    g = gu.GoldenScene(name)
    flat = g.flat
    if name == "texquad":
        assert flat.n_textures >= 1 and (flat.tri_tex >= 0).any()
    M = rq.rigid(T, 4.0) if matrix == "rigid" else rq.SHEAR
    c = oracle.render(flat, rq.camera_params(W, H, M, rq.FOCAL[name], g.light))
    n_hit = int((c["hit_id"] >= 0).sum())
    assert 0.1 * W * H < n_hit < 0.9 * W * H, n_hit
    rays = rq.frame_rays(W, H, M, rq.FOCAL[name])
    ds = srt.DeviceScene(flat)
    o = ds.trace_rays(rays, count=True)
    what = f"{name} {matrix}"
    check_against_frame(oracle, flat, rays, o, c, what)
    print(what, "node tests", o["stats"]["node_tests_primary"], c["stats"]["node_tests_primary"], "triangle tests", o["stats"]["tri_tests_primary"],
          c["stats"]["tri_tests_primary"])
    assert o["stats"]["node_tests_primary"] == c["stats"]["node_tests_primary"], what
    assert o["stats"]["tri_tests_primary"] == c["stats"]["tri_tests_primary"], what
    plain = ds.trace_rays(rays)
    check_against_frame(oracle, flat, rays, plain, c, what + ", no counting")
    assert plain["stats"]["node_tests_primary"] == 0 and plain["stats"]["tri_tests_primary"] == 0
    # the same batch in another order gives the same results in that order
    perm = np.random.default_rng(11).permutation(rays.shape[0])
    q = ds.trace_rays(rays[perm])
    assert np.array_equal(q["hit_id"], o["hit_id"][perm]) and np.array_equal(bits(q["t"]), bits(o["t"][perm]))
    assert np.array_equal(bits(q["bary"]), bits(o["bary"][perm]))
    # any output pointer may be NULL
    only_t = ds.trace_rays(rays, want=("t",))
    assert set(only_t) == {"t", "stats"} and np.array_equal(bits(only_t["t"]), bits(o["t"]))
    assert ds.trace_rays(rays, want=())["stats"]["hit_rays"] == n_hit
    ds.close()


@pytest.mark.parametrize("name", ["ground_bunny", "cubes4_a40"])
def test_unrelated_rays(srt, oracle, name):
    """2,000 rays that share nothing, each against its own 1 x 1 oracle frame."""
    g = gu.GoldenScene(name)
    rays = rq.unrelated_rays(g.flat, 2000)
    assert not np.signbit(rays[:, 3:6][rays[:, 3:6] == 0]).any()
    hit, t = rq.oracle_trace(oracle, g.flat, rays)
    share = float((hit >= 0).mean())
    print(name, "hit share", share)
    assert share >= 0.2 and 1.0 - share >= 0.2
    ds = srt.DeviceScene(g.flat)
    o = ds.trace_rays(rays)
    bad = o["hit_id"] != hit
    assert not bad.any(), f"{int(bad.sum())} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}: {rays[np.flatnonzero(bad)[0]]}"
    assert np.array_equal(bits(o["t"]), bits(t))
    assert np.array_equal(bits(o["bary"]), bits(want_bary(oracle, g.flat, rays, hit, t)))
    ds.close()


@pytest.mark.parametrize("name", sorted(rq.SHADOW_LIGHT))
def test_occlusion(srt, oracle, T, name):
    """Every hit pixel of a frame: the shadow ray of in_shadow, the hit object skipped, against the two-frame read-out."""
    g = gu.GoldenScene(name)
    flat = g.flat
    M, focal, light = rq.rigid(T, 4.0), rq.FOCAL[name], rq.SHADOW_LIGHT[name]
    hit, t, shadowed, usable = rq.shadow_readout(oracle, flat, W, H, M, focal, light)
    sel = hit >= 0
    assert np.array_equal(usable, sel), f"{int((sel & ~usable).sum())} hit pixels would be left out of the comparison"
    share = float(shadowed[sel].mean())
    print(name, "hit pixels", int(sel.sum()), "shadowed share", share)
    assert share >= 0.01 and 1.0 - share >= 0.01
    rays = rq.frame_rays(W, H, M, focal)
    sray = rq.shadow_rays(rays[sel], t[sel], light)
    skip = flat.tri_obj[hit[sel]].astype(np.int32)
    ds = srt.DeviceScene(flat)
    occ = ds.occluded(sray, skip)
    assert set(np.unique(occ)) <= {0, 1}
    bad = occ.astype(bool) != shadowed[sel]
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} shadow rays differ from the oracle's frames"
    # nothing skipped: NULL, -1 and out-of-range entries are the same thing, and can only add occluders
    none = ds.occluded(sray)
    assert np.array_equal(none, ds.occluded(sray, np.full(sray.shape[0], -1, np.int32)))
    wild = np.full(sray.shape[0], flat.n_objects, np.int32)
    wild[1::3] = 2 ** 31 - 1; wild[2::3] = -2 ** 31
    assert np.array_equal(none, ds.occluded(sray, wild))
    assert (none >= occ).all()
    perm = np.random.default_rng(5).permutation(sray.shape[0])
    assert np.array_equal(ds.occluded(sray[perm], skip[perm]), occ[perm])
    ds.close()


def test_after_pose(srt, oracle, T):
    """One orbit step on ground_bunny: the query reads the moved records, pinned by the oracle on pose_ref's flat scene."""
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    rays = rq.frame_rays(192, 108, rq.SHEAR, 40.0)
    before = ds.trace_rays(rays)
    mats = np.tile(pose_ref.orbit_matrix(T, 3.0), (flat.n_objects, 1))
    ds.pose(mats)                                             # asynchronous on the scene's own stream: the query is ordered behind it
    o = ds.trace_rays(rays, count=True)
    want = pose_ref.pose_flat(flat, mats)
    c = oracle.render(want, rq.camera_params(192, 108, rq.SHEAR, 40.0, g.light))
    check_against_frame(oracle, want, rays, o, c, "posed")
    assert o["stats"]["node_tests_primary"] == c["stats"]["node_tests_primary"] and o["stats"]["tri_tests_primary"] == c["stats"]["tri_tests_primary"]
    assert not np.array_equal(before["hit_id"], o["hit_id"])
    ds.close()


def test_edge_cases_and_argument_errors(srt, oracle):
    g = gu.GoldenScene("cubes4_a40")
    flat = g.flat
    ds = srt.DeviceScene(flat)
    L = srt.load()
    f32p, i32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    # n = 0
    o = ds.trace_rays(np.zeros((0, 6), np.float32))
    assert o["hit_id"].shape == (0,) and o["stats"]["primary_rays"] == 0 and o["stats"]["hit_rays"] == 0
    assert ds.occluded(np.zeros((0, 6), np.float32)).shape == (0,)
    assert L.srt_trace_rays(ds.h, 0, None, 0, None, None, None, None) == abi.SRT_OK
    assert L.srt_occluded(ds.h, 0, None, None, None) == abi.SRT_OK
    # n = 1 and n = 257 (one full workgroup and one lane of the next)
    rays = rq.unrelated_rays(flat, 257, seed=3)
    hit, t = rq.oracle_trace(oracle, flat, rays)
    for n in (1, 257):
        o = ds.trace_rays(rays[:n], count=True)
        assert np.array_equal(o["hit_id"], hit[:n]) and np.array_equal(bits(o["t"]), bits(t[:n])), n
        assert o["stats"]["primary_rays"] == n and o["stats"]["hit_rays"] == int((hit[:n] >= 0).sum())
        assert o["stats"]["node_tests_primary"] >= n * flat.n_objects
    # a second handle on the same records
    sh = ds.share()
    o = sh.trace_rays(rays)
    assert np.array_equal(o["hit_id"], hit) and np.array_equal(bits(o["t"]), bits(t))
    sh.close()
    # non-finite rays: the call returns, and gives what the oracle's walk gives
    bad = np.full((257, 6), np.nan, np.float32)
    bad[1::4, 3:6] = np.inf
    bad[2::4, 0:3] = -np.inf
    bhit, bt = rq.oracle_trace(oracle, flat, bad[:8])
    o = ds.trace_rays(bad)
    assert np.array_equal(o["hit_id"][:8], bhit) and np.array_equal(bits(o["t"][:8]), bits(bt))
    assert set(np.unique(ds.occluded(bad))) <= {0, 1}
    assert np.array_equal(ds.trace_rays(rays)["hit_id"], hit), "the scene still answers after the non-finite batch"
    # argument errors, all before anything is touched
    out = np.full(4, -7, np.int32)
    r4 = np.ascontiguousarray(rays[:4])
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, 2 << 8, abi.SRT_FLAG_COUNT_WORK | abi.SRT_FLAG_FRAMES_IN_FLIGHT):
        assert L.srt_trace_rays(ds.h, 4, r4.ctypes.data_as(f32p), flags, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG, flags
        assert L.srt_trace_rays_device(ds.h, 4, None, flags, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays(ds.h, 4, None, 0, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded(ds.h, 4, None, None, np.zeros(4, np.uint8).ctypes.data_as(u8p)) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_device(ds.h, 4, None, 0, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_device(ds.h, 4, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays(None, 4, r4.ctypes.data_as(f32p), 0, out.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
    assert (out == -7).all()
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "ray_query_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"ray query {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_points():
    """Device pointers from torch tensors, a second stream, results equal to the host entry points', and renders around the queries
    that give the frame and the srt_sync statistics they give without them (own process: torch initialises HIP first)."""
    run_case("device")


def test_trace_rays_device_captured_into_a_hip_graph():
    """srt_trace_rays_device captured once into a hipGraph and replayed twice: the same bits (own process, as
    tests/test_gpu_graph_capture.py)."""
    run_case("graph")
