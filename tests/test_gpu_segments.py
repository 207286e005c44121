"""GPU (-m gpu): srt_closest_segments and its _device form (include/srt_segments.h) on whole scenes -- the golden cube and ground_bunny and
the trees of tests/tree_shapes.py -- every output bit for bit against tests/segment_ref.py, the work counts included, at 1, 63, 64, 65
and 257 segments.  The segments of a case are points, random segments up to half the scene's extent, axis-parallel and in-plane ones
(not sloped), crossings through a triangle's interior and through the middle of an edge, and segments that leave from beside a vertex;
tests/test_segment_ref.py shows which cases they reach."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import pose_ref
import segment_ref as sr
import test_gpu_points as tp
import tree_shapes as ts

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32
SCENES = tp.SCENES
COUNTS = (1, 63, 64, 65, 257)
N = max(COUNTS)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def segments_for(flat, n, seed):
    """n segments of eight kinds in turn (i % 8) and the scene's extent:
    0 a point beside a vertex; 1 from beside a vertex in a random direction; 2 anywhere in and around the box; 3 parallel to an axis;
    4 through the middle of a triangle's edge 1-2, along the normal; 5 leaving from beside a vertex, away from the scene's centre;
    6 through a triangle's centroid, along the normal; 7 with d.z == 0."""
    rng = np.random.default_rng(seed)
    T = np.ascontiguousarray(flat.tri_points, F)[..., :3].astype(np.float64)             # n_tris x 3 x 3
    P = T.reshape(-1, 3)
    ok = np.isfinite(T).all((1, 2))
    mn, mx = P[np.isfinite(P).all(1)].min(0), P[np.isfinite(P).all(1)].max(0)
    ext = float(np.linalg.norm(mx - mn))
    centre = 0.5 * (mn + mx)
    seg = np.zeros((n, 6))
    good = np.flatnonzero(ok)
    for i in range(n):
        tri = T[good[rng.integers(0, good.size)]]
        V = tri[rng.integers(0, 3)]
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        L = ext * 0.5 * rng.uniform(0.0, 1.0) ** 2
        nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        nrm = nrm / np.linalg.norm(nrm) if np.linalg.norm(nrm) > 0 else u
        kind = i % 8
        if kind == 0:
            A = V + rng.normal(0.0, 0.01 * ext, 3); B = A
        elif kind == 1:
            A = V + rng.normal(0.0, 0.01 * ext, 3); B = A + u * L
        elif kind == 2:
            A = mn + (mx - mn) * rng.uniform(-0.3, 1.3, 3); B = A + u * L
        elif kind == 3:
            A = mn + (mx - mn) * rng.uniform(-0.1, 1.1, 3); B = A.copy(); B[rng.integers(0, 3)] += L * rng.choice([-1.0, 1.0])
        elif kind == 4:
            M = 0.5 * (tri[0] + tri[1]); h = ext * 2.0 ** -rng.integers(3, 8); A = M + nrm * h; B = M - nrm * h
        elif kind == 5:
            o = V - centre; o = o / np.linalg.norm(o) if np.linalg.norm(o) > 0 else u
            h = ext * 2.0 ** -rng.integers(4, 9); A = V + o * h; B = V + o * (h + L)
        elif kind == 6:
            M = tri.mean(0); h = ext * 2.0 ** -rng.integers(3, 8); A = M + nrm * h; B = M - nrm * (h * rng.uniform(0.0, 2.0))
        else:
            A = V + rng.normal(0.0, 0.01 * ext, 3); B = A + u * L; B[2] = A[2]
        seg[i, :3], seg[i, 3:] = A, B
    return seg.astype(F), ext


def tie_segments(flat):
    """On the cube, whose coordinates are exact: through the middle of the diagonal two triangles of a face share, straight along the face's
    normal (both cross at t = 1/2: dist2 +0 twice), and from beside a corner straight away from it (every triangle at the corner has the
    corner as its closest point)."""
    T = np.ascontiguousarray(flat.tri_points, F)[..., :3].astype(np.float64)
    out = []
    for tri in T[:4]:
        nrm = np.cross(tri[1] - tri[0], tri[2] - tri[0]); nrm /= np.linalg.norm(nrm)
        for a, b in ((0, 1), (1, 2), (0, 2)):
            M = 0.5 * (tri[a] + tri[b])
            out.append(np.r_[M + nrm * 0.25, M - nrm * 0.25])
    centre = T.reshape(-1, 3).mean(0)
    for V in T[:4, 0]:
        o = np.sign(V - centre)
        out.append(np.r_[V + o * 0.125, V + o * 0.5])
        out.append(np.r_[V + o * 0.5, V + o * 0.125])
    return np.asarray(out).astype(F)


def radii_for(ext, n, seed, unbounded):
    """n radii between a 300th and a third of the scene's extent; `unbounded` of them +inf, two that walk nothing."""
    return tp.radii_for(ext, n, seed + 1, unbounded)


@functools.lru_cache(maxsize=None)
def case(name):
    """(flat, segments, radii, the yardstick's result) of a scene, made once and never changed.  The cube's first segments are the ties."""
    flat = tp.flat_of(name)
    seg, ext = segments_for(flat, N, 23)
    if name == "cube":
        ties = tie_segments(flat)
        seg[8:8 + len(ties)] = ties
    rad = radii_for(ext, N, 23, 4 if name == "ground_bunny" else 48)
    return flat, seg, rad, sr.closest_segments(flat, seg, rad)


@pytest.mark.parametrize("name", SCENES)
def test_against_the_yardstick(srt, name):
    flat, seg, rad, want = case(name)
    assert 0.15 * N < want["hits"] < N, want["hits"]
    ds = srt.DeviceScene(flat)
    for n in COUNTS:
        w = sr.first(want, n)
        got = ds.closest_segments(seg[:n], radius=rad[:n], count=True)
        sr.same(got, w, f"{name}, {n} segments")
        sr.same_counts(got["stats"], w, n, f"{name}, {n} segments")
        plain = ds.closest_segments(seg[:n], radius=rad[:n])
        sr.same(plain, w, f"{name}, {n} segments, no counting")
        assert plain["stats"]["hit_rays"] == w["hits"] and plain["stats"]["node_tests_primary"] == 0
    print(name, "segments", N, "found", want["hits"], "node tests", want["node_tests"], "triangle tests", want["tri_tests"],
          "features", np.bincount(want["feature"][want["tri"] >= 0], minlength=6).tolist())
    # any output may be NULL; another order of the segments gives the same rows in that order
    only = ds.closest_segments(seg, radius=rad, want=("s",))
    assert set(only) == {"s", "stats"} and np.array_equal(only["s"].view(np.uint32), want["s"].view(np.uint32))
    assert ds.closest_segments(seg, radius=rad, want=())["stats"]["hit_rays"] == want["hits"]
    perm = np.random.default_rng(3).permutation(N)
    sr.same(ds.closest_segments(seg[perm], radius=rad[perm]), {k: want[k][perm] for k in sr.SAME_KEYS}, name + ", permuted")
    ds.close()


@pytest.mark.parametrize("name", ["cube", "sliced", "roots33", "comb256", "loose"])
def test_without_a_radius(srt, name):
    """radius NULL is +inf for every segment: every node passes (box test 2 needs a finite radius), every triangle is a candidate, and the
    winner is brute force."""
    flat, seg, _, _ = case(name)
    want = sr.closest_segments(flat, seg)
    assert want["node_tests"] == N * flat.n_nodes and want["tri_tests"] == N * flat.n_tris
    brute, _ = sr.brute_force(flat, seg[:65])
    sr.same(sr.first(want, 65), brute, name + ", brute force")
    ds = srt.DeviceScene(flat)
    got = ds.closest_segments(seg, count=True)
    sr.same(got, want, name)
    sr.same_counts(got["stats"], want, N, name)
    sr.same(ds.closest_segments(seg, radius=np.inf), want, name + ", one radius for all")
    ds.close()


@pytest.mark.parametrize("name", ["cube", "sliced", "loose", "ground_bunny"])
def test_point_segments(srt, name):
    """B = A: srt_closest_points' tri, dist2, point and vw and both counters, on the device, with s = 0 and feature = 0."""
    flat, pts, rad, _ = tp.case(name)
    ds = srt.DeviceScene(flat)
    want = ds.closest_points(pts, radius=rad, count=True)
    got = ds.closest_segments(np.concatenate([pts, pts], 1), radius=rad, count=True)
    for k in ("tri", "dist2", "point", "vw"):
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    assert got["stats"] == want["stats"], (got["stats"], want["stats"])
    assert (got["s"].view(np.uint32) == 0).all() and (got["feature"] == 0).all()
    assert 0 < want["stats"]["hit_rays"] < len(pts)
    ds.close()


@pytest.mark.parametrize("name,hide", [("sliced", 1), ("sliced", 0), ("roots33", 32), ("comb256", 0)])
def test_masks(srt, name, hide):
    objects = {"sliced": ts.sliced_objects, "roots33": lambda: ts.roots_objects(33), "comb256": lambda: ts.comb_objects(256)}[name]()
    full, less, ids = tp.reduced(objects, hide)
    _, seg, rad, want = case(name)
    ds = srt.DeviceScene(full)
    # all ones, by a table never set, a table of ones and masks of ones: the unmasked call's bits and counts
    for table in (None, np.full(full.n_objects, 0xFFFFFFFF, np.uint32)):
        if table is not None:
            ds.set_object_masks(table)
        for sm in (True, np.full(N, 0xFFFFFFFF, np.uint32)):
            got = ds.closest_segments(seg, radius=rad, seg_mask=sm, count=True)
            sr.same(got, want, f"{name}, all ones")
            sr.same_counts(got["stats"], want, N, f"{name}, all ones")
    # object `hide` hidden from every segment: the reduced scene's result, its ids renumbered
    om = np.where(np.arange(full.n_objects) == hide, 2, 1 | (4 << (np.arange(full.n_objects) % 8))).astype(np.uint32)
    ds.set_object_masks(om)
    small = sr.closest_segments(less, seg, rad)
    w = dict(small, tri=np.where(small["tri"] >= 0, ids[np.maximum(small["tri"], 0)], -1).astype(np.int32))
    masked = sr.closest_segments(full, seg, rad, seg_mask=np.full(N, 1, np.uint32), obj_mask=om)
    sr.same(masked, w, "the yardstick's masks against the reduced scene")
    assert (masked["node_tests"], masked["tri_tests"]) == (small["node_tests"], small["tri_tests"])
    got = ds.closest_segments(seg, radius=rad, seg_mask=np.full(N, 1, np.uint32), count=True)
    sr.same(got, w, f"{name}, object {hide} hidden")
    sr.same_counts(got["stats"], w, N, f"{name}, object {hide} hidden")
    assert not np.isin(got["tri"], np.flatnonzero(full.tri_obj == hide)).any()
    # a mask per segment: some see everything, some all but `hide`, some only `hide`, some nothing
    sm = np.resize(np.uint32([0xFFFFFFFF, 1, 2, 0, 4, 8]), N)
    w = sr.closest_segments(full, seg, rad, seg_mask=sm, obj_mask=om)
    got = ds.closest_segments(seg, radius=rad, seg_mask=sm, count=True)
    sr.same(got, w, f"{name}, a mask per segment")
    sr.same_counts(got["stats"], w, N, f"{name}, a mask per segment")
    assert (got["tri"][sm == 0] == -1).all()
    # the unmasked call ignores the table
    sr.same(ds.closest_segments(seg, radius=rad), want, f"{name}, unmasked beside a table")
    ds.close()


@pytest.mark.parametrize("name", ["sliced", "roots33", "ground_bunny"])
def test_after_pose(srt, name):
    """srt_scene_pose moves the records the query reads: the yardstick on pose_ref's flat scene."""
    flat, seg, rad, before = case(name)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = np.stack([tp.turn(k, flat.n_objects) for k in range(flat.n_objects)])
    ds.pose(mats)                                               # asynchronous on the scene's own stream: the query is ordered behind it
    got = ds.closest_segments(seg, radius=rad, count=True)
    moved = pose_ref.pose_flat(flat, mats)
    want = sr.closest_segments(moved, seg, rad)
    sr.same(got, want, name + ", posed")
    sr.same_counts(got["stats"], want, N, name + ", posed")
    assert not np.array_equal(want["tri"], before["tri"]) or not np.array_equal(want["dist2"], before["dist2"])
    ds.close()


def run_case(mode):
    r = subprocess.run([sys.executable, os.path.join(HERE, "segments_device_case.py"), mode], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"segments {mode} case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_device_entry_point():
    """Device pointers from torch tensors: a second stream beside a pending render, the host form's bits, NULL outputs one by one,
    float-aligned pointers, a mask per segment, a shared handle (own process: torch initialises HIP first)."""
    run_case("device")


def test_after_refit_device():
    """srt_scene_refit_device from a torch tensor, then the query on the same stream: the yardstick on the moved flat scene."""
    run_case("refit")


def test_captured_into_a_hip_graph():
    """srt_closest_segments_device captured once into a hipGraph and replayed twice: the same bits."""
    run_case("graph")
