"""GPU (-m gpu): srt_scene_refit_device -- the caller's vertex buffer in device memory, the hierarchy refitted on the device
(include/srt.h, REFIT).

Every case creates the scene, prepares it, refits it from a buffer the device reads, and compares with a SECOND scene made by
srt_scene_create from the tests' own restatement (tests/refit_ref.py: same order, same tree, the new points, refitted boxes, the new
normals): records at the bar of refit_ref.same_records, frames against the oracle run with the device's pow on that flat scene at the
bar of gpu_frames.compare_exact.  The cases of this file hand over pinned host memory (srt_host_alloc), which the device reads in
place; the cases on torch tensors -- vertices made by torch ops, one stream without a host wait, a captured hipGraph -- run in their own
processes (tests/refit_device_case.py, tests/refit_graph_case.py: torch must initialise HIP before the library does)."""
import ctypes as C
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import pose_ref
import ray_query_ref as rq
import refit_ref
import tree_shapes as ts
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 128, 96


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


class DeviceBuffers:
    """Arrays in pinned host memory, which the device reads and writes in place: put(a) copies a in and returns its address (16-byte
    aligned, or `misalign` bytes past such an address); array(shape, dtype, fill) is an output the test reads back after a wait."""

    def __init__(self, srt):
        self.L = srt.load()
        self.ptrs = []

    def array(self, shape, dtype, fill=0, misalign=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.L.srt_host_alloc(n + 16 + misalign)
        assert ptr and ptr % 16 == 0, "srt_host_alloc"
        self.ptrs.append(ptr)
        a = np.frombuffer((C.c_uint8 * max(n, 1)).from_address(ptr + misalign), dtype=dtype, count=int(np.prod(shape))).reshape(shape)
        a[...] = fill
        return a

    def put(self, a, misalign=0):
        a = np.ascontiguousarray(a)
        b = self.array(a.shape, a.dtype, misalign=misalign)
        b[...] = a
        assert b.ctypes.data % 16 == misalign
        return b.ctypes.data

    def free(self):
        for p in self.ptrs:
            self.L.srt_host_free(p)
        self.ptrs = []


@pytest.fixture()
def dev(srt):
    d = DeviceBuffers(srt)
    yield d
    d.free()


def check_refit(srt, oracle, ds, flat0, points, params, normals=None, what=""):
    """ds has been refitted and waited for: its records against a scene created from refit_flat(flat0, points, normals), then every
    frame of `params` against the oracle on that flat scene.  Returns (the flat scene, the pipelines the frames took)."""
    want = refit_ref.refit_flat(flat0, points, normals)
    fresh = srt.DeviceScene(want)
    refit_ref.same_records(ds.records(), fresh.records(), what)
    fresh.close()
    pipes = []
    for p in params:
        o = ds.render(p)
        c = oracle.render(want, p, pow="device")
        gf.compare_exact(srt, o, c, gf.owned(p), want, p, f"{what} L={p.n_lights}")
        if p.flags & abi.SRT_FLAG_COUNT_WORK:
            assert o["stats"]["node_tests"] == c["stats"]["node_tests"] and o["stats"]["tri_tests"] == c["stats"]["tri_tests"], what
        pipes.append(ds.pipeline)
    return want, pipes


def bend(points, k=0.02, amp=6.0, phase=0.3):
    """A deformation no matrix makes: x += amp * sin(k * y + phase), y += amp * cos(k * z), in float32; w stays."""
    p = np.ascontiguousarray(points, np.float32).copy()
    x, y, z = p[..., 0].copy(), p[..., 1].copy(), p[..., 2].copy()
    p[..., 0] = x + np.float32(amp) * np.sin(np.float32(k) * y + np.float32(phase)).astype(np.float32)
    p[..., 1] = y + np.float32(amp) * np.cos(np.float32(k) * z).astype(np.float32)
    return p


# ---- 1. identity with pose ---------------------------------------------------------------------------------------------------------
def test_refit_with_posed_points_leaves_what_pose_leaves(srt, oracle, T, dev):
    """cubes4_a0 at the three orbit angles: a direct refit with xyzw points = M * source leaves, byte for byte, the records
    srt_scene_pose leaves from M; frames at 1, 8 and 16 light samples (the counts at which the shadow pipeline changes), work counted once."""
    g = gu.GoldenScene("cubes4_a0")
    flat = g.flat
    ds = srt.DeviceScene(flat); ds.refit_prepare()
    posed = srt.DeviceScene(flat); posed.set_pose_source()
    pipes = []
    for k, a in enumerate(pose_ref.ORBIT_ANGLES):
        mats = np.tile(pose_ref.orbit_matrix(T, a), (flat.n_objects, 1))
        pts = pose_ref.transform_objects(flat, mats)
        ds.refit_device(dev.put(pts), stride=4); ds.sync()
        posed.pose(mats); posed.sync()
        refit_ref.same_bytes(ds.records(), posed.records(), f"refit against pose, {a} deg")
        ps = [g.params(W, H, L, flags=abi.SRT_FLAG_COUNT_WORK if (k == 0 and L == 8) else 0) for L in ((1, 8, 16) if k == 0 else (2,))]
        pipes += check_refit(srt, oracle, ds, flat, pts, ps, what=f"four cubes {a} deg")[1]
    assert len(set(pipes)) > 1, pipes
    ds.close(); posed.close()


# ---- 3. normals ----------------------------------------------------------------------------------------------------------------------
def test_normals_indexed_direct_and_unchanged(srt, oracle, dev):
    """The bunny over its slab with vertex normals, shaded with SRT_FLAG_SMOOTH_NORMALS: indexed normals (n_verts x 3) are gathered into
    the rows in point order, direct normals (n_tris x 9) are copied, no normals leave the rows as they were."""
    g = gu.GoldenScene("ground_bunny")
    verts, tv = refit_ref.weld(g.flat)
    nV = verts.shape[0]
    c = verts[:, :3].mean(0)
    def away(v, push):
        n = v - c + np.float32(push)
        return np.ascontiguousarray(n / np.linalg.norm(n, axis=1, keepdims=True), np.float32)
    vn0 = away(verts[:, :3], (0.0, 0.0, -40.0))
    flat = dataclasses.replace(g.flat, tri_normals=refit_ref.expand_normals(vn0, tv))
    ds = srt.DeviceScene(flat); ds.refit_prepare(tv, nV)
    ps = [g.params(W, H, 2, flags=abi.SRT_FLAG_SMOOTH_NORMALS), g.params(W, H, 1)]
    # indexed, stride 3, normals per vertex
    v1 = bend(verts)
    vn1 = away(v1[:, :3], (0.0, 30.0, -10.0))
    ds.refit_device(dev.put(v1[:, :3]), stride=3, n_verts=nV, normals=dev.put(vn1)); ds.sync()
    pts1 = refit_ref.expand(v1[:, :3], tv, 3)
    n1 = refit_ref.expand_normals(vn1, tv)
    assert np.array_equal(refit_ref.bits(ds.records()["tri_normals"]), refit_ref.bits(n1))
    check_refit(srt, oracle, ds, flat, pts1, ps, n1, "indexed normals")
    # points move again, no normals: the rows stay
    v2 = bend(verts, phase=1.1)
    ds.refit_device(dev.put(v2), stride=4, n_verts=nV); ds.sync()
    assert np.array_equal(refit_ref.bits(ds.records()["tri_normals"]), refit_ref.bits(n1))
    check_refit(srt, oracle, ds, flat, refit_ref.expand(v2, tv, 4), ps[:1], n1, "normals unchanged")
    # direct: a row per triangle, nothing shared between triangles
    rng = np.random.default_rng(3)
    n3 = n1 + rng.uniform(-0.05, 0.05, n1.shape).astype(np.float32)
    pts3 = refit_ref.expand(v1, tv, 4)
    ds.refit_device(dev.put(pts3[..., :3]), stride=3, normals=dev.put(n3)); ds.sync()
    assert np.array_equal(refit_ref.bits(ds.records()["tri_normals"]), refit_ref.bits(n3))
    check_refit(srt, oracle, ds, flat, refit_ref.direct(pts3[..., :3], 3), ps[:1], n3, "direct normals")
    ds.close()


# ---- 4. small and odd shapes -----------------------------------------------------------------------------------------------------------
def shape_flat(name):
    return pose_ref.one_triangle_scene() if name == "one_triangle" else ts.family(name)


@pytest.mark.parametrize("name", ["one_triangle", "comb255", "sliced", "roots300"])
def test_small_and_odd_shapes(srt, oracle, dev, name):
    """one_triangle: an empty leaf, 13 triangles in all (no multiple of 64); comb255: the deepest tree the schedule admits; sliced:
    leaves of up to 31 triangles; roots300: 300 objects of one node.  Direct xyz, then indexed xyzw, both at an address that is only float-aligned."""
    flat = shape_flat(name)
    verts, tv = refit_ref.weld(flat)
    assert flat.n_tris % 64 != 0
    p = abi.make_params(240, 160, abi.light_staircase((120.0, -260.0, -40.0), 2), flags=abi.SRT_FLAG_COUNT_WORK) if name == "one_triangle" \
        else ts.frame_params(2, flags=abi.SRT_FLAG_COUNT_WORK)
    ds = srt.DeviceScene(flat); ds.refit_prepare(tv, verts.shape[0])
    pts = bend(flat.tri_points, k=0.05, amp=2.0)
    assert (pts[..., 3] == 1.0).all()
    ds.refit_device(dev.put(pts[..., :3], misalign=4), stride=3); ds.sync()
    want, _ = check_refit(srt, oracle, ds, flat, refit_ref.direct(pts[..., :3], 3), [p], what=f"{name} direct xyz")
    if name == "one_triangle":
        nodes, _ = pose_ref.split_boxes(ds.records(), "nodes")
        assert (nodes[:, 0] == pose_ref.FLT_MAX).any() and (nodes[:, 3] == -pose_ref.FLT_MAX).any(), "the empty leaf keeps the start values"
    v2 = bend(verts, k=0.03, amp=3.0, phase=2.0)
    ds.refit_device(dev.put(v2, misalign=4), stride=4, n_verts=verts.shape[0]); ds.sync()          # float-aligned: the 4-byte loads
    check_refit(srt, oracle, ds, flat, refit_ref.expand(v2, tv, 4), [p], what=f"{name} indexed xyzw")
    ds.close()


def test_comb256_is_beyond_the_refit_limit(srt, oracle):
    """A tree of height 256: srt_scene_refit_prepare refuses it with SRT_ERR_LIMIT, a refit without preparation is SRT_ERR_ARG, and
    the scene renders the same frame afterwards."""
    flat = ts.family("comb256")
    ds = srt.DeviceScene(flat)
    p = ts.frame_params(2)
    before = ds.render(p)
    with pytest.raises(srt.SrtError) as e:
        ds.refit_prepare()
    assert e.value.code == abi.SRT_ERR_LIMIT
    with pytest.raises(srt.SrtError) as e:
        ds.refit_device(4096, stride=4)                          # (an address nobody reads: the call is refused first)
    assert e.value.code == abi.SRT_ERR_ARG
    after = ds.render(p)
    c = oracle.render(flat, p, pow="device")
    gf.compare_exact(srt, after, c, gf.owned(p), flat, p, "comb256 after the refused calls")
    for k in ("hit_id", "rgb8"):
        assert np.array_equal(before[k], after[k]), k
    ds.close()


# ---- 6. queries see the refit ------------------------------------------------------------------------------------------------------------
def test_queries_see_the_refit(srt, oracle, dev):
    """192 x 108 rays after a refit of ground_bunny: srt_trace_rays_device against the oracle's camera-mode frame of the refitted flat
    scene, srt_occluded_device on the hits' shadow rays against the oracle's two-frame read-out."""
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    verts, tv = refit_ref.weld(flat)
    QW, QH, focal, light = 192, 108, 40.0, rq.SHADOW_LIGHT["ground_bunny"]
    rays = rq.frame_rays(QW, QH, rq.SHEAR, focal)
    n = rays.shape[0]
    ds = srt.DeviceScene(flat); ds.refit_prepare(tv, verts.shape[0])
    before = ds.trace_rays(rays)
    v1 = bend(verts, amp=12.0)
    ds.refit_device(dev.put(v1[:, :3]), stride=3, n_verts=verts.shape[0])          # asynchronous on the scene's own stream: the queries are ordered behind it
    want = refit_ref.refit_flat(flat, refit_ref.expand(v1[:, :3], tv, 3))
    hit, t, shadowed, usable = rq.shadow_readout(oracle, want, QW, QH, rq.SHEAR, focal, light)
    sel = usable                                               # the read-out shows a shadow only where the unshadowed colour is not zero
    assert sel.sum() >= 0.95 * (hit >= 0).sum() and 0.1 * n < sel.sum() < 0.9 * n
    d_hit, d_t, d_bary = dev.array((n,), np.int32, -5), dev.array((n,), np.float32, -1.0), dev.array((n, 3), np.float32, -1.0)
    ds.trace_rays_device(n, dev.put(rays), hit_id=d_hit.ctypes.data, t=d_t.ctypes.data, bary=d_bary.ctypes.data)
    sray = rq.shadow_rays(rays[sel], t[sel], light)
    skip = want.tri_obj[hit[sel]].astype(np.int32)
    m = sray.shape[0]
    d_occ = dev.array((m,), np.uint8, 7)
    ds.occluded_device(m, dev.put(sray), d_occ.ctypes.data, skip_obj=dev.put(skip))
    ds.records()                                               # (waits for the device: srt_sync waits for renders only)
    bad = d_hit != hit
    assert not bad.any(), f"{int(bad.sum())} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(refit_ref.bits(d_t), refit_ref.bits(t))
    assert not np.array_equal(before["hit_id"], d_hit), "the refit moves what the rays see"
    assert set(np.unique(d_occ)) <= {0, 1}
    bad = d_occ.astype(bool) != shadowed[sel]
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} shadow rays differ from the oracle's frames"
    assert 0 < shadowed[sel].sum() < m
    ds.close()


# ---- 7. sharing and errors ---------------------------------------------------------------------------------------------------------------
def test_shared_handle_pose_after_refit_update_and_argument_errors(srt, oracle, T, dev):
    g = gu.GoldenScene("cubes4_a0")
    flat = g.flat
    verts, tv = refit_ref.weld(flat)
    nV = verts.shape[0]
    p = g.params(W, H, 2)
    ds = srt.DeviceScene(flat)
    d_pts, d_verts = dev.put(bend(flat.tri_points)), dev.put(bend(verts))
    created = ds.records()

    def refused(code, what, **kw):
        with pytest.raises(srt.SrtError) as e:
            ds.refit_device(**kw)
        assert e.value.code == code, what
    def prepare_refused(code, what, *a):
        with pytest.raises(srt.SrtError) as e:
            ds.refit_prepare(*a)
        assert e.value.code == code, what

    refused(abi.SRT_ERR_ARG, "not prepared", points=d_pts, stride=4)
    bad = tv.copy(); bad[-1, 2] = nV
    prepare_refused(abi.SRT_ERR_LAYOUT, "an index equal to n_verts", bad, nV)
    prepare_refused(abi.SRT_ERR_LAYOUT, "indices with n_verts 0", tv, 0)
    refused(abi.SRT_ERR_ARG, "a refused preparation prepares nothing", points=d_pts, stride=4)
    ds.refit_prepare()                                          # the direct form only
    refused(abi.SRT_ERR_ARG, "indexed form without prepared indices", points=d_verts, stride=4, n_verts=nV)
    ds.refit_prepare(tv, nV)
    refused(abi.SRT_ERR_ARG, "NULL points", points=0, stride=4)
    refused(abi.SRT_ERR_ARG, "stride 2", points=d_pts, stride=2)
    refused(abi.SRT_ERR_ARG, "stride 5", points=d_pts, stride=5)
    refused(abi.SRT_ERR_ARG, "stride 0", points=d_pts, stride=0)
    refused(abi.SRT_ERR_ARG, "normals on a scene created without", points=d_pts, stride=4, normals=d_pts)
    refused(abi.SRT_ERR_LAYOUT, "another n_verts", points=d_verts, stride=4, n_verts=nV - 1)
    refused(abi.SRT_ERR_LAYOUT, "another n_verts", points=d_verts, stride=4, n_verts=nV + 1)
    L_ = srt.load()
    assert L_.srt_scene_refit_device(ds.h, None, None) == abi.SRT_ERR_ARG
    ds.sync()
    refit_ref.same_bytes(ds.records(), created, "refused calls change nothing")
    # a refit through a shared handle rewrites the records every handle reads; the preparation belongs to the records
    sh = ds.share()
    sh.refit_device(d_verts, stride=4, n_verts=nV); sh.sync()
    pts = refit_ref.expand(bend(verts), tv, 4)
    want = refit_ref.refit_flat(flat, pts)
    fresh = srt.DeviceScene(want)
    refit_ref.same_records(sh.records(), fresh.records(), "shared handle")
    for h in (ds, sh):
        gf.compare_exact(srt, h.render(p), oracle.render(want, p, pow="device"), gf.owned(p), want, p, "shared handle")
    sh.close()
    # a pose after a refit applies to the pose source, not to the refitted points; the preparation survives it
    ds.set_pose_source()
    mats = np.tile(pose_ref.orbit_matrix(T, 3.0), (flat.n_objects, 1))
    ds.pose(mats); ds.sync()
    posed = pose_ref.pose_flat(flat, mats)
    fp = srt.DeviceScene(posed)
    refit_ref.same_records(ds.records(), fp.records(), "pose after refit")
    fp.close()
    ds.refit_device(d_pts, stride=4); ds.sync()
    check_refit(srt, oracle, ds, flat, bend(flat.tri_points), [p], what="refit after pose")
    # srt_scene_update discards the preparation ...
    ds.update(want); ds.sync()
    refused(abi.SRT_ERR_ARG, "update discards the preparation", points=d_pts, stride=4)
    refit_ref.same_records(ds.records(), fresh.records(), "a refused refit changes nothing")
    fresh.close()
    # ... and a new one serves the updated scene
    ds.refit_prepare()
    ds.refit_device(d_pts, stride=4); ds.sync()
    check_refit(srt, oracle, ds, want, bend(flat.tri_points), [p], what="refit after update")
    ds.close()


# ---- 2, 5, 8: torch tensors, in their own processes ----------------------------------------------------------------------------------------
def run_case(script, mode, ok):
    r = subprocess.run([sys.executable, os.path.join(HERE, script)] + ([mode] if mode else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and ok in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_vertices_made_by_torch_ops():
    """ground_bunny welded, displaced by a non-affine torch expression on the device: indexed xyz and xyzw, direct xyz at an address
    with data_ptr() % 16 == 4 and 16-byte aligned; twice the same bits."""
    run_case("refit_device_case.py", "torch", "refit torch case: ok")


def test_write_refit_render_twice_on_one_stream_without_a_host_wait():
    run_case("refit_device_case.py", "stream", "refit stream case: ok")


def test_refit_and_renders_captured_into_a_hip_graph_replay_bit_exact():
    run_case("refit_graph_case.py", None, "refit graph case: ok")
