"""GPU (-m gpu): the visibility masks (include/srt.h, "Visibility masks") -- srt_scene_set_object_masks, srt_trace_rays_masked,
srt_occluded_masked, srt_shade_paths_masked and srt_render_paths_masked pinned bit for bit by tests/visibility_ref.py, a filter on the
candidate sets of tests/ray_range_ref.py (tests/test_visibility_ref.py pins that filter to the oracle on the reduced scene and checks
every case's input conditions on the yardstick alone).  Floats compare by bits; where the yardstick is NaN the device must be NaN."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ray_range_ref as rr
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh
import surface_ref as sf
import tree_shapes as ts
import visibility_ref as vr
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = vr.ALL
TMIN, DEPTH = vr.BOUNCE_T_MIN, vr.DEPTH
RULES = {"None": None, "ENDED": sh.ENDED}
COUNTERS = ("node_tests_primary", "tri_tests_primary")
bits = sf.bits


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def same_trace(got, hit, t, what, bary=None):
    assert np.array_equal(got["hit_id"], hit), (what, "hit ids")
    assert np.array_equal(bits(got["t"]), bits(t)), (what, "t")
    if bary is not None:
        assert np.array_equal(bits(got["bary"]), bits(bary)), (what, "bary")


def cut(ref, sel):
    return {k: (v[sel] if k in ("rgb_linear", "rgb8") else v[:, sel]) for k, v in ref.items() if k in sp.ALL_KEYS}


# ---- 1. closest hit and occlusion under per-ray masks ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["cubes4_a40", "ground_bunny"])
def test_closest_and_occlusion_under_ray_masks(srt, oracle, name):
    flat, rays, _, _ = sh.lamp_case(name)
    n = rays.shape[0]
    c = vr.case_candidates(oracle, name)
    table = vr.case_table(flat)
    masks, kind = vr.ray_masks(name, n)
    assert (masks[1:] != masks[:-1]).all()
    tr, _, _ = rr.mixed_intervals(c, seed=3)
    # skip_obj on top of the masks: the hidden object itself (object 1), the one before it and the one after it (in a scene of two: nothing)
    skip = np.array([1, 0, 2, -1], np.int32)[np.arange(n) % 4]
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    for label, t_range in (("no interval", None), ("mixed intervals", tr)):
        hit, t = vr.closest(c, flat, masks, table, t_range)
        assert (hit >= 0).any() and (hit[kind == 0] < 0).all() and (hit[kind == 2] < 0).all()
        for count in (False, True):
            o = ds.trace_rays(rays, t_range=t_range, ray_mask=masks, count=count)
            same_trace(o, hit, t, (name, label, count), rr.want_bary(oracle, flat, rays, hit, t))
            assert o["stats"]["hit_rays"] == int((hit >= 0).sum())
        for sk in (None, skip):
            want = vr.occluded(c, flat, masks, table, t_range, sk)
            assert 0 < want.sum() < n and not want[kind == 0].any() and not want[kind == 2].any()
            assert np.array_equal(ds.occluded(rays, sk, t_range=t_range, ray_mask=masks), want), (name, label, sk is not None)
    assert not np.array_equal(vr.occluded(c, flat, masks, table, None, skip), vr.occluded(c, flat, masks, table, None, None)), "skip_obj changes nothing"
    ds.close()


# ---- 2. tree shapes ------------------------------------------------------------------------------------------------------------------------
def shape_masks(name, flat, n):
    """(table, per-ray masks) of a tree-shape family."""
    k = np.arange(flat.n_objects, dtype=np.uint32)
    i = np.arange(n)
    if name == "roots33":
        # object k has bit k % 32 (objects 0 and 32 share one); single bits, a block mask hiding objects 0..15, a mask hiding the last object
        table = (np.uint32(1) << (k % np.uint32(32))).astype(np.uint32)
        single = (np.uint32(1) << (i % 32).astype(np.uint32)).astype(np.uint32)
        masks = np.select([i % 4 == 0, i % 4 == 1, i % 4 == 2], [single, np.uint32(0xFFFF0000), np.uint32(ALL & ~1)], np.uint32(ALL)).astype(np.uint32)
    elif name == "roots300":
        # bits 0 / 1: alternate objects; bits 2 / 3: alternate runs of 40 objects
        table = ((np.uint32(1) << (k % np.uint32(2))) | (np.uint32(4) << ((k // np.uint32(40)) % np.uint32(2)))).astype(np.uint32)
        masks = np.array([1, 4, 2, 8, ALL, 0, 5], np.uint32)[i % 7]
    else:
        # object k has bit k; the first object hidden, everything, the second object hidden
        table = (np.uint32(1) << k).astype(np.uint32)
        masks = np.array([ALL & ~1, ALL, ALL & ~2], np.uint32)[i % 3]
    return table, masks


@gpu
@pytest.mark.parametrize("name", ["roots33", "roots300", "sliced", "shuffled", "ties"])
def test_tree_shapes(srt, oracle, name):
    flat, rays = ts.family(name), np.ascontiguousarray(ts.ray_batch(name))
    n = rays.shape[0]
    assert n % 64
    c = rr.candidates(oracle, flat, rays)
    table, masks = shape_masks(name, flat, n)
    h0, t0 = rr.closest(c)
    hit, t = vr.closest(c, flat, masks, table)
    assert (hit != h0).any() and (hit >= 0).any()
    if name in ("sliced", "shuffled"):
        assert flat.node_count.max() > 8, "no leaf is taken in slices"
        first_hidden = masks == (ALL & ~1)
        assert (flat.tri_obj[h0[first_hidden & (h0 >= 0)]] == 0).any() and not (flat.tri_obj[hit[first_hidden & (hit >= 0)]] == 0).any()
    if name == "ties":
        # hiding the object that owns the lower id of a tie hands the hit to the other object, at the same t
        moved = (masks == (ALL & ~1)) & (h0 >= 0) & (flat.tri_obj[np.maximum(h0, 0)] == 0) & (hit >= 0)
        assert moved.any() and (flat.tri_obj[hit[moved]] == 1).all() and np.array_equal(bits(t[moved]), bits(t0[moved]))
    tr, _, _ = rr.mixed_intervals(c, seed=9)
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    for count in (False, True):
        same_trace(ds.trace_rays(rays, ray_mask=masks, count=count), hit, t, (name, count), rr.want_bary(oracle, flat, rays, hit, t))
    same_trace(ds.trace_rays(rays, ray_mask=masks, t_range=tr, want=("hit_id", "t")), *vr.closest(c, flat, masks, table, tr), (name, "intervals"))
    skip = (np.arange(n) % max(flat.n_objects, 2)).astype(np.int32)
    assert np.array_equal(ds.occluded(rays, ray_mask=masks), vr.occluded(c, flat, masks, table))
    assert np.array_equal(ds.occluded(rays, skip, t_range=tr, ray_mask=masks), vr.occluded(c, flat, masks, table, tr, skip))
    ds.close()


# ---- 3. the reduced scene on the device: a hidden tree is not walked ----------------------------------------------------------------------
def reduced_scene_case(srt, flat, rays, c, hide):
    table, m = vr.hidden(flat, *hide)
    sub, ids = vr.sub_scene(flat, [k for k in range(flat.n_objects) if k not in hide])
    small = srt.DeviceScene(sub)
    want = small.trace_rays(rays, count=True)
    small.close()
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    for masks in (np.full(rays.shape[0], m, np.uint32),):
        got = ds.trace_rays(rays, ray_mask=masks, count=True)
        same_trace(got, vr.map_back(want["hit_id"], ids), want["t"], hide)
        same_trace(got, *vr.closest(c, flat, m, table), hide)
        assert all(got["stats"][k] == want["stats"][k] and got["stats"][k] > 0 for k in COUNTERS), (hide, got["stats"], want["stats"])
    # hidden through the table instead of the ray mask: the same walk
    off = np.full(flat.n_objects, ALL, np.uint32); off[list(hide)] = 0
    ds.set_object_masks(off)
    got = ds.trace_rays(rays, ray_mask=True, count=True)
    same_trace(got, vr.map_back(want["hit_id"], ids), want["t"], hide)
    assert all(got["stats"][k] == want["stats"][k] for k in COUNTERS), (hide, got["stats"], want["stats"])
    # every object hidden: every ray misses and nothing is tested
    ds.set_object_masks(np.zeros(flat.n_objects, np.uint32))
    none = ds.trace_rays(rays, ray_mask=True, count=True)
    assert (none["hit_id"] == -1).all() and np.isposinf(none["t"]).all() and all(none["stats"][k] == 0 for k in COUNTERS) and none["stats"]["hit_rays"] == 0
    assert not ds.occluded(rays, ray_mask=True).any()
    ds.close()


@gpu
@pytest.mark.parametrize("hide", [(0,), (1,), (2,), (3,)])
def test_the_reduced_scene_on_the_device(srt, oracle, hide):
    flat, rays, _, _ = sh.lamp_case("cubes4_a40")
    reduced_scene_case(srt, flat, rays, vr.case_candidates(oracle, "cubes4_a40"), hide)


@gpu
def test_the_reduced_scene_of_many_roots(srt, oracle):
    flat, rays = ts.family("roots33"), np.ascontiguousarray(ts.ray_batch("roots33"))
    reduced_scene_case(srt, flat, rays, rr.candidates(oracle, flat, rays), (5, 7))       # (bit k % 32: neither shares its bit with a kept object)


# ---- 4. identities ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_identities_of_the_ray_queries(srt, oracle):
    name = "cubes4_a40"
    flat, rays, _, _ = sh.lamp_case(name)
    n = rays.shape[0]
    tr, _, _ = rr.mixed_intervals(vr.case_candidates(oracle, name), seed=3)
    skip = (np.arange(n) % 5 - 1).astype(np.int32)
    ds = srt.DeviceScene(flat)
    for table in ("never set", np.full(flat.n_objects, ALL, np.uint32)):
        if not isinstance(table, str):
            ds.set_object_masks(table)
        for t_range in (None, tr):
            plain = ds.trace_rays(rays, t_range=t_range, count=True)
            occ = ds.occluded(rays, skip, t_range=t_range)
            for ray_mask in (True, np.full(n, ALL, np.uint32)):
                got = ds.trace_rays(rays, t_range=t_range, ray_mask=ray_mask, count=True)
                same_trace(got, plain["hit_id"], plain["t"], "identity", plain["bary"])
                assert got["stats"] == plain["stats"], (got["stats"], plain["stats"])
                assert np.array_equal(ds.occluded(rays, skip, t_range=t_range, ray_mask=ray_mask), occ)
    ds.close()


def raw_masked_paths(ds, rays, p, refl, rule, vis):
    """srt_shade_paths_masked through the C ABI, so that vis may be NULL: (rgb_linear, rgb8, seg_hit_id)."""
    r = np.ascontiguousarray(rays, np.float32)
    n = r.shape[0]
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lin, rgb8, hit = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8), np.empty((DEPTH, n), np.int32)
    k = np.ascontiguousarray(refl, np.float32)
    pd, po, st = abi.PathDesc(DEPTH, TMIN, k.ctypes.data), abi.PathOut(), abi.Stats()
    po.hit_id = hit.ctypes.data
    rule, vis = abi.shadow_rule(rule), abi.visibility(vis)
    rc = ds.L.srt_shade_paths_masked(ds.h, n, r.ctypes.data_as(f32p), None, C.byref(p), C.byref(pd), C.byref(rule) if rule is not None else None,
                                     C.byref(vis) if vis is not None else None, lin.ctypes.data_as(f32p), rgb8.ctypes.data_as(u8p), C.byref(po), C.byref(st))
    assert rc == abi.SRT_OK
    return lin, rgb8, hit


@gpu
def test_identities_of_the_shaded_paths(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    p = sq.shade_params(lights)
    fp = rpr.camera_params(name, lights)
    ds = srt.DeviceScene(flat)
    for table in ("never set", np.full(flat.n_objects, ALL, np.uint32)):
        if not isinstance(table, str):
            ds.set_object_masks(table)
        for rule in (None, sh.SELF):
            plain = ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=rule, count=True)
            sp.assert_same(plain, sh.case_reference(oracle, name, rule), f"the _shadow call, rule {rule}")
            got = ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=rule, visibility=(ALL, ALL, ALL), count=True)
            sp.assert_same(got, plain, f"all ones, rule {rule}")
            assert got["stats"] == plain["stats"], (got["stats"], plain["stats"])
            for vis in (None, (ALL, ALL, ALL)):
                lin, rgb8, hit = raw_masked_paths(ds, rays, p, refl, rule, vis)
                assert np.array_equal(bits(lin), bits(plain["rgb_linear"])) and np.array_equal(rgb8, plain["rgb8"]) and np.array_equal(hit, plain["seg_hit_id"]), (rule, vis)
            frame = ds.render_paths(fp, DEPTH, refl, TMIN, shadow=rule)
            sp.assert_same(rpr.flat_rows(ds.render_paths(fp, DEPTH, refl, TMIN, shadow=rule, visibility=(ALL, ALL, ALL))), rpr.flat_rows(frame), f"frame, all ones, rule {rule}")
    ds.close()


# ---- 5. paths and frames under a mask per ray kind --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_paths_under_visibility_triples(srt, oracle, name):
    flat, rays, lights, refl = sh.lamp_case(name)
    p = sq.shade_params(lights)
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(vr.case_table(flat))
    for which in (0, 1):
        vis = vr.case_vis(name, which)
        for label, rule in RULES.items():
            want = vr.case_reference(oracle, name, which, rule)
            o = ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=rule, visibility=vis)
            sp.assert_same(o, want, f"{name}, triple {which}, rule {label}")
            hits = int((want["seg_hit_id"] >= 0).sum())
            assert o["stats"]["primary_rays"] == rays.shape[0] and o["stats"]["hit_rays"] == hits and o["stats"]["shadow_rays"] == hits * vr.N_LIGHTS
        # depth 1: the masked shade of the rays, segment 0 of the yardstick; and the counting build gives the same rows
        want = vr.case_reference(oracle, name, which, sh.ENDED)
        one = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=sh.ENDED, visibility=vis)
        sp.assert_same(one, {k: want[k][:1] for k in sp.SEG_KEYS}, "depth 1", sp.SEG_KEYS)
        assert np.array_equal(bits(one["rgb_linear"]), bits(want["seg_rgb_linear"][0]))
        sp.assert_same(ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=sh.ENDED, visibility=vis, count=True), want, "counting")
    ds.close()


@gpu
@pytest.mark.parametrize("share", [None, dict(block_rows=8, block_cols=8, block_first=1, block_stride=2)])
def test_a_frame_is_its_rays(srt, share):
    """spp = 1: srt_render_paths_masked equals srt_shade_paths_masked on the frame's rays, at the owned pixels (padding keeps the fill); a
    tile-dealt share writes the whole frame's values."""
    name = "cubes4_a40"
    flat, _, lights, refl = sh.lamp_case(name)
    p = rpr.camera_params(name, lights, **(share or {}))
    rays, live = rpr.frame_rays_owned(p)
    vis = vr.case_vis(name, 0)
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(vr.case_table(flat))
    for rule in (None, sh.ENDED):
        o = rpr.flat_rows(ds.render_paths(p, DEPTH, refl, TMIN, fill=7, shadow=rule, visibility=vis))
        sel = np.flatnonzero(live.reshape(-1))
        assert sel.size and (share is None or sel.size < live.size)
        want = ds.shade_paths(rays.reshape(-1, 6)[sel], sq.shade_params(lights), DEPTH, refl, TMIN, shadow=rule, visibility=vis)
        assert (want["seg_hit_id"][1] >= 0).any()
        sp.assert_same(cut(o, sel), want, f"share {share}, rule {rule}")
        for k, v in cut(o, np.flatnonzero(~live.reshape(-1))).items():
            assert (v == 7).all(), ("padding written", k)
        plain = rpr.flat_rows(ds.render_paths(p, DEPTH, refl, TMIN, fill=7, shadow=rule))
        assert (plain["rgb8"][sel] != o["rgb8"][sel]).any(), "the masks change no pixel of the frame"
    ds.close()


@gpu
def test_a_frame_at_spp_4(srt, oracle):
    name = "cubes4_a40"
    flat, _, lights, refl = sh.lamp_case(name)
    vis, table = vr.case_vis(name, 0), vr.case_table(flat)
    p = rpr.camera_params(name, lights, 24, 14, spp=4)
    want = vr.render_paths(oracle, flat, p, DEPTH, vis, table, refl, TMIN, rule=sh.ENDED)
    assert (want["seg_hit_id"][1] >= 0).any()
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    o = ds.render_paths(p, DEPTH, refl, TMIN, shadow=sh.ENDED, visibility=vis, count=True)
    sp.assert_same(rpr.flat_rows(o), rpr.flat_rows(want), "spp 4")
    assert o["stats"]["primary_rays"] == 24 * 14 * 4
    ds.close()


# ---- 6. persistence and sharing -----------------------------------------------------------------------------------------------------------
@gpu
def test_persistence_and_sharing(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    c = vr.case_candidates(oracle, name)
    table, m = vr.hidden(flat, 1)
    masks = np.full(rays.shape[0], m, np.uint32)
    hit, t = vr.closest(c, flat, m, table)
    ds = srt.DeviceScene(flat)
    other = ds.share()
    plain = other.trace_rays(rays, ray_mask=masks)
    assert not np.array_equal(plain["hit_id"], hit)
    ds.set_object_masks(table)
    ds.trace_rays(rays[:1])          # (a host call on the stream the table went to: it has arrived before another handle's stream reads it)
    same_trace(other.trace_rays(rays, ray_mask=masks), hit, t, "set through one handle, seen through the other")
    late = ds.share()
    same_trace(late.trace_rays(rays, ray_mask=masks), hit, t, "a handle shared after the call")
    late.close()
    # a pose with identity matrices, and an update with the same scene: the table stays
    ds.set_pose_source()
    ds.pose(np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1)))
    same_trace(ds.trace_rays(rays, ray_mask=masks), hit, t, "after srt_scene_pose")
    ds.update(flat)
    same_trace(ds.trace_rays(rays, ray_mask=masks), hit, t, "after srt_scene_update")
    # the unmasked calls never read the table
    full = ds.trace_rays(rays)
    same_trace(full, *rr.closest(c), "srt_trace_rays with a table set")
    # NULL restores the identity
    other.set_object_masks(None)
    other.trace_rays(rays[:1])
    same_trace(ds.trace_rays(rays, ray_mask=masks), plain["hit_id"], plain["t"], "set_object_masks(None)")
    ds.close(); other.close()


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_errors(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    c = vr.case_candidates(oracle, name)
    table, m = vr.hidden(flat, 1)
    masks = np.full(rays.shape[0], m, np.uint32)
    ds = srt.DeviceScene(flat)
    L = ds.L
    ds.set_object_masks(table)
    u32p, f32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    bad = np.zeros(flat.n_objects + 1, np.uint32)
    for n_obj in (flat.n_objects - 1, flat.n_objects + 1, 0):
        assert L.srt_scene_set_object_masks(ds.h, n_obj, bad.ctypes.data_as(u32p), None) == abi.SRT_ERR_LAYOUT
        assert L.srt_scene_set_object_masks(ds.h, n_obj, None, None) == abi.SRT_ERR_LAYOUT
    same_trace(ds.trace_rays(rays, ray_mask=masks), *vr.closest(c, flat, m, table), "the previous table stays in force")
    n = 8
    r = np.ascontiguousarray(rays[:n]); hit = np.full(n, -9, np.int32); occ = np.full(n, 9, np.uint8)
    rp, mp = r.ctypes.data_as(f32p), masks.ctypes.data_as(u32p)
    for flags in (abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_NO_TIMING, 1 << 8, 1 << 31):
        assert L.srt_trace_rays_masked(ds.h, n, rp, None, mp, flags, hit.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_trace_rays_masked_device(ds.h, n, r.ctypes.data, None, None, flags, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_masked(ds.h, n, None, None, mp, 0, hit.ctypes.data_as(i32p), None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_occluded_masked(ds.h, n, None, None, mp, None, occ.ctypes.data_as(C.POINTER(C.c_uint8))) == abi.SRT_ERR_ARG
    assert (hit == -9).all() and (occ == 9).all(), "an error touched an output"
    # n == 0 and a NULL `occluded`: nothing to do
    assert L.srt_trace_rays_masked(ds.h, 0, None, None, None, 0, None, None, None, None) == abi.SRT_OK
    assert L.srt_occluded_masked(ds.h, n, rp, None, mp, None, None) == abi.SRT_OK
    # the errors of the _shadow calls keep their codes with a srt_visibility present
    p, fp = sq.shade_params(lights), rpr.camera_params(name, lights, 4, 2)
    vis, rule = abi.visibility((1, 2, 4)), abi.shadow_rule(sh.ENDED)
    lin = np.full((n, 3), -9.0, np.float32)
    ref = lambda v: C.byref(v) if v is not None else None
    paths = lambda pd, rule_: L.srt_shade_paths_masked(ds.h, n, rp, None, C.byref(p), ref(pd), ref(rule_), C.byref(vis), lin.ctypes.data_as(f32p), None, None, None)
    frame = lambda pd, rule_: L.srt_render_paths_masked(ds.h, C.byref(fp), ref(pd), ref(rule_), C.byref(vis), lin.ctypes.data_as(f32p), None, None, None)
    for call in (paths, frame):
        assert call(abi.PathDesc(0, TMIN, None), rule) == abi.SRT_ERR_ARG and call(None, rule) == abi.SRT_ERR_ARG
        assert call(abi.PathDesc(abi.SRT_PATH_DEPTH_MAX + 1, TMIN, None), None) == abi.SRT_ERR_LIMIT
        assert call(abi.PathDesc(3, TMIN, None), abi.ShadowRule(1e-3, 1.0, 2)) == abi.SRT_ERR_ARG
    assert (lin == -9.0).all(), "an error touched an output"
    assert L.srt_shade_paths_masked(ds.h, n, rp, None, C.byref(p), C.byref(abi.PathDesc(3, TMIN, None)), None, C.byref(vis), None, None, None, None) == abi.SRT_OK
    same_trace(ds.trace_rays(rays, ray_mask=masks), *vr.closest(c, flat, m, table), "after the errors")
    ds.close()


# ---- 8. the device forms, and hipGraph capture, in a process of its own --------------------------------------------------------------------
@gpu
def test_device_forms_and_graph_capture():
    r = subprocess.run([sys.executable, os.path.join(HERE, "visibility_device_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "visibility device case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
