"""GPU (-m gpu): shaded paths under a shadow rule (include/srt.h, "Shadow rays with an end") -- srt_shade_paths_shadow and
srt_render_paths_shadow pinned bit for bit by tests/shadow_rule_ref.py, on shade_path_ref.FRAMES' frames lit by a lamp INSIDE the scene
(shadow_rule_ref.LAMPS; tests/test_shadow_rule_ref.py checks each case's input conditions on the yardstick alone).  Floats compare by
bits; where the yardstick is NaN the device must be NaN."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh
import surface_ref as sf
import tree_shapes as ts
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = np.float32(np.inf)
TMIN, DEPTH = sh.BOUNCE_T_MIN, sh.DEPTH
RULES = {"SELF": sh.SELF, "ENDED": sh.ENDED}
PLAIN_LAMP = (30.0, -40.0, 150.0)      # the lamp of the frame without a matrix: in front of the tree-shape objects
COUNTERS = ("node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow")
bits = sf.bits


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def cut(ref, sel):
    return {k: (v[sel] if k in ("rgb_linear", "rgb8") else v[:, sel]) for k, v in ref.items() if k in sp.ALL_KEYS}


# ---- 1. the host form on the three lamp cases ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_frames_of_rays_under_a_rule(srt, oracle, name):
    flat, rays, lights, refl = sh.lamp_case(name)
    ds = srt.DeviceScene(flat)
    for label, rule in RULES.items():
        want = sh.case_reference(oracle, name, rule)
        o = ds.shade_paths(rays, sq.shade_params(lights), DEPTH, refl, TMIN, shadow=rule)
        sp.assert_same(o, want, f"{name}, {label}")
        hits = int((want["seg_hit_id"] >= 0).sum())
        assert o["stats"]["primary_rays"] == rays.shape[0] and o["stats"]["hit_rays"] == hits and o["stats"]["shadow_rays"] == hits * sh.N_LIGHTS
    ds.close()


# ---- 2. the chain: the definition names srt_occluded_range -----------------------------------------------------------------------------
@gpu
def test_the_bits_are_srt_occluded_range_on_the_shadow_rays(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    segs = sh.case_trace(oracle, name)
    ds = srt.DeviceScene(flat)
    cur, tr = rays, None
    for b, seg in enumerate(segs):
        f = ds.surface_rays(cur, want=("hit_id", "obj", "point", "bounce"), t_range=tr)
        assert np.array_equal(f["hit_id"], seg.hit), b
        sel = seg.sel
        for label, rule in RULES.items():
            want = sh.shadow_bits(flat, seg, rule)
            for l in range(lights.shape[0]):
                so = f["point"][sel]
                srays = np.ascontiguousarray(np.concatenate([so, (lights[l][None, :] - so).astype(np.float32)], axis=1), np.float32)
                assert np.array_equal(bits(srays), bits(seg.srays[l * sel.size:(l + 1) * sel.size])), (b, l)
                skip = np.full(sel.size, -1, np.int32) if rule[2] else f["obj"][sel].astype(np.int32)
                got = ds.occluded(srays, skip_obj=skip, t_range=np.tile(np.float32(rule[:2]), (sel.size, 1)))
                assert np.array_equal(got.astype(bool), want[:, l]), (b, l, label)
        on = seg.hit >= 0
        cur = np.ascontiguousarray(f["bounce"])
        tr = np.stack([np.where(on, np.float32(TMIN), np.float32(1.0)), np.where(on, INF, np.float32(0.0))], axis=1).astype(np.float32)
    ds.close()


# ---- 3. identities ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_identities(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    p = sq.shade_params(lights)
    ds = srt.DeviceScene(flat)
    plain = ds.shade_paths(rays, p, DEPTH, refl, TMIN)
    sp.assert_same(plain, sh.case_reference(oracle, name, None), "no rule")
    # a NULL rule through the new entry point, and each identity rule: srt_shade_paths' bytes
    st = abi.Stats()
    r = np.ascontiguousarray(rays, np.float32)
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lin, rgb8 = np.empty((r.shape[0], 3), np.float32), np.empty((r.shape[0], 3), np.uint8)
    d_refl = np.ascontiguousarray(refl, np.float32)
    pd = abi.PathDesc(DEPTH, TMIN, d_refl.ctypes.data)
    assert ds.L.srt_shade_paths_shadow(ds.h, r.shape[0], r.ctypes.data_as(f32p), None, C.byref(p), C.byref(pd), None, lin.ctypes.data_as(f32p), rgb8.ctypes.data_as(u8p),
                                       None, C.byref(st)) == abi.SRT_OK
    assert np.array_equal(bits(lin), bits(plain["rgb_linear"])) and np.array_equal(rgb8, plain["rgb8"])
    for label, rule in sh.IDENTITIES.items():
        sp.assert_same(ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=rule), plain, label)
    # depth 1 under a rule: the yardstick's segment 0
    want = sh.case_reference(oracle, name, sh.SELF)
    one = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=sh.SELF)
    sp.assert_same(one, {k: want[k][:1] for k in sp.SEG_KEYS}, "depth 1", sp.SEG_KEYS)
    assert np.array_equal(bits(one["rgb_linear"]), bits(want["seg_rgb_linear"][0]))
    # depth 2: the first two rows of depth 3
    two = ds.shade_paths(rays, p, 2, refl, TMIN, shadow=sh.SELF)
    sp.assert_same(two, {k: want[k][:2] for k in sp.SEG_KEYS}, "depth 2 of depth 3", sp.SEG_KEYS)
    # a reversed batch: the reversed rows
    rev = ds.shade_paths(np.ascontiguousarray(rays[::-1]), p, DEPTH, refl, TMIN, shadow=sh.SELF)
    sp.assert_same(rev, cut(want, slice(None, None, -1)), "reversed")
    # t_min > t_max: a scene without shadows
    sp.assert_same(ds.shade_paths(rays, p, DEPTH, refl, TMIN, shadow=sh.NO_SHADOWS), sh.case_reference(oracle, name, sh.NO_SHADOWS), "t_min > t_max")
    ds.close()


# ---- 4. frames ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("share", [None, dict(block_rows=8, block_cols=8, block_first=1, block_stride=2)])
def test_a_frame_is_its_rays(srt, share):
    """spp = 1: srt_render_paths_shadow equals srt_shade_paths_shadow on the frame's rays, at the owned pixels (padding keeps the fill)."""
    name = "cubes4_a40"
    flat, _, lights, refl = sh.lamp_case(name)
    p = rpr.camera_params(name, lights, **(share or {}))
    rays, live = rpr.frame_rays_owned(p)
    ds = srt.DeviceScene(flat)
    o = rpr.flat_rows(ds.render_paths(p, DEPTH, refl, TMIN, fill=7, shadow=sh.SELF))
    sel = np.flatnonzero(live.reshape(-1))
    assert sel.size and (share is None or sel.size < live.size)
    want = ds.shade_paths(rays.reshape(-1, 6)[sel], sq.shade_params(lights), DEPTH, refl, TMIN, shadow=sh.SELF)
    assert (want["seg_hit_id"][1] >= 0).any()
    sp.assert_same(cut(o, sel), want, f"share {share}")
    pad = np.flatnonzero(~live.reshape(-1))
    for k, v in cut(o, pad).items():
        assert (v == 7).all(), ("padding written", k)
    plain = rpr.flat_rows(ds.render_paths(p, DEPTH, refl, TMIN, fill=7))
    assert (plain["rgb8"][sel] != o["rgb8"][sel]).any(), "the rule changes no pixel of the frame"
    ds.close()


@gpu
def test_a_frame_at_spp_4_and_a_frame_without_a_matrix(srt, oracle):
    name = "cubes4_a40"
    flat, _, lights, refl = sh.lamp_case(name)
    ds = srt.DeviceScene(flat)
    p = rpr.camera_params(name, lights, 24, 14, spp=4)
    want = sh.render_paths(oracle, flat, p, DEPTH, refl, TMIN, rule=sh.SELF)
    assert (want["seg_hit_id"][1] >= 0).any()
    sp.assert_same(rpr.flat_rows(ds.render_paths(p, DEPTH, refl, TMIN, shadow=sh.SELF)), rpr.flat_rows(want), "spp 4")
    ds.close()
    # no matrix, depth 1, the rule on: the tree-shape frame (the camera at the origin looks down +z at it), the lamp in front of the objects
    flat = ts.family("sliced")
    p = abi.make_params(ts.W, ts.H, abi.light_staircase(np.float32(PLAIN_LAMP), 2), focal=ts.FOCAL)
    want = sh.render_paths(oracle, flat, p, 1, None, TMIN, rule=sh.SELF)
    assert (want["seg_hit_id"][0] >= 0).sum() > 100
    ds = srt.DeviceScene(flat)
    sp.assert_same(rpr.flat_rows(ds.render_paths(p, 1, None, TMIN, shadow=sh.SELF)), rpr.flat_rows(want), "no matrix, depth 1")
    ds.close()


# ---- 5. the device forms, and hipGraph capture, in a process of its own ----------------------------------------------------------------
@gpu
def test_device_forms_and_graph_capture():
    r = subprocess.run([sys.executable, os.path.join(HERE, "shadow_rule_device_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "shadow rule device case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 6. the counting build ---------------------------------------------------------------------------------------------------------------
@gpu
def test_counting_build(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    p = sq.shade_params(lights)
    ds = srt.DeviceScene(flat)
    base = ds.shade_paths(rays, p, DEPTH, refl, TMIN, count=True)["stats"]
    assert all(base[k] > 0 for k in COUNTERS)
    same = ds.shade_paths(rays, p, DEPTH, refl, TMIN, count=True, shadow=sh.IDENTITIES["(0, inf)"])["stats"]
    assert all(same[k] == base[k] for k in COUNTERS), (same, base)
    for label, rule in RULES.items():
        o = ds.shade_paths(rays, p, DEPTH, refl, TMIN, count=True, shadow=rule)
        sp.assert_same(o, sh.case_reference(oracle, name, rule), f"counting, {label}")
        st = o["stats"]
        assert st["node_tests_primary"] == base["node_tests_primary"] and st["tri_tests_primary"] == base["tri_tests_primary"], (label, st, base)
        assert st["hit_rays"] == base["hit_rays"] and st["shadow_rays"] == base["shadow_rays"]
        if not rule[2]:      # bounding can only postpone the first blocking hit
            assert st["node_tests_shadow"] >= base["node_tests_shadow"] and st["tri_tests_shadow"] >= base["tri_tests_shadow"], (st, base)
    # a frame: the same through the other kernel
    fp = rpr.camera_params(name, lights)
    fbase = ds.render_paths(fp, DEPTH, refl, TMIN, count=True)
    frule = ds.render_paths(fp, DEPTH, refl, TMIN, count=True, shadow=sh.ENDED)
    sp.assert_same(rpr.flat_rows(frule), rpr.flat_rows(ds.render_paths(fp, DEPTH, refl, TMIN, shadow=sh.ENDED)), "frame, counting or not")
    assert all(frule["stats"][k] == fbase["stats"][k] for k in COUNTERS[:2]) and all(frule["stats"][k] >= fbase["stats"][k] for k in COUNTERS[2:])
    ds.close()


# ---- 7. shapes where SELF takes a path the old code never took -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(flat, rays, lights): one object whose root is a leaf -- skipping the own tree walks NOTHING there, SELF walks everything -- or the
    comb of height 256; 48 rays aimed at the leaves, the lamp behind the rays' origins."""
    flat = ts.flat_scene(ts.roots_objects(1)) if name == "one_root_leaf" else ts.family(name)
    return flat, ts.aimed_rays(flat, 48), abi.light_staircase(np.asarray(ts.LIGHT, np.float32), 2)


@gpu
@pytest.mark.parametrize("name", ["one_root_leaf", "comb256"])
def test_tree_shapes_under_self(srt, oracle, name):
    flat, rays, lights = shape_case(name)
    refl = np.full(int(flat.tri_obj.max()) + 1, 0.5, np.float32)
    rule = (1e-3, 1.0, True)
    segs = sh.trace(oracle, flat, rays, lights, 2, TMIN)
    want = sh.shade_paths_of(oracle, flat, segs, 2, rule, refl)
    assert (want["seg_hit_id"][0] >= 0).sum() * 4 >= rays.shape[0]
    if name == "one_root_leaf":
        assert int(flat.tri_obj.max()) == 0 and flat.n_nodes == 1
        assert not any(sh.shadow_bits(flat, s, None).any() for s in segs) and any(sh.shadow_bits(flat, s, rule).any() for s in segs)
    ds = srt.DeviceScene(flat)
    sp.assert_same(ds.shade_paths(rays, sq.shade_params(lights), 2, refl, TMIN, shadow=rule, count=True), want, name)
    sp.assert_same(ds.shade_paths(rays, sq.shade_params(lights), 2, refl, TMIN, shadow=rule), want, name)
    ds.close()


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_errors(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    ds = srt.DeviceScene(flat)
    L = ds.L
    n = 8
    r = np.ascontiguousarray(rays[:n]); lin = np.full((n, 3), -9.0, np.float32); hit = np.full((3, n), -9, np.int32)
    f32p = C.POINTER(C.c_float)
    rp, lp = r.ctypes.data_as(f32p), lin.ctypes.data_as(f32p)
    po = abi.PathOut(); po.hit_id = hit.ctypes.data
    good, fp = sq.shade_params(lights), rpr.camera_params(name, lights, 4, 2)
    flin = np.full((2, 4, 3), -9.0, np.float32)
    ok_rule = abi.shadow_rule(sh.SELF)
    ref = lambda v: C.byref(v) if v is not None else None
    paths = lambda p, pd, rule, rays_=rp: L.srt_shade_paths_shadow(ds.h, n, rays_, None, ref(p), ref(pd), ref(rule), lp, None, C.byref(po), None)
    frame = lambda p, pd, rule: L.srt_render_paths_shadow(ds.h, ref(p), ref(pd), ref(rule), flin.ctypes.data_as(f32p), None, None, None)
    # bad rule flags
    for flags in (2, 3, 1 << 31):
        bad = abi.ShadowRule(1e-3, 1.0, flags)
        assert paths(good, abi.PathDesc(3, TMIN, None), bad) == abi.SRT_ERR_ARG and frame(fp, abi.PathDesc(3, TMIN, None), bad) == abi.SRT_ERR_ARG, flags
        assert L.srt_shade_paths_shadow_device(ds.h, n, r.ctypes.data, 0, C.byref(good), C.byref(abi.PathDesc(3, TMIN, None)), C.byref(bad), 0, 0, 0, C.byref(po)) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_shadow_device(ds.h, C.byref(fp), C.byref(abi.PathDesc(3, TMIN, None)), C.byref(bad), 0, 0, 0, C.byref(po)) == abi.SRT_ERR_ARG
    # the errors of srt_shade_paths / srt_render_paths keep their codes with a rule present
    assert paths(good, abi.PathDesc(0, TMIN, None), ok_rule) == abi.SRT_ERR_ARG
    assert paths(good, abi.PathDesc(abi.SRT_PATH_DEPTH_MAX + 1, TMIN, None), ok_rule) == abi.SRT_ERR_LIMIT
    assert paths(good, None, ok_rule) == abi.SRT_ERR_ARG
    assert paths(good, abi.PathDesc(3, TMIN, None), ok_rule, None) == abi.SRT_ERR_ARG
    assert paths(None, abi.PathDesc(3, TMIN, None), ok_rule) == abi.SRT_ERR_ARG
    for flags in (1 << 8, abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_SMOOTH_NORMALS):                               # (no normals in this scene)
        assert paths(sq.shade_params(lights, flags=flags), abi.PathDesc(3, TMIN, None), ok_rule) == abi.SRT_ERR_ARG, flags
    assert frame(fp, abi.PathDesc(0, TMIN, None), ok_rule) == abi.SRT_ERR_ARG
    assert frame(fp, abi.PathDesc(abi.SRT_PATH_DEPTH_MAX + 1, TMIN, None), ok_rule) == abi.SRT_ERR_LIMIT
    assert frame(fp, None, ok_rule) == abi.SRT_ERR_ARG and frame(None, abi.PathDesc(3, TMIN, None), ok_rule) == abi.SRT_ERR_ARG
    assert frame(rpr.camera_params(name, lights, 4, 2, flags=1 << 8), abi.PathDesc(3, TMIN, None), ok_rule) == abi.SRT_ERR_ARG
    assert frame(rpr.camera_params(name, lights, 4, 2, spp=3), abi.PathDesc(3, TMIN, None), ok_rule) != abi.SRT_OK
    assert (lin == -9.0).all() and (hit == -9).all() and (flin == -9.0).all(), "an error touched an output"
    # all outputs NULL
    assert L.srt_shade_paths_shadow(ds.h, n, rp, None, C.byref(good), C.byref(abi.PathDesc(3, TMIN, None)), C.byref(ok_rule), None, None, None, None) == abi.SRT_OK
    assert L.srt_render_paths_shadow(ds.h, C.byref(fp), C.byref(abi.PathDesc(3, TMIN, None)), C.byref(ok_rule), None, None, None, None) == abi.SRT_OK
    # a good call still matches: nothing was touched
    sp.assert_same(ds.shade_paths(rays, good, DEPTH, refl, TMIN, shadow=sh.SELF), sh.case_reference(oracle, name, sh.SELF), "after the errors")
    ds.close()
