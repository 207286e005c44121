"""GPU (-m gpu): refracting paths (include/srt.h, "Refracting paths") -- srt_shade_paths_refract and srt_render_paths_refract pinned bit
for bit by tests/refract_ref.py where the batch is small enough for the yardstick (tests/test_refract_ref.py pins that yardstick to the
mirror yardstick and to Snell's law, and checks every case's input conditions), and by the chain of existing host calls with
refract_ref.refract_dir between them where it is not.  Floats compare by bits; where the yardstick is NaN the device must be NaN.  The
last test needs no GPU: the header declares the four entry points and the struct, and the library exports them."""
import ctypes as C
import dataclasses
import functools
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import golden_util as gu
import ray_query_ref as rq
import ray_range_ref as rr
import refract_ref as rf
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh
import surface_ref as sf
import tree_shapes as ts
import visibility_ref as vr
from adversarial import with_vertex_normals
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INF = np.float32(np.inf)
ALL = vr.ALL
TMIN = rf.BOUNCE_T_MIN
NEW = ("srt_shade_paths_refract_device", "srt_shade_paths_refract", "srt_render_paths_refract_device", "srt_render_paths_refract")
COUNTERS = ("node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow")
bits = sf.bits


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def cut(ref, sel):
    return {k: (v[sel] if k in ("rgb_linear", "rgb8") else v[:, sel]) for k, v in ref.items() if k in sp.ALL_KEYS}


def check_stats(o, want, n, n_lights):
    hits = int((want["seg_hit_id"] >= 0).sum())
    assert o["stats"]["primary_rays"] == n and o["stats"]["hit_rays"] == hits and o["stats"]["shadow_rays"] == hits * n_lights, o["stats"]


# ---- 1. frames of rays ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(rf.DEPTHS))
def test_frames_of_rays(srt, oracle, name):
    flat, rays, lights, refl = sp.frame_case(name)
    rf.condition(*rf.case_walks(oracle, name))
    want = rf.case_reference(oracle, name)
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.shade_paths(rays, sq.shade_params(lights), rf.DEPTHS[name], refl, TMIN, count=count, ior=rf.case_ior(flat))
        sp.assert_same(o, want, f"{name}, counting {count}")
        check_stats(o, want, rays.shape[0], rf.N_LIGHTS)
    ds.close()


# ---- 2. wave and workgroup edges, order ----------------------------------------------------------------------------------------------
def does_all_three(kinds, first):
    seen = {k: any((kk[:first] == k).any() for kk in kinds) for k in (rf.ENTER, rf.LEAVE, rf.TIR)}
    return all(seen.values())


@functools.lru_cache(maxsize=None)
def edge_batch():
    """257 rays over cubes4_a40 whose first 63 hold an entering, a leaving and a totally reflected ray: rq.unrelated_rays if they do, else a
    fixed shuffled subset of the frame's rays.  With 3 lights and the yardstick's rows at depth 3 (computed once, never changed)."""
    from oracle import pyoracle
    flat, frame, lights, refl = sp.frame_case("cubes4_a40")
    ior = rf.case_ior(flat)
    none = np.zeros((0, 3), np.float32)
    rays = rq.unrelated_rays(flat, 257)
    if not does_all_three(rf.trace(pyoracle, flat, rays[:63], none, 3, ior, bounce_t_min=TMIN)[1], 63):
        rays = np.ascontiguousarray(frame[np.random.default_rng(5).permutation(frame.shape[0])[:257]])
    memo = vr.CandidateMemo(pyoracle, flat)
    assert does_all_three(rf.trace(pyoracle, flat, rays[:63], none, 3, ior, bounce_t_min=TMIN, cands=memo)[1], 63), "the first 63 rays do not enter, leave and reflect"
    ref = rf.shade_paths(pyoracle, flat, rays, lights, 3, ior, refl, TMIN, cands=memo)
    for v in ref.values():
        v.setflags(write=False)
    return flat, rays, lights, refl, ior, ref


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_edges(srt, n):
    flat, rays, lights, refl, ior, ref = edge_batch()
    ds = srt.DeviceScene(flat)
    sp.assert_same(ds.shade_paths(rays[:n], sq.shade_params(lights), 3, refl, TMIN, ior=ior), cut(ref, slice(0, n)), f"n {n}")
    ds.close()


@gpu
def test_a_permuted_batch_gives_permuted_rows(srt):
    flat, rays, lights, refl, ior, ref = edge_batch()
    perm = np.random.default_rng(3).permutation(rays.shape[0])
    ds = srt.DeviceScene(flat)
    # 16 lights: the deal of rays to waves is the spread one
    l16 = sq.lights_for("cubes4_a40", gu.GoldenScene("cubes4_a40").light, 16)
    for lt, want in ((lights, ref), (l16, None)):
        a = ds.shade_paths(rays, sq.shade_params(lt), 3, refl, TMIN, ior=ior)
        if want is not None:
            sp.assert_same(a, want, "in order")
        sp.assert_same(ds.shade_paths(np.ascontiguousarray(rays[perm]), sq.shade_params(lt), 3, refl, TMIN, ior=ior), cut(a, perm), f"permuted, {len(lt)} lights")
    o = ds.shade_paths(np.zeros((0, 6), np.float32), sq.shade_params(lights), 3, refl, TMIN, ior=ior)                  # n == 0
    assert o["rgb8"].shape == (0, 3) and o["seg_hit_id"].shape == (3, 0)
    ds.close()


# ---- 3. identities -------------------------------------------------------------------------------------------------------------------
def raw_refract_paths(ds, rays, p, depth, refl, rule, vis, refr):
    """srt_shade_paths_refract through the C ABI, so that refr and refr->ior may be NULL: (rgb_linear, rgb8, seg_hit_id, stats)."""
    r = np.ascontiguousarray(rays, np.float32)
    n = r.shape[0]
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lin, rgb8, hit = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8), np.empty((depth, n), np.int32)
    k = np.ascontiguousarray(refl, np.float32)
    pd, po, st = abi.PathDesc(depth, TMIN, k.ctypes.data), abi.PathOut(), abi.Stats()
    po.hit_id = hit.ctypes.data
    rule, vis = abi.shadow_rule(rule), abi.visibility(vis)
    ref = lambda v: C.byref(v) if v is not None else None
    rc = ds.L.srt_shade_paths_refract(ds.h, n, r.ctypes.data_as(f32p), None, C.byref(p), C.byref(pd), ref(rule), ref(vis), ref(refr), lin.ctypes.data_as(f32p),
                                      rgb8.ctypes.data_as(u8p), C.byref(po), C.byref(st))
    assert rc == abi.SRT_OK
    return lin, rgb8, hit, st.as_dict()


@gpu
def test_identities(srt):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    depth = rf.DEPTHS[name]
    nO = flat.n_objects
    fp = rpr.camera_params(name, lights)
    ds = srt.DeviceScene(flat)
    glass = ds.shade_paths(rays, sq.shade_params(lights), depth, refl, TMIN, ior=rf.case_ior(flat))
    for rule, vis in ((None, None), (sh.SELF, None), (sh.ENDED, (ALL, ALL, ALL))):
        p = sq.shade_params(lights, flags=abi.SRT_FLAG_COUNT_WORK)
        masked = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True)
        assert (masked["seg_hit_id"][1] != glass["seg_hit_id"][1]).any(), "the glass changes nothing"
        # no table: refr NULL, or refr->ior NULL
        for refr in (None, abi.Refraction(None, 0)):
            lin, rgb8, hit, st = raw_refract_paths(ds, rays, p, depth, refl, rule, vis, refr)
            assert np.array_equal(bits(lin), bits(masked["rgb_linear"])) and np.array_equal(rgb8, masked["rgb8"]) and np.array_equal(hit, masked["seg_hit_id"]), (rule, vis)
            assert st == masked["stats"], (st, masked["stats"])
        # a table without a positive entry
        for label, table in (("0", np.zeros(nO, np.float32)), ("-1", np.full(nO, -1.0, np.float32)), ("NaN", np.full(nO, np.nan, np.float32)),
                             ("-0, -inf", np.where(np.arange(nO) % 2 == 0, np.float32(-0.0), -INF).astype(np.float32))):
            got = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=table)
            sp.assert_same(got, masked, f"ior all {label}, rule {rule}, vis {vis}")
            assert got["stats"] == masked["stats"] and all(got["stats"][k] > 0 for k in COUNTERS), (label, got["stats"], masked["stats"])
            frame = ds.render_paths(fp, depth, refl, TMIN, shadow=rule, visibility=vis, count=True)
            o = ds.render_paths(fp, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=table)
            sp.assert_same(rpr.flat_rows(o), rpr.flat_rows(frame), f"frame, ior all {label}")
            assert o["stats"] == frame["stats"]
        # depth 1 is unchanged by any table
        one = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=rule, visibility=vis, count=True)
        got = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=np.full(nO, 1.5, np.float32))
        sp.assert_same(got, one, "depth 1")
        assert got["stats"] == one["stats"]
    ds.close()


# ---- 4. the chain, on a batch too big for the yardstick ------------------------------------------------------------------------------
def chain(ds, rays, params, depth, ior, reflectance, smooth, count):
    """The chain of existing host calls the one launch replaces: per segment shade_rays(t_range=...) and surface_rays' obj, normal and
    bounce on the LIVE rays only, the next direction refract_ref.refract_dir for glass hits and the bounce otherwise; the mix by
    shade_path_ref.mix.  Returns the seg_* rows, rgb_linear, and the sums of the calls' statistics."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    out = {"seg_hit_id": np.full((depth, n), -1, np.int32), "seg_t": np.full((depth, n), INF, np.float32), "seg_obj": np.full((depth, n), -1, np.int32),
           "seg_rgb_linear": np.zeros((depth, n, 3), np.float32), "seg_rays": np.zeros((depth, n, 6), np.float32)}
    stats = dict.fromkeys(("hit_rays", "shadow_rays") + COUNTERS, 0)
    kinds = []
    live, cur, tr = np.arange(n), rays, None
    for b in range(depth):
        if live.size == 0:
            break
        s = ds.shade_rays(cur, params, want=("hit_id", "t", "rgb_linear"), count=count, t_range=tr)
        f = ds.surface_rays(cur, want=("obj", "normal", "bounce"), smooth=smooth, t_range=tr)
        out["seg_hit_id"][b, live], out["seg_t"][b, live], out["seg_rgb_linear"][b, live] = s["hit_id"], s["t"], s["rgb_linear"]
        out["seg_obj"][b, live], out["seg_rays"][b, live] = f["obj"], cur
        for k in stats:
            stats[k] += s["stats"][k]
        nxt, kind = rf.next_rays(cur, f, ior)
        kinds.append(kind)
        on = s["hit_id"] >= 0
        live, cur = live[on], np.ascontiguousarray(nxt[on])
        tr = np.tile(np.float32([TMIN, INF]), (live.size, 1))
    out["rgb_linear"] = sp.mix(out["seg_hit_id"], out["seg_obj"], out["seg_rgb_linear"], reflectance)
    out["stats"] = stats
    return out, kinds


@gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_chain_equality_and_counters(srt, smooth):
    flat, rays, lights, refl = sp.frame_case("ground_bunny")
    flat = with_vertex_normals(flat)
    ior = rf.case_ior(flat)
    depth = 5
    p = sq.shade_params(lights, flags=abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0)
    ds = srt.DeviceScene(flat)
    want, kinds = chain(ds, rays, p, depth, ior, refl, smooth, True)
    assert (want["seg_hit_id"][depth - 1] >= 0).any()
    assert does_all_three(kinds[1:], rays.shape[0]) and (kinds[0] == rf.MIRROR).any() and (kinds[0] == rf.ENTER).any()
    o = ds.shade_paths(rays, p, depth, refl, TMIN, count=True, smooth=smooth, ior=ior)
    sp.assert_same(o, want, f"ground_bunny, depth {depth}, smooth {smooth}", ("rgb_linear",) + sp.SEG_KEYS)
    hits = int((want["seg_hit_id"] >= 0).sum())
    assert o["stats"]["primary_rays"] == rays.shape[0] and o["stats"]["hit_rays"] == hits == want["stats"]["hit_rays"]
    assert o["stats"]["shadow_rays"] == hits * len(lights) == want["stats"]["shadow_rays"]
    for k in COUNTERS:
        assert o["stats"][k] == want["stats"][k] > 0, (k, o["stats"], want["stats"])
    ds.close()


# ---- 5. together with the masks and the rule ------------------------------------------------------------------------------------------
@gpu
def test_glass_that_casts_no_shadow_under_a_rule(srt, oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    depth, ior = rf.DEPTHS[name], rf.case_ior(flat)
    glass = [k for k in range(flat.n_objects) if ior[k] > 0]
    table, no_glass = vr.hidden(flat, *glass)
    vis = (ALL, ALL, no_glass)
    want = rf.shade_paths(oracle, flat, rays, lights, depth, ior, refl, TMIN, rule=sh.SELF, vis=vis, obj_mask=table, colours=rf.case_colours(oracle, name),
                          cands=rf.case_memo(oracle, name))
    casting = rf.case_reference(oracle, name, sh.SELF)
    assert (want["rgb8"] != casting["rgb8"]).any(), "the glass cast no shadow to begin with"
    assert np.array_equal(want["seg_hit_id"], casting["seg_hit_id"])
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    for count in (False, True):
        o = ds.shade_paths(rays, sq.shade_params(lights), depth, refl, TMIN, shadow=sh.SELF, visibility=vis, count=count, ior=ior)
        sp.assert_same(o, want, f"glass without a shadow, counting {count}")
        check_stats(o, want, rays.shape[0], rf.N_LIGHTS)
    sp.assert_same(ds.shade_paths(rays, sq.shade_params(lights), depth, refl, TMIN, shadow=sh.SELF, visibility=(ALL, ALL, ALL), ior=ior), casting, "glass with its shadow")
    ds.close()


# ---- 5b. everything a host call can bring, through the staging block at once -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def staged_batch():
    """65 rays of cubes4_a40's frame (a fixed shuffle whose first ray goes through the glass inside its interval), one mixed interval per ray, the table that gives every object a bit, and a triple
    that hides the glass from the shadow rays.  With the yardstick's rows under sh.SELF (computed once, never changed), the per-ray masks
    of the closest-hit call that follows and the rays' candidate sets."""
    from oracle import pyoracle
    name = "cubes4_a40"
    flat, frame, lights, refl = sp.frame_case(name)
    ior = rf.case_ior(flat)
    rays = np.ascontiguousarray(frame[np.random.default_rng(3).permutation(frame.shape[0])[:65]])
    memo = rf.case_memo(pyoracle, name)
    c = memo(rays)
    tr, _, _ = rr.mixed_intervals(c, seed=5)
    table, no_glass = vr.hidden(flat, *[k for k in range(flat.n_objects) if ior[k] > 0])
    vis = (ALL, ALL, no_glass)
    ref = rf.shade_paths(pyoracle, flat, rays, lights, rf.DEPTHS[name], ior, refl, TMIN, t_range=tr, rule=sh.SELF, vis=vis, obj_mask=table,
                         colours=rf.case_colours(pyoracle, name), cands=memo)
    masks = np.array([ALL, vr.hidden(flat, 1)[1], 0, vr.hidden(flat, 0, 2)[1]], np.uint32)[np.arange(65) % 4]
    for v in list(ref.values()) + [rays, tr, masks]:
        v.setflags(write=False)
    return flat, rays, lights, refl, ior, tr, table, vis, ref, masks, c


@gpu
@pytest.mark.parametrize("n", [1, 65])
def test_every_staged_array_at_once(srt, n):
    """Host srt_shade_paths_refract with t_range, reflectance, ior, a rule and a triple all present: rays, intervals, both tables travel
    in one staging block (at n = 65 none of n * 24, n * 8, n_objects * 4 bytes is a multiple of its 256-byte granule).  Then
    srt_trace_rays_masked on the same handle: its mask words go through the buffer the path call left alone."""
    flat, rays, lights, refl, ior, tr, table, vis, ref, masks, c = staged_batch()
    assert (n * 24) % 256 and (n * 8) % 256 and (flat.n_objects * 4) % 256
    want = cut(ref, slice(0, n))
    assert want["seg_hit_id"][0, 0] >= 0 and ior[want["seg_obj"][0, 0]] > 0 and want["seg_hit_id"][2, 0] >= 0, "ray 0 does not go through the glass"
    if n == 65:
        assert (want["seg_hit_id"][0] >= 0).any() and (want["seg_hit_id"][0] < 0).any() and (want["seg_hit_id"][2] >= 0).any()
        assert (ior[want["seg_obj"][0][want["seg_obj"][0] >= 0]] > 0).any(), "no ray enters the glass"
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    o = ds.shade_paths(rays[:n], sq.shade_params(lights), rf.DEPTHS["cubes4_a40"], refl, TMIN, t_range=tr[:n], shadow=sh.SELF, visibility=vis, ior=ior)
    sp.assert_same(o, want, f"everything staged, n {n}")
    check_stats(o, want, n, rf.N_LIGHTS)
    sub = rr.Candidates(n, c.ray[c.ray < n], c.tri[c.ray < n], c.t[c.ray < n])
    hit, t = vr.closest(sub, flat, masks[:n], table, tr[:n])
    if n == 65:
        assert (hit >= 0).any() and (hit != vr.closest(sub, flat, None, table, tr[:n])[0]).any(), "the ray masks change nothing"
    got = ds.trace_rays(rays[:n], t_range=tr[:n], ray_mask=masks[:n], want=("hit_id", "t"))
    assert np.array_equal(got["hit_id"], hit) and np.array_equal(bits(got["t"]), bits(t)), f"masked closest hit after the path call, n {n}"
    ds.close()


# ---- 6. tables longer than a wave's worth of objects ----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["roots33", "roots300"])
def test_many_objects(srt, oracle, name):
    flat, rays = ts.family(name), np.ascontiguousarray(ts.ray_batch(name))
    nO = flat.n_objects
    assert nO in (33, 300) and rays.shape[0] % 64
    ior = np.where(np.arange(nO) % 2 == 1, np.float32(1.3) + np.float32(0.01) * (np.arange(nO) % 40).astype(np.float32), np.float32(0.0)).astype(np.float32)
    refl = (np.float32(0.2) + np.float32(0.15) * (np.arange(nO) % 5).astype(np.float32)).astype(np.float32)
    lights = abi.light_staircase(np.float32(ts.LIGHT), 3)
    segs, kinds = rf.trace(oracle, flat, rays, np.zeros((0, 3), np.float32), 3, ior, bounce_t_min=TMIN)
    c = rf.kind_counts(kinds)
    assert sum(k["mirror"] for k in c) > 0 and sum(k["enter"] for k in c) > 0 and sum(k["leave"] + k["tir"] for k in c) > 0, c
    assert len({int(o) for s in segs for o in s.obj[s.obj >= 0]}) > (16 if nO == 33 else 64), "few objects are hit"
    want = rf.shade_paths(oracle, flat, rays, lights, 3, ior, refl, TMIN)
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.shade_paths(rays, sq.shade_params(lights), 3, refl, TMIN, count=count, ior=ior)
        sp.assert_same(o, want, f"{name}, counting {count}")
        check_stats(o, want, rays.shape[0], 3)
    ds.close()


# ---- 7. the frame form ------------------------------------------------------------------------------------------------------------------
def frame_params(name, camera, w, h, lights, **kw):
    return rpr.camera_params(name, lights, w, h, **kw) if camera else abi.make_params(w, h, lights, focal=rpr.PLAIN_FOCAL * w / rpr.W, **kw)


@gpu
@pytest.mark.parametrize("name,camera,size", [("cubes4_a40", True, (48, 27)), ("ground_bunny", False, (40, 24))])
def test_a_frame_is_its_rays(srt, name, camera, size):
    """spp = 1: srt_render_paths_refract equals srt_shade_paths_refract on the frame's rays, with and without ray_matrix; an 8 x 16 tile deal
    over 3 calls writes the whole-frame call's values (padding keeps the fill)."""
    g = gu.GoldenScene(name)
    flat, lights = g.flat, sq.lights_for(name, g.light, 2)
    refl, ior = np.float32(sp.REFLECTANCE[:flat.n_objects]), rf.case_ior(flat)
    depth = 3
    p = frame_params(name, camera, *size, lights)
    assert bool(p.ray_matrix) == camera
    rays, live = rpr.frame_rays_owned(p)
    assert live.all()
    ds = srt.DeviceScene(flat)
    for rule in (None, sh.SELF):
        whole = rpr.flat_rows(ds.render_paths(p, depth, refl, TMIN, shadow=rule, ior=ior))
        want = ds.shade_paths(rays.reshape(-1, 6), sq.shade_params(lights), depth, refl, TMIN, shadow=rule, ior=ior)
        assert (want["seg_hit_id"][2] >= 0).any()
        sp.assert_same(whole, want, f"{name}, rule {rule}")
        mirror = rpr.flat_rows(ds.render_paths(p, depth, refl, TMIN, shadow=rule))
        assert (mirror["rgb8"] != whole["rgb8"]).any(), "the glass changes no pixel of the frame"
        seen = np.zeros(live.size, bool)
        for first in range(3):
            share = frame_params(name, camera, *size, lights, block_rows=8, block_cols=16, block_first=first, block_stride=3)
            own = rpr.owned(share).reshape(-1)
            o = rpr.flat_rows(ds.render_paths(share, depth, refl, TMIN, fill=7, shadow=rule, ior=ior))
            mine = np.flatnonzero(own >= 0)
            assert mine.size
            sp.assert_same(cut(o, mine), cut(whole, own[mine]), f"{name}, share {first} of 3, rule {rule}")
            for k, v in cut(o, np.flatnonzero(own < 0)).items():
                assert (v == 7).all(), ("padding written", k)
            assert not seen[own[mine]].any()
            seen[own[mine]] = True
        assert seen.all()
    ds.close()


@gpu
def test_a_frame_at_spp_4(srt, oracle):
    name = "cubes4_a40"
    flat, _, lights, refl = sp.frame_case(name)
    ior = rf.case_ior(flat)
    w, h = 40, 24
    p = rpr.camera_params(name, lights, w, h, spp=4)
    want = rf.render_paths(oracle, flat, p, 3, ior, refl, TMIN, rule=sh.SELF)
    assert (want["seg_hit_id"][2] >= 0).any()
    ds = srt.DeviceScene(flat)
    o = ds.render_paths(p, 3, refl, TMIN, shadow=sh.SELF, count=True, ior=ior)
    sp.assert_same(rpr.flat_rows(o), rpr.flat_rows(want), "spp 4")
    assert o["stats"]["primary_rays"] == w * h * 4
    ds.close()


# ---- 8. errors ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_errors(srt):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    ior = rf.case_ior(flat)
    ds = srt.DeviceScene(flat)
    L = ds.L
    f32p = C.POINTER(C.c_float)
    n = 8
    r = np.ascontiguousarray(rays[:n])
    rp = r.ctypes.data_as(f32p)
    p, fp = sq.shade_params(lights), rpr.camera_params(name, lights, 4, 2)
    lin = np.full((n, 3), -9.0, np.float32)
    lp = lin.ctypes.data_as(f32p)
    ref = lambda v: C.byref(v) if v is not None else None
    good, bad = abi.Refraction(ior.ctypes.data, 0), abi.Refraction(ior.ctypes.data, 1)
    vis, rule = abi.visibility((1, 2, 4)), abi.shadow_rule(sh.ENDED)
    pd3 = abi.PathDesc(3, TMIN, None)
    paths = lambda pd, rule_, vis_, refr: L.srt_shade_paths_refract(ds.h, n, rp, None, C.byref(p), ref(pd), ref(rule_), ref(vis_), ref(refr), lp, None, None, None)
    frame = lambda pd, rule_, vis_, refr: L.srt_render_paths_refract(ds.h, C.byref(fp), ref(pd), ref(rule_), ref(vis_), ref(refr), lp, None, None, None)
    # the _device forms are refused before any pointer is read
    paths_d = lambda pd, rule_, vis_, refr: L.srt_shade_paths_refract_device(ds.h, n, r.ctypes.data, None, C.byref(p), ref(pd), ref(rule_), ref(vis_), ref(refr), None,
                                                                             lin.ctypes.data, None, None)
    frame_d = lambda pd, rule_, vis_, refr: L.srt_render_paths_refract_device(ds.h, C.byref(fp), ref(pd), ref(rule_), ref(vis_), ref(refr), None, lin.ctypes.data, None, None)
    for call in (paths, frame, paths_d, frame_d):
        for v in (None, vis):
            # flags other than 0
            assert call(pd3, rule, v, bad) == abi.SRT_ERR_ARG and call(pd3, None, v, abi.Refraction(None, 1 << 31)) == abi.SRT_ERR_ARG
            # every error of the _masked call keeps its code with a table present
            assert call(abi.PathDesc(0, TMIN, None), rule, v, good) == abi.SRT_ERR_ARG and call(None, rule, v, good) == abi.SRT_ERR_ARG
            assert call(abi.PathDesc(abi.SRT_PATH_DEPTH_MAX + 1, TMIN, None), None, v, good) == abi.SRT_ERR_LIMIT
            assert call(pd3, abi.ShadowRule(1e-3, 1.0, 2), v, good) == abi.SRT_ERR_ARG
    assert L.srt_shade_paths_refract(None, n, rp, None, C.byref(p), C.byref(pd3), None, None, C.byref(good), lp, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_shade_paths_refract(ds.h, n, None, None, C.byref(p), C.byref(pd3), None, None, C.byref(good), lp, None, None, None) == abi.SRT_ERR_ARG
    assert (lin == -9.0).all(), "an error touched an output"
    # nothing wanted, and n == 0: nothing to do
    assert L.srt_shade_paths_refract(ds.h, n, rp, None, C.byref(p), C.byref(pd3), None, None, C.byref(good), None, None, None, None) == abi.SRT_OK
    assert L.srt_shade_paths_refract(ds.h, 0, None, None, C.byref(p), C.byref(pd3), None, None, C.byref(good), lp, None, None, None) == abi.SRT_OK
    assert (lin == -9.0).all()
    # and the handle still works
    assert paths(pd3, rule, vis, good) == abi.SRT_OK and not (lin == -9.0).any()
    ds.close()


# ---- 9. the device forms, and hipGraph capture, in a process of its own ----------------------------------------------------------------
@gpu
def test_device_forms_and_graph_capture():
    r = subprocess.run([sys.executable, os.path.join(HERE, "refract_device_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "refract device case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 10. no GPU: the ABI surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from simple_raytracer_amd import build, lib
    build.build_all()
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "srt.h")).read()
    declared = set(re.findall(r"^int\s+(srt_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared and name in lib.ABI_SYMBOLS and hasattr(L, name), name
    assert re.search(r"typedef\s+struct\s+srt_refraction\s*\{\s*const\s+float\s*\*\s*ior\s*;.*?uint32_t\s+flags\s*;.*?\}\s*srt_refraction\s*;", hdr, re.S)
    assert re.search(r"#define\s+SRT_ABI_VERSION\s+3\b", hdr) and L.srt_abi_version() == 3      # additive only
    # refr comes directly after vis in all four
    for name in NEW:
        proto = re.search(r"^int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.M | re.S).group(1)
        assert re.search(r"const\s+srt_visibility\s*\*\s*vis\s*(/\*.*?\*/)?\s*,\s*const\s+srt_refraction\s*\*\s*refr", proto, re.S), name
    # what is left out, and the inward normals, are said in the header
    para = hdr[hdr.index("Refracting paths"):hdr.index("typedef struct srt_refraction")]
    assert "Fresnel" in para[para.index("NOT HERE"):] and "inside out" in para
    # the compiler's layout of the struct is the mirror's
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "srt.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(srt_refraction), '
                    'offsetof(srt_refraction, ior), offsetof(srt_refraction, flags)); return 0; }\n')
        exe = os.path.join(d, "size")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        size, o_ior, o_flags = (int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert (size, o_ior, o_flags) == (C.sizeof(abi.Refraction), abi.Refraction.ior.offset, abi.Refraction.flags.offset) == (16, 0, 8)
    for method in ("shade_paths", "shade_paths_device", "render_paths", "render_paths_device"):
        assert inspect.signature(getattr(lib.DeviceScene, method)).parameters["ior"].default is None, method
    # a NULL handle is refused without device work
    p, pd = abi.make_params(8, 8, abi.light_staircase(np.float32([0.0, 0.0, 0.0]), 1)), abi.PathDesc(2, 1e-3, None)
    rays, table = np.zeros((1, 6), np.float32), np.ones(1, np.float32)
    for refr in (None, abi.Refraction(table.ctypes.data, 0)):
        rr_ = C.byref(refr) if refr is not None else None
        assert L.srt_shade_paths_refract(None, 1, rays.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(p), C.byref(pd), None, None, rr_, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_shade_paths_refract_device(None, 1, rays.ctypes.data, None, C.byref(p), C.byref(pd), None, None, rr_, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_refract(None, C.byref(p), C.byref(pd), None, None, rr_, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_refract_device(None, C.byref(p), C.byref(pd), None, None, rr_, None, None, None, None) == abi.SRT_ERR_ARG
