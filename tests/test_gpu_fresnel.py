"""GPU (-m gpu): the Fresnel split (include/srt.h, "Fresnel split") -- srt_shade_paths_fresnel and srt_render_paths_fresnel pinned bit for
bit by tests/fresnel_ref.py where the batch is small enough for the yardstick (tests/test_fresnel_ref.py pins that yardstick to the
refracting one and the weight to Schlick's polynomial, and checks every case's input conditions), and by the chain of shipped host calls
-- the _refract call with seg, srt_surface_hits for the bounce rows, the depth-1 _masked call for the side rays, the mix in numpy --
where it is not.  Floats compare by bits; where the yardstick is NaN the device must be NaN.  The last test needs no GPU: the header
declares the four entry points and both structs, the library exports them, and the structs' layout is abi.py's."""
import ctypes as C
import functools
import inspect
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import fresnel_ref as fr
import golden_util as gu
import ray_query_ref as rq
import refract_edges as re_
import refract_ref as rf
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh
import surface_ref as sf
import visibility_ref as vr
from adversarial import with_vertex_normals
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
INF = np.float32(np.inf)
ALL = vr.ALL
TMIN = fr.BOUNCE_T_MIN
NEW = ("srt_shade_paths_fresnel_device", "srt_shade_paths_fresnel", "srt_render_paths_fresnel_device", "srt_render_paths_fresnel")
COUNTERS = ("node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow")
WANT = fr.ALL_KEYS
bits = sf.bits


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def cut(ref, sel):
    return {k: (v[sel] if k in ("rgb_linear", "rgb8") else v[:, sel]) for k, v in ref.items() if k in fr.ALL_KEYS}


def flat_rows(o):
    """A frame-shaped result as shade_paths lays it out: [rows, cols, ...] -> [n, ...], [depth, rows, cols, ...] -> [depth, n, ...]."""
    out = {}
    for key, v in o.items():
        if key in ("rgb_linear", "rgb8"):
            out[key] = v.reshape((v.shape[0] * v.shape[1],) + v.shape[2:])
        elif key in fr.ALL_KEYS:
            out[key] = v.reshape((v.shape[0], v.shape[1] * v.shape[2]) + v.shape[3:])
        else:
            out[key] = v
    return out


def check_stats(o, want, n, n_lights):
    hits = fr.hits_of(want)
    assert o["stats"]["primary_rays"] == n and o["stats"]["hit_rays"] == hits and o["stats"]["shadow_rays"] == hits * n_lights, (o["stats"], hits)


# ---- 1. frames of rays ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(fr.DEPTHS))
def test_frames_of_rays(srt, oracle, name):
    flat, rays, lights, refl = sp.frame_case(name)
    fr.condition(*fr.case_walks(oracle, name))
    want = fr.case_reference(oracle, name)
    assert (want["rgb8"] != rf.case_reference(oracle, name)["rgb8"]).any(), "the split changes no pixel"
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.shade_paths(rays, sq.shade_params(lights), fr.DEPTHS[name], refl, TMIN, count=count, ior=rf.case_ior(flat), fresnel=fr.case_f0(flat), want=WANT)
        fr.assert_same(o, want, f"{name}, counting {count}")
        check_stats(o, want, rays.shape[0], fr.N_LIGHTS)
    ds.close()


# ---- 2. wave and workgroup edges, order ----------------------------------------------------------------------------------------------
def leads_with_every_kind(segs, kinds, sides, first):
    """Among the first `first` rays: a split with both branches hitting, a total reflection and a mirror hit."""
    both = any(((s.hit >= 0) & walked & (segs[b + 1].hit >= 0))[:first].any() for b, (walked, F, s) in enumerate(sides) if b + 1 < len(segs))
    return both and any((k[:first] == rf.TIR).any() for k in kinds) and any((k[:first] == rf.MIRROR).any() for k in kinds)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """257 rays over cubes4_a40 whose first 63 hold a split with both branches hitting, a total reflection and a mirror hit:
    rq.unrelated_rays if they do, else a fixed shuffled subset of the frame's rays.  With 3 lights and the yardstick's rows at depth 3
    (computed once, never changed)."""
    from oracle import pyoracle
    flat, frame, lights, refl = sp.frame_case("cubes4_a40")
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    none = np.zeros((0, 3), np.float32)
    memo = vr.CandidateMemo(pyoracle, flat)
    rays = rq.unrelated_rays(flat, 257)
    if not leads_with_every_kind(*fr.trace(pyoracle, flat, rays[:63], none, 3, ior, f0, bounce_t_min=TMIN, cands=memo), 63):
        rays = np.ascontiguousarray(frame[np.random.default_rng(5).permutation(frame.shape[0])[:257]])
    assert leads_with_every_kind(*fr.trace(pyoracle, flat, rays[:63], none, 3, ior, f0, bounce_t_min=TMIN, cands=memo), 63), "the first 63 rays do not hold every kind"
    ref = fr.shade_paths(pyoracle, flat, rays, lights, 3, ior, f0, refl, TMIN, cands=memo)
    for v in ref.values():
        v.setflags(write=False)
    return flat, rays, lights, refl, ior, f0, ref


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_wave_and_block_edges(srt, n):
    flat, rays, lights, refl, ior, f0, ref = edge_batch()
    ds = srt.DeviceScene(flat)
    fr.assert_same(ds.shade_paths(rays[:n], sq.shade_params(lights), 3, refl, TMIN, ior=ior, fresnel=f0, want=WANT), cut(ref, slice(0, n)), f"n {n}")
    ds.close()


@gpu
def test_a_permuted_batch_gives_permuted_rows(srt):
    flat, rays, lights, refl, ior, f0, ref = edge_batch()
    perm = np.random.default_rng(3).permutation(rays.shape[0])
    ds = srt.DeviceScene(flat)
    # 16 lights: the deal of rays to waves is the spread one
    l16 = sq.lights_for("cubes4_a40", gu.GoldenScene("cubes4_a40").light, 16)
    for lt, want in ((lights, ref), (l16, None)):
        a = ds.shade_paths(rays, sq.shade_params(lt), 3, refl, TMIN, ior=ior, fresnel=f0, want=WANT)
        if want is not None:
            fr.assert_same(a, want, "in order")
        assert (a["side_hit_id"] >= 0).any()
        got = ds.shade_paths(np.ascontiguousarray(rays[perm]), sq.shade_params(lt), 3, refl, TMIN, ior=ior, fresnel=f0, want=WANT)
        fr.assert_same(got, cut(a, perm), f"permuted, {len(lt)} lights")
    o = ds.shade_paths(np.zeros((0, 6), np.float32), sq.shade_params(lights), 3, refl, TMIN, ior=ior, fresnel=f0, want=WANT)                  # n == 0
    assert o["rgb8"].shape == (0, 3) and o["side_hit_id"].shape == (3, 0)
    ds.close()


@gpu
def test_a_wave_that_splits_beside_one_that_does_not(srt, oracle):
    """128 rays in one call: 64 that all take a side ray at segment 0, then 64 of which none takes one at any segment -- the second wave
    never enters the side walk."""
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    want = fr.case_reference(oracle, name)
    _, _, sides = fr.case_walks(oracle, name)
    walked = np.stack([w for w, _, _ in sides])
    first, never = np.flatnonzero(walked[0])[:64], np.flatnonzero(~walked.any(axis=0) & (want["seg_hit_id"][0] >= 0))[:64]
    assert first.size == 64 and never.size == 64
    idx = np.concatenate([first, never])
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.shade_paths(rays[idx], sq.shade_params(lights), fr.DEPTHS[name], refl, TMIN, count=count, ior=rf.case_ior(flat), fresnel=fr.case_f0(flat), want=WANT)
        fr.assert_same(o, cut(want, idx), f"64 + 64, counting {count}")
        check_stats(o, cut(want, idx), idx.size, fr.N_LIGHTS)
    ds.close()


# ---- 3. identities -------------------------------------------------------------------------------------------------------------------
def raw_fresnel_paths(ds, rays, p, depth, refl, rule, vis, ior, fres):
    """srt_shade_paths_fresnel through the C ABI, so that fres and fres->f0 may be NULL: (rgb_linear, rgb8, seg_hit_id, stats)."""
    r = np.ascontiguousarray(rays, np.float32)
    n = r.shape[0]
    f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    lin, rgb8, hit = np.empty((n, 3), np.float32), np.empty((n, 3), np.uint8), np.empty((depth, n), np.int32)
    k = np.ascontiguousarray(refl, np.float32)
    pd, po, st = abi.PathDesc(depth, TMIN, k.ctypes.data), abi.PathOut(), abi.Stats()
    po.hit_id = hit.ctypes.data
    rule, vis, refr = abi.shadow_rule(rule), abi.visibility(vis), abi.Refraction(ior.ctypes.data, 0)
    ref = lambda v: C.byref(v) if v is not None else None
    rc = ds.L.srt_shade_paths_fresnel(ds.h, n, r.ctypes.data_as(f32p), None, C.byref(p), C.byref(pd), ref(rule), ref(vis), C.byref(refr), ref(fres),
                                      lin.ctypes.data_as(f32p), rgb8.ctypes.data_as(u8p), C.byref(po), C.byref(st))
    assert rc == abi.SRT_OK
    return lin, rgb8, hit, st.as_dict()


@gpu
def test_identities(srt):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    depth = fr.DEPTHS[name]
    nO = flat.n_objects
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    fp = rpr.camera_params(name, lights)
    ds = srt.DeviceScene(flat)
    for rule, vis in ((None, None), (sh.SELF, None), (sh.ENDED, (ALL, ALL, ALL))):
        p = sq.shade_params(lights, flags=abi.SRT_FLAG_COUNT_WORK)
        glass = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior)
        split = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior, fresnel=f0, want=WANT)
        assert (split["rgb8"] != glass["rgb8"]).any() and split["stats"]["hit_rays"] > glass["stats"]["hit_rays"], "the split changes nothing"
        sp.assert_same(split, glass, "the split changes a segment", sp.SEG_KEYS)
        # no table: fres NULL, or fres->f0 NULL
        side = np.full((depth, rays.shape[0]), 7, np.int32)
        fout = abi.FresnelOut(side.ctypes.data, None, None, None)
        for fres in (None, abi.Fresnel(None, 0, None), abi.Fresnel(None, 0, C.pointer(fout))):
            lin, rgb8, hit, st = raw_fresnel_paths(ds, rays, p, depth, refl, rule, vis, ior, fres)
            assert np.array_equal(bits(lin), bits(glass["rgb_linear"])) and np.array_equal(rgb8, glass["rgb8"]) and np.array_equal(hit, glass["seg_hit_id"]), (rule, vis)
            assert st == glass["stats"], (st, glass["stats"])
        assert (side == 7).all()
        # a table under which no object splits
        for label, table in (("-1", np.full(nO, -1.0, np.float32)), ("NaN", np.full(nO, np.nan, np.float32)), ("-inf", np.full(nO, -INF, np.float32)),
                             ("mirrors only", np.where(ior > 0, F32(-1e-45), F32(0.04)).astype(np.float32))):
            got = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior, fresnel=table, want=WANT)
            sp.assert_same(got, glass, f"f0 all {label}, rule {rule}, vis {vis}")
            assert got["stats"] == glass["stats"] and all(got["stats"][k] > 0 for k in COUNTERS), (label, got["stats"], glass["stats"])
            assert (got["side_hit_id"] == -1).all() and np.isposinf(got["side_t"]).all() and not bits(got["side_rgb_linear"]).any() and not bits(got["fresnel"]).any()
            frame = ds.render_paths(fp, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior)
            o = ds.render_paths(fp, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior, fresnel=table)
            sp.assert_same(rpr.flat_rows(o), rpr.flat_rows(frame), f"frame, f0 all {label}")
            assert o["stats"] == frame["stats"]
        # depth 1 is unchanged by any table
        one = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior)
        got = ds.shade_paths(rays, p, 1, refl, TMIN, shadow=rule, visibility=vis, count=True, ior=ior, fresnel=f0, want=WANT)
        sp.assert_same(got, one, "depth 1")
        assert got["stats"] == one["stats"] and (got["side_hit_id"] == -1).all() and not bits(got["fresnel"]).any()
        # the rows at depth D are the first D rows at depth D + 1
        for d in range(1, depth):
            less = ds.shade_paths(rays, p, d, refl, TMIN, shadow=rule, visibility=vis, ior=ior, fresnel=f0, want=fr.SIDE_KEYS + sp.SEG_KEYS)
            more = ds.shade_paths(rays, p, d + 1, refl, TMIN, shadow=rule, visibility=vis, ior=ior, fresnel=f0, want=fr.SIDE_KEYS + sp.SEG_KEYS)
            # (row d - 1 takes no side ray at depth d: b + 1 < depth -- the prefix is of the rows that can hold one)
            for k in fr.SIDE_KEYS:
                assert np.array_equal(bits(less[k][:d - 1]) if less[k].dtype == np.float32 else less[k][:d - 1],
                                      bits(more[k][:d - 1]) if more[k].dtype == np.float32 else more[k][:d - 1]), (k, d)
                assert not (less[k][d - 1] != {"side_hit_id": -1, "side_t": INF}.get(k, 0)).any(), (k, d)
            sp.assert_same({k: more[k][:d] for k in sp.SEG_KEYS}, {k: less[k] for k in sp.SEG_KEYS}, f"segments, depth {d}", sp.SEG_KEYS)
    ds.close()


# ---- 4. the chain of shipped host calls, on a batch too big for the yardstick ------------------------------------------------------------
def chain(ds, rays, params, depth, ior, f0, reflectance, smooth, rule, vis):
    """The chain the one launch replaces: the _refract call with seg (the path, its sums and its counters); per segment b + 1 < depth
    srt_surface_hits on the segment's live rays for the normal and the bounce row, refract_ref.refract_steps and fresnel_ref.schlick for
    who splits and F, the depth-1 _masked call on the side rays with the interval (bounce_t_min, +inf) and vis' = (bounce, bounce,
    shadow); the mix by fresnel_ref.mix.  Returns the rows, rgb_linear, and the sums of the calls' statistics."""
    n = rays.shape[0]
    base = ds.shade_paths(rays, params, depth, reflectance, TMIN, shadow=rule, visibility=vis, count=True, smooth=smooth, ior=ior)
    out = {k: base[k] for k in sp.SEG_KEYS}
    out.update(side_hit_id=np.full((depth, n), -1, np.int32), side_t=np.full((depth, n), INF, np.float32), side_rgb_linear=np.zeros((depth, n, 3), np.float32),
               fresnel=np.zeros((depth, n), np.float32))
    stats = {k: base["stats"][k] for k in ("hit_rays", "shadow_rays") + COUNTERS}
    both = 0
    for b in range(depth - 1):
        live = np.flatnonzero(base["seg_hit_id"][b] >= 0)
        if live.size == 0:
            break
        cur = np.ascontiguousarray(base["seg_rays"][b][live])
        f = ds.surface_hits(cur, base["seg_hit_id"][b][live], base["seg_t"][b][live], want=("obj", "normal", "bounce"), smooth=smooth)
        p = rf.refract_steps(cur[:, 3:6], f["normal"], ior[f["obj"]])
        with np.errstate(invalid="ignore"):
            walked = fr.splits(ior, f0)[f["obj"]] & ~(p["k"] < F32(0.0))
        if not walked.any():
            continue
        F = fr.schlick(f0[f["obj"]], p["entering"], p["dv"], p["k"])
        srays = np.ascontiguousarray(f["bounce"][walked])
        s = ds.shade_paths(srays, params, 1, None, TMIN, t_range=np.tile(F32([TMIN, INF]), (srays.shape[0], 1)), shadow=rule, visibility=(vis[1], vis[1], vis[2]),
                           count=True, smooth=smooth, want=("seg_hit_id", "seg_t", "seg_rgb_linear"))
        at = live[walked]
        out["side_hit_id"][b, at], out["side_t"][b, at], out["side_rgb_linear"][b, at], out["fresnel"][b, at] = s["seg_hit_id"][0], s["seg_t"][0], s["seg_rgb_linear"][0], F[walked]
        both += int(((s["seg_hit_id"][0] >= 0) & (base["seg_hit_id"][b + 1][at] >= 0)).sum())
        for k in stats:
            stats[k] += s["stats"][k]
    out["rgb_linear"] = fr.mix(out["seg_hit_id"], out["seg_obj"], out["seg_rgb_linear"], out["side_hit_id"], out["side_rgb_linear"], out["fresnel"], reflectance)
    out["stats"] = stats
    return out, both


@gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_chain_equality_and_counters(srt, smooth):
    """Under a shadow rule and the masks (1, 2, 4): the ground carries every bit, the bunny none of the shadow rays' -- it casts no shadow."""
    flat, rays, lights, refl = sp.frame_case("ground_bunny")
    flat = with_vertex_normals(flat)
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    depth, rule, vis = 4, sh.SELF, (1, 2, 4)
    table = np.uint32([7, 3])
    assert flat.n_objects == 2
    p = sq.shade_params(lights, flags=abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0)
    ds = srt.DeviceScene(flat)
    ds.set_object_masks(table)
    want, both = chain(ds, rays, p, depth, ior, f0, refl, smooth, rule, vis)
    assert both > 0 and (want["side_hit_id"][depth - 2] >= 0).any() and (want["side_hit_id"][depth - 1] == -1).all()
    o = ds.shade_paths(rays, p, depth, refl, TMIN, shadow=rule, visibility=vis, count=True, smooth=smooth, ior=ior, fresnel=f0, want=WANT)
    fr.assert_same(o, want, f"ground_bunny, depth {depth}, smooth {smooth}", ("rgb_linear",) + sp.SEG_KEYS + fr.SIDE_KEYS)
    hits = fr.hits_of(want)
    assert o["stats"]["primary_rays"] == rays.shape[0] and o["stats"]["hit_rays"] == hits == want["stats"]["hit_rays"]
    assert o["stats"]["shadow_rays"] == hits * len(lights) == want["stats"]["shadow_rays"]
    for k in COUNTERS:
        assert o["stats"][k] == want["stats"][k] > 0, (k, o["stats"], want["stats"])
    ds.close()


# ---- 5. the frame form ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name,size", [("cubes4_a40", (48, 27)), ("ground_bunny", (40, 24))])
def test_a_frame_is_its_rays(srt, name, size):
    """spp = 1: srt_render_paths_fresnel equals srt_shade_paths_fresnel on the frame's rays; a 2-way deal of blocks of 8 rows and a 2-way
    deal of 8 x 16 tiles write the whole-frame call's values (padding keeps the fill)."""
    g = gu.GoldenScene(name)
    flat, lights = g.flat, sq.lights_for(name, g.light, 2)
    refl, ior, f0 = np.float32(sp.REFLECTANCE[:flat.n_objects]), rf.case_ior(flat), fr.case_f0(flat)
    depth = 3
    p = rpr.camera_params(name, lights, *size)
    rays, live = rpr.frame_rays_owned(p)
    assert live.all()
    ds = srt.DeviceScene(flat)
    for rule in (None, sh.SELF):
        whole = flat_rows(ds.render_paths(p, depth, refl, TMIN, shadow=rule, ior=ior, fresnel=f0, want=WANT, count=True))
        want = ds.shade_paths(rays.reshape(-1, 6), sq.shade_params(lights), depth, refl, TMIN, shadow=rule, ior=ior, fresnel=f0, want=WANT, count=True)
        assert (want["side_hit_id"][1] >= 0).any()
        fr.assert_same(whole, want, f"{name}, rule {rule}")
        for k in ("primary_rays", "hit_rays", "shadow_rays") + COUNTERS:
            assert whole["stats"][k] == want["stats"][k] > 0, (k, whole["stats"], want["stats"])
        for kw in (dict(block_rows=8, block_stride=2), dict(block_rows=8, block_cols=16, block_stride=2)):
            seen = np.zeros(live.size, bool)
            for first in range(2):
                share = rpr.camera_params(name, lights, *size, block_first=first, **kw)
                own = rpr.owned(share).reshape(-1)
                o = flat_rows(ds.render_paths(share, depth, refl, TMIN, fill=7, shadow=rule, ior=ior, fresnel=f0, want=WANT))
                mine = np.flatnonzero(own >= 0)
                assert mine.size
                fr.assert_same(cut(o, mine), cut(whole, own[mine]), f"{name}, share {first} of 2, {kw}, rule {rule}")
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
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    w, h = 24, 14
    p = rpr.camera_params(name, lights, w, h, spp=4)
    want = fr.render_paths(oracle, flat, p, 3, ior, f0, refl, TMIN, rule=sh.SELF)
    assert (want["side_hit_id"][1] >= 0).any() and (want["seg_hit_id"][2] >= 0).any()
    ds = srt.DeviceScene(flat)
    o = ds.render_paths(p, 3, refl, TMIN, shadow=sh.SELF, count=True, ior=ior, fresnel=f0, want=WANT)
    fr.assert_same(flat_rows(o), flat_rows(want), "spp 4")
    assert o["stats"]["primary_rays"] == w * h * 4
    ds.close()


# ---- 6. errors ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_errors(srt):
    name = "cubes4_a40"
    flat, rays, lights, refl = sp.frame_case(name)
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    ds = srt.DeviceScene(flat)
    L = ds.L
    f32p = C.POINTER(C.c_float)
    n = 8
    r = np.ascontiguousarray(rays[:n])
    rp = r.ctypes.data_as(f32p)
    p, fp = sq.shade_params(lights), rpr.camera_params(name, lights, 4, 2)
    lin = np.full((n, 3), -9.0, np.float32)
    side = {k: np.full((3, n) + ((3,) if k == "rgb_linear" else ()), -9, ty) for k, (ty, _) in abi.FRESNEL_FIELDS.items()}
    fout = abi.FresnelOut(*(side[k].ctypes.data for k in abi.FRESNEL_FIELDS))
    lp = lin.ctypes.data_as(f32p)
    ref = lambda v: C.byref(v) if v is not None else None
    refr = abi.Refraction(ior.ctypes.data, 0)
    good, bad = abi.Fresnel(f0.ctypes.data, 0, C.pointer(fout)), abi.Fresnel(f0.ctypes.data, 1, C.pointer(fout))
    vis, rule = abi.visibility((1, 2, 4)), abi.shadow_rule(sh.ENDED)
    pd3 = abi.PathDesc(3, TMIN, None)
    paths = lambda pd, rule_, vis_, refr_, fres: L.srt_shade_paths_fresnel(ds.h, n, rp, None, C.byref(p), ref(pd), ref(rule_), ref(vis_), ref(refr_), ref(fres), lp, None, None, None)
    frame = lambda pd, rule_, vis_, refr_, fres: L.srt_render_paths_fresnel(ds.h, C.byref(fp), ref(pd), ref(rule_), ref(vis_), ref(refr_), ref(fres), lp, None, None, None)
    # the _device forms are refused before any pointer is read
    paths_d = lambda pd, rule_, vis_, refr_, fres: L.srt_shade_paths_fresnel_device(ds.h, n, r.ctypes.data, None, C.byref(p), ref(pd), ref(rule_), ref(vis_), ref(refr_),
                                                                                    ref(fres), None, lin.ctypes.data, None, None)
    frame_d = lambda pd, rule_, vis_, refr_, fres: L.srt_render_paths_fresnel_device(ds.h, C.byref(fp), ref(pd), ref(rule_), ref(vis_), ref(refr_), ref(fres), None,
                                                                                     lin.ctypes.data, None, None)
    for call in (paths, frame, paths_d, frame_d):
        for v in (None, vis):
            # flags other than 0, with and without the tables
            assert call(pd3, rule, v, refr, bad) == abi.SRT_ERR_ARG and call(pd3, None, v, None, abi.Fresnel(None, 1 << 31, None)) == abi.SRT_ERR_ARG
            assert call(pd3, rule, v, abi.Refraction(ior.ctypes.data, 1), good) == abi.SRT_ERR_ARG
            # every error of the _refract call keeps its code with a table present
            assert call(abi.PathDesc(0, TMIN, None), rule, v, refr, good) == abi.SRT_ERR_ARG and call(None, rule, v, refr, good) == abi.SRT_ERR_ARG
            assert call(abi.PathDesc(abi.SRT_PATH_DEPTH_MAX + 1, TMIN, None), None, v, refr, good) == abi.SRT_ERR_LIMIT
            assert call(pd3, abi.ShadowRule(1e-3, 1.0, 2), v, refr, good) == abi.SRT_ERR_ARG
    assert L.srt_shade_paths_fresnel(None, n, rp, None, C.byref(p), C.byref(pd3), None, None, C.byref(refr), C.byref(good), lp, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_shade_paths_fresnel(ds.h, n, None, None, C.byref(p), C.byref(pd3), None, None, C.byref(refr), C.byref(good), lp, None, None, None) == abi.SRT_ERR_ARG
    assert (lin == -9.0).all() and all((v == -9).all() for v in side.values()), "an error touched an output"
    # nothing wanted, the fields of out included, and n == 0: nothing to do
    empty = abi.FresnelOut()
    nothing = abi.Fresnel(f0.ctypes.data, 0, C.pointer(empty))
    assert L.srt_shade_paths_fresnel(ds.h, n, rp, None, C.byref(p), C.byref(pd3), None, None, C.byref(refr), C.byref(nothing), None, None, None, None) == abi.SRT_OK
    assert L.srt_shade_paths_fresnel(ds.h, 0, None, None, C.byref(p), C.byref(pd3), None, None, C.byref(refr), C.byref(good), lp, None, None, None) == abi.SRT_OK
    assert (lin == -9.0).all() and all((v == -9).all() for v in side.values())
    # the side rows alone are an output: the call runs, and writes them and nothing else
    assert L.srt_shade_paths_fresnel(ds.h, n, rp, None, C.byref(p), C.byref(pd3), None, None, C.byref(refr), C.byref(good), None, None, None, None) == abi.SRT_OK
    assert (lin == -9.0).all() and not any((v == -9).any() for v in side.values())
    want = ds.shade_paths(r, p, 3, None, TMIN, ior=ior, fresnel=f0, want=fr.SIDE_KEYS)
    for k in abi.FRESNEL_FIELDS:
        fr.assert_same({"x": side[k]}, {"x": want["fresnel" if k == "fresnel" else "side_" + k]}, f"the side rows alone, {k}", ("x",))
    # and the handle still works
    assert paths(pd3, rule, vis, refr, good) == abi.SRT_OK and not (lin == -9.0).any()
    ds.close()


# ---- 7. the device forms, and hipGraph capture, in a process of its own ----------------------------------------------------------------
@gpu
def test_device_forms_and_graph_capture():
    r = subprocess.run([sys.executable, os.path.join(HERE, "fresnel_device_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fresnel device case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- 8. the weight at its edges ---------------------------------------------------------------------------------------------------------
F0_EDGES = {"0": 0.0, "0.04": 0.04, "1": 1.0, "-0": -0.0, "subnormal": 1e-45, "-1": -1.0, "NaN": np.nan}


@functools.lru_cache(maxsize=None)
def edge_sides(label, smooth):
    """The yardstick's side rows (hit, t, F) of refract_edges' batch at depth 2 under a table that holds F0_EDGES[label] for every object:
    the walks alone, no light is needed for them."""
    from oracle import pyoracle
    flat, rays = re_.scene(), re_.batch()[0]
    f0 = np.full(flat.n_objects, F0_EDGES[label], np.float32)
    flags = abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0
    _, _, sides = fr.trace(pyoracle, flat, rays, np.zeros((0, 3), np.float32), 2, re_.IOR, f0, bounce_t_min=re_.BOUNCE_T_MIN, flags=flags, cands=edge_memo())
    walked, F, s = sides[0]
    return walked, F, s.hit, s.t


@functools.lru_cache(maxsize=None)
def edge_memo():
    from oracle import pyoracle
    return vr.CandidateMemo(pyoracle, re_.scene())


@gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_the_weight_at_its_edges(srt, smooth):
    """refract_edges' sheets (ior 1, 1.5, 2, 0.5, the one-ulp sweeps across the critical angle, long and short d): out.fresnel, out.hit_id
    and out.t bit for bit under every f0 of F0_EDGES; NaN where the yardstick's arithmetic is NaN."""
    flat, (rays, kind, sheet, scale) = re_.scene(), re_.batch()
    ds = srt.DeviceScene(flat)
    for label in F0_EDGES:
        walked, F, hit, t = edge_sides(label, smooth)
        f0 = np.full(flat.n_objects, F0_EDGES[label], np.float32)
        if label in ("-1", "NaN"):
            assert not walked.any()
        else:
            sweep = kind == re_.KIND_SWEEP
            assert walked[sweep].any() and not walked[sweep].all(), "the sweeps do not cross the critical angle"
            assert np.isnan(F[walked]).any() and (hit[walked] >= 0).any() and (hit[walked] < 0).any()
            if label == "0.04":
                assert (F[walked & ~np.isnan(F)] >= F32(0.04)).all() and (F[walked] == F32(1.0)).any() and (F[walked] == F32(0.04)).any()
        o = ds.shade_paths(rays, sq.shade_params(re_.lights(1)), 2, re_.REFLECTANCE, re_.BOUNCE_T_MIN, smooth=smooth, ior=re_.IOR, fresnel=f0, want=fr.SIDE_KEYS)
        want = {"fresnel": np.stack([F, np.zeros_like(F)]), "side_hit_id": np.stack([hit, np.full_like(hit, -1)]), "side_t": np.stack([t, np.full_like(t, INF)])}
        fr.assert_same(o, want, f"f0 {label}, smooth {smooth}", ("fresnel", "side_hit_id", "side_t"))
    ds.close()


# ---- 9. no GPU: the ABI surface ---------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    from simple_raytracer_amd import build, lib
    build.build_all()
    L = lib.load()
    hdr = open(os.path.join(ROOT, "include", "srt.h")).read()
    declared = set(re.findall(r"^int\s+(srt_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in NEW:
        assert name in declared and name in lib.ABI_SYMBOLS and hasattr(L, name), name
    assert re.search(r"typedef\s+struct\s+srt_fresnel_out\s*\{\s*(/\*.*?\*/)?\s*int32_t\s*\*\s*hit_id\s*;.*?float\s*\*\s*t\s*;.*?float\s*\*\s*rgb_linear\s*;.*?float\s*\*\s*fresnel\s*;.*?\}\s*srt_fresnel_out\s*;",
                     hdr, re.S)
    assert re.search(r"typedef\s+struct\s+srt_fresnel\s*\{\s*const\s+float\s*\*\s*f0\s*;.*?uint32_t\s+flags\s*;.*?const\s+srt_fresnel_out\s*\*\s*out\s*;.*?\}\s*srt_fresnel\s*;", hdr, re.S)
    assert re.search(r"#define\s+SRT_ABI_VERSION\s+3\b", hdr) and L.srt_abi_version() == 3      # additive only
    # fres comes directly after refr in all four
    for name in NEW:
        proto = re.search(r"^int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, re.M | re.S).group(1)
        assert re.search(r"const\s+srt_refraction\s*\*\s*refr\s*(/\*.*?\*/)?\s*,\s*const\s+srt_fresnel\s*\*\s*fres", proto, re.S), name
    # the definition is in the header: who splits, the weight, the mix
    para = hdr[hdr.index("Fresnel split: glass"):hdr.index("typedef struct srt_fresnel_out")]
    for text in ("ior[k] > 0.0f && f0[k] >= 0.0f", "entering ? -dv : sqrtf(k)", "(m2 * m2) * m", "Wk * (1.0f - Fe)", "b + 1 < depth"):
        assert text in para, text
    # the compiler's layout of the structs is the mirror's
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "size.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "srt.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(srt_fresnel), '
                    'offsetof(srt_fresnel, f0), offsetof(srt_fresnel, flags), offsetof(srt_fresnel, out), sizeof(srt_fresnel_out), offsetof(srt_fresnel_out, hit_id), '
                    'offsetof(srt_fresnel_out, t), offsetof(srt_fresnel_out, rgb_linear), offsetof(srt_fresnel_out, fresnel)); return 0; }\n')
        exe = os.path.join(d, "size")
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True, capture_output=True)
        got = tuple(int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    A, O = abi.Fresnel, abi.FresnelOut
    assert got == (C.sizeof(A), A.f0.offset, A.flags.offset, A.out.offset, C.sizeof(O), O.hit_id.offset, O.t.offset, O.rgb_linear.offset, O.fresnel.offset) \
        == (24, 0, 8, 16, 32, 0, 8, 16, 24)
    for method in ("shade_paths", "shade_paths_device", "render_paths", "render_paths_device"):
        assert inspect.signature(getattr(lib.DeviceScene, method)).parameters["fresnel"].default is None, method
    assert lib.schlick_f0(1.5) == F32(0.04)
    # a NULL handle is refused without device work
    p, pd = abi.make_params(8, 8, abi.light_staircase(np.float32([0.0, 0.0, 0.0]), 1)), abi.PathDesc(2, 1e-3, None)
    rays, table = np.zeros((1, 6), np.float32), np.ones(1, np.float32)
    refr = abi.Refraction(table.ctypes.data, 0)
    for fres in (None, abi.Fresnel(table.ctypes.data, 0, None)):
        ff = C.byref(fres) if fres is not None else None
        assert L.srt_shade_paths_fresnel(None, 1, rays.ctypes.data_as(C.POINTER(C.c_float)), None, C.byref(p), C.byref(pd), None, None, C.byref(refr), ff, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_shade_paths_fresnel_device(None, 1, rays.ctypes.data, None, C.byref(p), C.byref(pd), None, None, C.byref(refr), ff, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_fresnel(None, C.byref(p), C.byref(pd), None, None, C.byref(refr), ff, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_fresnel_device(None, C.byref(p), C.byref(pd), None, None, C.byref(refr), ff, None, None, None, None) == abi.SRT_ERR_ARG
