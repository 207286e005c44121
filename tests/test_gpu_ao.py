"""GPU (-m gpu): srt_ao_rays / srt_ao_hits (include/srt.h, "Ambient occlusion") -- the hemisphere visibility at a hit in one launch --
pinned bit for bit by tests/ao_ref.py, which composes the answer from the yardsticks of the calls the definition names (tests/test_ao_ref.py
pins that file's own arithmetic and the input conditions of the cases used here).  Ints compare by value, floats by bits."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import adversarial as adv
import ao_ref as ar
import golden_util as gu
import ray_query_ref as rq
import render_paths_ref as rpr
import shade_query_ref as sq
import shadow_rule_ref as sh
import tree_shapes as ts
import visibility_ref as vr
from simple_raytracer_amd import abi

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
INF = np.float32(np.inf)
K = ar.N_DIRS
DIRS = ar.directions(K)
ALL = ("hit_id", "t") + ar.FIELDS
ALL_ONES = 0xFFFFFFFF
SHADOW_KEYS = ("node_tests_shadow", "tri_tests_shadow")
PRIMARY_KEYS = ("node_tests_primary", "tri_tests_primary")
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    assert np.array_equal(bits(lib.ao_directions(K)), bits(DIRS)) and np.array_equal(bits(lib.ao_directions(130, False)), bits(ar.directions(130, False)))
    return lib


def check(o, want, what, keys=ALL, n_dirs=K):
    ar.assert_same(o, want, what, keys)
    if "stats" in o:
        hits = int((want["hit_id"] >= 0).sum())
        st = o["stats"]
        assert st["primary_rays"] == want["hit_id"].shape[0] and st["hit_rays"] == hits and st["shadow_rays"] == hits * n_dirs, (what, st)


def rows(ref, idx):
    return {k: v[idx] for k, v in ref.items() if k != "stats"}


def miss_rows(ref, where):
    """`ref` with the rows `where` turned into miss rows."""
    out = {k: v.copy() for k, v in ref.items()}
    out["hit_id"][where] = -1; out["t"][where] = INF; out["n_occluded"][where] = 0; out["ao"][where] = 1.0; out["occ_bits"][where] = 0
    return out


# ---- 1. against the yardstick ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(ar.STRIDE))
def test_lamp_cases_against_the_yardstick(srt, oracle, name):
    c = ar.case(oracle, name)
    ds = srt.DeviceScene(c.flat)
    for t_max in ar.RADII:
        for skip in (False, True):
            want = c.reference(t_max=t_max, skip_self=skip)
            for count in (False, True):
                o = ds.ao_rays(c.rays, DIRS, t_max=t_max, skip_self=skip, count=count)
                check(o, want, f"{name}, t_max {t_max}, skip_self {skip}, counting {count}")
                assert (o["stats"]["node_tests_shadow"] > 0) == count and (o["stats"]["node_tests_primary"] > 0) == count
    ds.close()


@functools.lru_cache(maxsize=None)
def smooth_case():
    """The scene with vertex normals tests/test_gpu_surface.py uses, at its frame of rays; flat and smooth."""
    from oracle import pyoracle
    flat = sq.texquad_with_normals(gu.GoldenScene("texquad"))
    rays = rq.frame_rays(48, 27, rq.SHEAR, rq.FOCAL["texquad"] * 48 / rq.FRAME_W)
    return flat, rays, ar.Case(pyoracle, flat, rays, DIRS, smooth=True), ar.Case(pyoracle, flat, rays, DIRS)


@gpu
def test_smooth_normals_against_the_yardstick(srt):
    flat, rays, smooth, plain = smooth_case()
    assert smooth.sel.size * 10 >= rays.shape[0] and np.any(bits(smooth.Nf) != bits(plain.Nf)), "the smooth normal must differ"
    want, flat_want = smooth.reference(t_min=1e-3, t_max=INF), plain.reference(t_min=1e-3, t_max=INF)
    assert np.any(want["occ_bits"] != flat_want["occ_bits"]), "the tilted hemisphere must meet the quad itself"
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        check(ds.ao_rays(rays, DIRS, smooth=True, count=count), want, f"smooth, counting {count}")
    check(ds.ao_rays(rays, DIRS), flat_want, "the same scene, face normals")
    o = ds.ao_rays(rays, DIRS, smooth=True)
    ar.assert_same(ds.ao_hits(rays, o["hit_id"], o["t"], DIRS, smooth=True), want, "ao_hits, smooth", ar.FIELDS)
    ds.close()


# ---- 2. against the chain of shipped calls ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("skip,shadow", [(False, None), (True, None), (False, 2), (True, 1)])
def test_the_chain_of_shipped_calls_gives_the_same_bits(srt, skip, shadow):
    """surface_rays -> the AO rays in numpy -> occluded(t_range, ray_mask) -> pack: what the call replaces."""
    flat, rays = ar.case_rays("cube_ground")
    ds = srt.DeviceScene(flat)
    table = vr.case_table(flat)
    if shadow is not None:
        ds.set_object_masks(table)
    s = ds.surface_rays(rays, want=("hit_id", "t", "obj", "point", "normal"))
    sel = np.flatnonzero(s["hit_id"] >= 0)
    T, B, Nf = ar.frame(rays[sel, 3:6], s["normal"][sel])
    aor = ar.ao_rays(s["point"][sel], T, B, Nf, DIRS).reshape(-1, 6)
    occ = ds.occluded(aor, np.repeat(s["obj"][sel], K).astype(np.int32) if skip else None, t_range=np.tile(np.float32([1e-3, 60.0]), (aor.shape[0], 1)),
                      ray_mask=True if shadow is None else np.full(aor.shape[0], shadow, np.uint32))
    full = np.zeros((rays.shape[0], K), bool); full[sel] = occ.reshape(-1, K).astype(bool)
    cnt, ao, words = ar.pack(full)
    assert 0 < cnt.sum() < full.size
    want = {"hit_id": s["hit_id"], "t": s["t"], "n_occluded": cnt, "ao": ao, "occ_bits": words}
    vis = None if shadow is None else (ALL_ONES, 0, shadow)
    check(ds.ao_rays(rays, DIRS, t_max=60.0, skip_self=skip, visibility=vis), want, f"chain, skip_self {skip}, shadow mask {shadow}")
    ds.close()


# ---- 3. shapes the deal can get wrong --------------------------------------------------------------------------------------------------
N_DIRS = (1, 7, 63, 64, 65, 130)      # a partial last chunk, exactly one chunk, two words, three chunks; 1 and 7 take the other deal of rays to waves
BIG = ar.directions(130, cosine=False)


@functools.lru_cache(maxsize=None)
def shape_case():
    """cube_ground's frame at the 65-direction prefix of BIG, radius 60: the yardstick, once."""
    from oracle import pyoracle
    flat, rays = ar.case_rays("cube_ground")
    c = ar.Case(pyoracle, flat, rays, BIG[:65])
    return flat, rays, c.reference(t_max=60.0)


@gpu
def test_direction_counts_are_prefixes_and_concatenations(srt):
    flat, rays, want65 = shape_case()
    n = rays.shape[0]
    ds = srt.DeviceScene(flat)
    o = {k: ds.ao_rays(rays, BIG[:k], t_max=60.0) for k in N_DIRS}
    check(o[65], want65, "65 directions", n_dirs=65)
    whole = ar.unpack(o[130]["occ_bits"], 130)
    assert 0 < whole[:, :1].sum() and whole[:, 65:].any() and not whole.all(axis=0).any()
    for k in N_DIRS:
        got = ar.unpack(o[k]["occ_bits"], k)
        assert o[k]["occ_bits"].shape == (n, (k + 31) // 32) and np.array_equal(got, whole[:, :k]), f"{k} directions are not a prefix of 130"
        cnt, ao, words = ar.pack(got)
        assert np.array_equal(o[k]["occ_bits"], words), f"{k}: a bit >= n_dirs is set"
        assert np.array_equal(o[k]["n_occluded"], cnt) and np.array_equal(bits(o[k]["ao"]), bits(ao)), k
        assert np.array_equal(o[k]["hit_id"], o[130]["hit_id"]) and np.array_equal(bits(o[k]["t"]), bits(o[130]["t"]))
    tail = ds.ao_rays(rays, BIG[65:], t_max=60.0)
    assert np.array_equal(np.concatenate([ar.unpack(o[65]["occ_bits"], 65), ar.unpack(tail["occ_bits"], 65)], axis=1), whole)
    mid = ds.ao_rays(rays, BIG[7:64], t_max=60.0)
    assert np.array_equal(ar.unpack(mid["occ_bits"], 57), whole[:, 7:64])
    ds.close()


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1296])
def test_ray_counts(srt, oracle, n):
    c = ar.case(oracle, "cube_ground")
    ds = srt.DeviceScene(c.flat)
    want = rows(c.reference(t_max=60.0), slice(0, n))
    o = ds.ao_rays(c.rays[:n], DIRS, t_max=60.0)
    check(o, want, f"n {n}")
    check(ds.ao_hits(c.rays[:n], o["hit_id"], o["t"], DIRS, t_max=60.0), want, f"n {n}, ao_hits", ar.FIELDS)
    ds.close()


SPREAD_FROM = 8      # srt_hip.hip's SRT_AO_SPREAD_FROM: from this many directions on a wave owns 8 groups of 8 rays instead of 64 consecutive ones


def wave_of(n, spread):
    """The wave (workgroup * 4 + wave in it) that owns each of n rays under k_query_ao's two deals: the grid is ceil(n / 256) workgroups;
    block: ray ri is lane ri % 64 of wave ri // 64; spread: lane l of wave wv owns ray ((l >> 3) * n_waves + wv) * 8 + (l & 7)."""
    ri = np.arange(n)
    n_waves = (n + 255) // 256 * 4
    return (ri // 8) % n_waves if spread else ri // 64


def per_wave(n, spread, is_hit):
    """[(live rays, hits)] of every wave of the grid."""
    w = wave_of(n, spread)
    n_waves = (n + 255) // 256 * 4
    return [(int((w == k).sum()), int(is_hit[w == k].sum())) for k in range(n_waves)]


def wave_batch(spread, miss, hits, n=512):
    """Indices into a case's rays for a batch of n = 512 rays (8 waves) laid out for one deal: wave 0 gets 64 misses, wave 1 64 different
    hits, wave 2 64 copies of one hit, wave 3 five hits among misses, the other waves hits and misses as they come."""
    w = wave_of(n, spread)
    idx = np.resize(np.concatenate([hits[64:], miss]), n)
    at = lambda k: np.flatnonzero(w == k)
    idx[at(0)] = np.resize(miss, 64)
    idx[at(1)] = hits[:64]
    idx[at(2)] = hits[3]
    idx[at(3)] = np.concatenate([hits[10:15], np.resize(miss, 59)])
    return idx


@gpu
def test_waves_without_a_hit_full_waves_and_order(srt, oracle):
    c = ar.case(oracle, "cube_ground")
    flat, rays65, ref65 = shape_case()
    assert np.array_equal(rays65, c.rays)
    ref16 = c.reference(t_max=60.0)
    cnt, ao, words = ar.pack(ar.unpack(ref16["occ_bits"], K)[:, :7])      # a table's row is the concatenation of its parts' rows
    ref7 = dict(ref16, n_occluded=cnt, ao=ao, occ_bits=words)
    tables = {7: (DIRS[:7], ref7), 16: (DIRS, ref16), 65: (BIG[:65], ref65)}
    assert any(k < SPREAD_FROM for k in tables) and any(k >= SPREAD_FROM for k in tables), "both deals must be reached"
    miss, partial = np.flatnonzero(ref16["hit_id"] < 0), np.flatnonzero((ref16["n_occluded"] > 0) & (ref16["n_occluded"] < K))
    assert miss.size and partial.size >= 70 and (ref65["n_occluded"][partial[:64]] > 0).any()
    ds = srt.DeviceScene(c.flat)
    for laid_out_for_spread in (False, True):
        idx = wave_batch(laid_out_for_spread, miss, partial)
        is_hit = ref16["hit_id"][idx] >= 0
        # under the deal it is laid out for: a wave with no hit (no item, a zero row from every lane), a full wave of different hits
        # (4096 items a chunk, every slot of the wave's words in use), a full wave of 64 equal rows, a wave of five hits
        assert per_wave(idx.size, laid_out_for_spread, is_hit)[:4] == [(64, 0), (64, 64), (64, 64), (64, 5)]
        assert per_wave(idx.size, not laid_out_for_spread, is_hit)[:4] != [(64, 0), (64, 64), (64, 64), (64, 5)]
        for k, (dirs, ref) in tables.items():      # every table on every layout: each layout meets its own deal whatever the rule's threshold is
            what = f"batch laid out for the {'spread' if laid_out_for_spread else 'block'} deal, {k} directions ({'spread' if k >= SPREAD_FROM else 'block'} deal)"
            o = ds.ao_rays(c.rays[idx], dirs, t_max=60.0)
            check(o, rows(ref, idx), what, n_dirs=k)
            check(ds.ao_hits(c.rays[idx], o["hit_id"], o["t"], dirs, t_max=60.0), rows(ref, idx), what + ", ao_hits", ar.FIELDS, n_dirs=k)
    # a ragged batch: the first 64 rays miss, 70 hits follow (under the block deal waves of (64, 0), (64, 64), (6, 6))
    idx = np.concatenate([np.resize(miss, 64), partial[:70]])
    assert per_wave(idx.size, False, ref16["hit_id"][idx] >= 0) == [(64, 0), (64, 64), (6, 6), (0, 0)]
    for k, (dirs, ref) in tables.items():
        check(ds.ao_rays(c.rays[idx], dirs, t_max=60.0), rows(ref, idx), f"ragged batch, {k} directions", n_dirs=k)
    # a permutation of the rays permutes the rows, under either deal
    perm = np.random.default_rng(4).permutation(c.rays.shape[0])
    for k, (dirs, ref) in tables.items():
        check(ds.ao_rays(np.ascontiguousarray(c.rays[perm]), dirs, t_max=60.0), rows(ref, perm), f"permuted, {k} directions", n_dirs=k)
    ds.close()


# ---- 4. srt_ao_hits --------------------------------------------------------------------------------------------------------------------
@gpu
def test_ao_hits(srt, oracle):
    c = ar.case(oracle, "cubes4_a40")
    flat, rays = c.flat, c.rays
    n = rays.shape[0]
    ds = srt.DeviceScene(flat)
    for skip in (False, True):
        want = c.reference(t_max=60.0, skip_self=skip)
        o = ds.ao_rays(rays, DIRS, t_max=60.0, skip_self=skip)
        h = ds.ao_hits(rays, o["hit_id"], o["t"], DIRS, t_max=60.0, skip_self=skip, count=True)
        check(dict(h, hit_id=o["hit_id"], t=o["t"]), want, f"ao_hits on ao_rays' hits, skip_self {skip}")
        assert h["stats"]["node_tests_primary"] == 0 and h["stats"]["tri_tests_primary"] == 0 and h["stats"]["node_tests_shadow"] > 0
        for k in ar.FIELDS:      # each output alone
            one = ds.ao_hits(rays, o["hit_id"], o["t"], DIRS, t_max=60.0, skip_self=skip, want=(k,))
            assert set(one) == {k, "stats"}
            ar.assert_same(one, want, f"ao_hits, only {k}", (k,))
    # ids outside [0, n_tris) are miss rows, whatever t says
    ids = np.resize(np.int32([-1, flat.n_tris, -2 ** 31, 2 ** 31 - 1]), n)
    h = ds.ao_hits(rays, ids, np.resize(np.float32([1.0, np.nan, INF, -3.0]), n), DIRS)
    assert (h["n_occluded"] == 0).all() and (bits(h["ao"]) == bits(np.float32(1.0))).all() and (h["occ_bits"] == 0).all() and h["stats"]["hit_rays"] == 0
    ds.close()


@gpu
def test_ao_hits_on_a_rendered_frame(srt):
    """A render's hit_id / t with the frame's own rays: the AO pass that needs no second closest-hit walk."""
    flat, _, lights, _ = sh.lamp_case("cube_ground")
    p = rpr.camera_params("cube_ground", lights)
    rays, live = rpr.frame_rays_owned(p)
    assert live.all()
    rays = np.ascontiguousarray(rays.reshape(-1, 6))
    ds = srt.DeviceScene(flat)
    frame = ds.render(p, want=("hit_id", "t"))
    o = ds.ao_rays(rays, DIRS, t_max=60.0)
    assert np.array_equal(frame["hit_id"].reshape(-1), o["hit_id"]) and np.array_equal(bits(frame["t"].reshape(-1)), bits(o["t"]))
    assert 0 < (o["n_occluded"] > 0).sum() < (o["hit_id"] >= 0).sum()
    ar.assert_same(ds.ao_hits(rays, frame["hit_id"].reshape(-1), frame["t"].reshape(-1), DIRS, t_max=60.0), o, "a render's hits", ar.FIELDS)
    ds.close()


# ---- 5. masks --------------------------------------------------------------------------------------------------------------------------
GROUND, BUNNY = 0, 1


@gpu
def test_masks(srt, oracle):
    c = ar.case(oracle, "ground_bunny")
    flat, rays = c.flat, c.rays
    table = vr.case_table(flat)                              # object k carries bit k
    no_ground, only_bunny = ALL_ONES & ~int(table[GROUND]), int(table[BUNNY])
    plain = c.reference(t_max=60.0)
    on_bunny = np.zeros(rays.shape[0], bool); on_bunny[c.sel] = c.obj == BUNNY
    on_ground = np.zeros(rays.shape[0], bool); on_ground[c.sel] = c.obj == GROUND
    assert on_bunny.sum() >= 50 and on_ground.sum() >= 50
    ds = srt.DeviceScene(flat)
    check(ds.ao_rays(rays, DIRS, t_max=60.0), plain, "before any table")
    ds.set_object_masks(table)
    # shadow without the ground's bit: the yardstick's filter
    want = c.reference(t_max=60.0, shadow=no_ground, obj_mask=table)
    assert np.any(want["occ_bits"] != plain["occ_bits"]) and want["n_occluded"].any()
    check(ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(ALL_ONES, 0, no_ground)), want, "the ground casts no AO")
    # the bunny's bit only, and the hit's own object skipped: nothing is left to block a hit on the bunny
    o = ds.ao_rays(rays, DIRS, t_max=60.0, skip_self=True, visibility=(ALL_ONES, 0, only_bunny))
    check(o, c.reference(t_max=60.0, skip_self=True, shadow=only_bunny, obj_mask=table), "the bunny's bit only, skip_self")
    assert (o["n_occluded"][on_bunny] == 0).all() and o["n_occluded"][on_ground].any()
    # primary hides the bunny: its rays go on to the ground or miss; the yardstick on a sample of them
    hidden = ALL_ONES & ~int(table[BUNNY])
    o = ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(hidden, 0, ALL_ONES))
    tr = ds.trace_rays(rays, want=("hit_id", "t"), ray_mask=np.full(rays.shape[0], hidden, np.uint32))
    assert np.array_equal(o["hit_id"], tr["hit_id"]) and np.array_equal(bits(o["t"]), bits(tr["t"]))
    moved = np.flatnonzero(on_bunny & (o["hit_id"] >= 0))
    assert moved.size >= 20 and (flat.tri_obj[o["hit_id"][o["hit_id"] >= 0]] == GROUND).all()
    idx = np.concatenate([moved[:40], np.flatnonzero(on_bunny & (o["hit_id"] < 0))[:8], np.flatnonzero(on_ground)[:16]])
    small = ar.Case(oracle, flat, rays[idx], DIRS, primary=hidden, obj_mask=table).reference(t_max=60.0)
    assert small["n_occluded"][:moved[:40].size].any(), "the bunny still blocks the ground under it"
    ar.assert_same(rows(o, idx), small, "primary hides the bunny", ALL)
    # a table entry of 0 equals the masks that hide the object from both walks (nothing lies behind the ground: its rays become misses)
    want = miss_rows(c.reference(t_max=60.0, shadow=no_ground, obj_mask=table), on_ground)
    check(ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(no_ground, 0, no_ground)), want, "the ground hidden by masks")
    off = table.copy(); off[GROUND] = 0
    ds.set_object_masks(off)
    check(ds.ao_rays(rays, DIRS, t_max=60.0), want, "the ground's table entry 0, vis NULL")
    check(ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(ALL_ONES, ALL_ONES, ALL_ONES)), want, "the ground's table entry 0, vis all ones")
    # all ones equals NULL, and after set_object_masks(None) the plain bits return
    ds.set_object_masks(np.full(flat.n_objects, ALL_ONES, np.uint32))
    check(ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(ALL_ONES, ALL_ONES, ALL_ONES)), plain, "all ones")
    ds.set_object_masks(off)
    ds.set_object_masks(None)
    check(ds.ao_rays(rays, DIRS, t_max=60.0), plain, "after set_object_masks(None)")
    check(ds.ao_rays(rays, DIRS, t_max=60.0, visibility=(ALL_ONES, 0, ALL_ONES)), plain, "after set_object_masks(None), vis")
    ds.close()


# ---- 6. one tree-shape family and one adversarial scene --------------------------------------------------------------------------------
@gpu
def test_tree_shape_family(srt, oracle):
    """roots33: more roots than a 32-bit root mask holds, leaves that are roots, empty objects."""
    flat = ts.family("roots33")
    rays = np.ascontiguousarray(ts.ray_batch("roots33"))
    assert rays.shape[0] % 64 != 0
    dirs = ar.directions(7, cosine=False)
    ds = srt.DeviceScene(flat)
    for skip in (False, True):
        c = ar.Case(oracle, flat, rays, dirs)
        want = c.reference(t_max=INF, skip_self=skip)
        assert c.sel.size * 4 >= rays.shape[0] and 0 < want["n_occluded"].sum() < c.sel.size * 7
        check(ds.ao_rays(rays, dirs, skip_self=skip, count=True), want, f"roots33, skip_self {skip}", n_dirs=7)
    ds.close()


@gpu
def test_coplanar_duplicates(srt, oracle):
    """adversarial.scene(1): the same triangles in several objects (equal t across objects), flat boxes, a sliver."""
    flat = adv.scene(1)[0]
    rays, _ = adv.rays(1)
    rays = np.ascontiguousarray(rays[adv.finite(rays)])
    rays = rays[:rays.shape[0] - (rays.shape[0] % 64 == 0)]
    assert rays.shape[0] % 64 != 0
    groups, is_dup, _ = adv.duplicates(1)
    dirs = ar.directions(9)
    c = ar.Case(oracle, flat, rays, dirs)
    assert is_dup[c.hit[c.sel]].sum() >= 10, "hits on duplicated triangles"
    ds = srt.DeviceScene(flat)
    for skip in (False, True):
        want = c.reference(t_max=INF, skip_self=skip)
        assert 0 < want["n_occluded"].sum()
        check(ds.ao_rays(rays, dirs, skip_self=skip), want, f"duplicates, skip_self {skip}", n_dirs=9)
    # (under skip_self a copy of the hit triangle in ANOTHER object still blocks: the two answers differ)
    assert np.any(c.reference(t_max=INF, skip_self=True)["occ_bits"] != c.reference(t_max=INF)["occ_bits"])
    ds.close()


# ---- 7. counters -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_counters(srt, oracle):
    c = ar.case(oracle, "cubes4_a40")
    flat, rays = c.flat, c.rays
    n = rays.shape[0]
    ds = srt.DeviceScene(flat)
    kw = dict(t_max=60.0, count=True)
    a, b = ds.ao_rays(rays, DIRS, **kw), ds.ao_rays(rays, DIRS, **kw)
    sa = a["stats"]
    assert all(sa[k] > 0 and sa[k] == b["stats"][k] for k in SHADOW_KEYS + PRIMARY_KEYS), (sa, b["stats"])
    hits = int((a["hit_id"] >= 0).sum())
    assert sa["primary_rays"] == n and sa["hit_rays"] == hits and sa["shadow_rays"] == hits * K
    # the primary counters are the masked closest-hit call's
    tr = ds.trace_rays(rays, want=("hit_id",), ray_mask=True, count=True)["stats"]
    assert all(sa[k] == tr[k] for k in PRIMARY_KEYS), (sa, tr)
    # ao_hits on the same hits: the same AO walks, no primary walk
    h = ds.ao_hits(rays, a["hit_id"], a["t"], DIRS, **kw)["stats"]
    assert all(h[k] == sa[k] for k in SHADOW_KEYS) and all(h[k] == 0 for k in PRIMARY_KEYS) and h["hit_rays"] == hits and h["shadow_rays"] == hits * K
    # additive over a split of the batch, unchanged by a permutation
    cut = 501
    parts = [ds.ao_rays(rays[:cut], DIRS, **kw)["stats"], ds.ao_rays(rays[cut:], DIRS, **kw)["stats"]]
    perm = np.random.default_rng(8).permutation(n)
    p = ds.ao_rays(np.ascontiguousarray(rays[perm]), DIRS, **kw)["stats"]
    for k in SHADOW_KEYS + PRIMARY_KEYS + ("hit_rays", "shadow_rays", "primary_rays"):
        assert parts[0][k] + parts[1][k] == sa[k] and p[k] == sa[k], (k, parts, p, sa)
    # a skipped or hidden tree is not entered: fewer tests, and without COUNT none are reported
    skipped = ds.ao_rays(rays, DIRS, skip_self=True, **kw)["stats"]
    assert skipped["node_tests_shadow"] < sa["node_tests_shadow"]
    quiet = ds.ao_rays(rays, DIRS, t_max=60.0)["stats"]
    assert all(quiet[k] == 0 for k in SHADOW_KEYS + PRIMARY_KEYS) and quiet["hit_rays"] == hits and quiet["shadow_rays"] == hits * K
    ds.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_errors(srt, oracle):
    c = ar.case(oracle, "cube_ground")
    flat, rays = c.flat, c.rays
    assert flat.tri_normals is None
    ds = srt.DeviceScene(flat)
    L = ds.L
    n = 8
    f32p, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    r = np.ascontiguousarray(rays[:n]); hit = np.full(n, -9, np.int32); t = np.full(n, -9.0, np.float32)
    cnt = np.full(n, 77, np.uint32); val = np.full(n, -9.0, np.float32); words = np.full((n, 1), 77, np.uint32)
    out = abi.AoOut(cnt.ctypes.data, val.ctypes.data, words.ctypes.data)
    dirs = np.ascontiguousarray(DIRS)
    desc = lambda k=K, d=dirs.ctypes.data, flags=0: abi.AoDesc(k, d, 1e-3, 60.0, flags)
    rp, hp, tp = r.ctypes.data_as(f32p), hit.ctypes.data_as(i32p), t.ctypes.data_as(f32p)

    def all_four(flags, d, want, n_=n, rays_=True):
        a = rp if rays_ else None
        assert L.srt_ao_rays(ds.h, n_, a, None, flags, d, None, hp, tp, C.byref(out), None) == want
        assert L.srt_ao_rays_device(ds.h, n_, r.ctypes.data if rays_ else 0, 0, flags, d, None, 0, 0, 0, C.byref(out)) == want      # (refused before any pointer is used)
        assert L.srt_ao_hits(ds.h, n_, a, hp, tp, flags, d, None, C.byref(out), None) == want
        assert L.srt_ao_hits_device(ds.h, n_, r.ctypes.data if rays_ else 0, hit.ctypes.data, t.ctypes.data, flags, d, None, 0, C.byref(out)) == want

    for flags in (abi.SRT_FLAG_NO_TIMING, abi.SRT_FLAG_FRAMES_IN_FLIGHT, 1 << 8, 1 << 31, abi.SRT_FLAG_SMOOTH_NORMALS):      # (no normals in this scene)
        all_four(flags, C.byref(desc()), abi.SRT_ERR_ARG)
    all_four(0, None, abi.SRT_ERR_ARG)                                       # a NULL ao
    all_four(0, C.byref(desc(d=None)), abi.SRT_ERR_ARG)                      # a NULL table
    all_four(0, C.byref(desc(k=0)), abi.SRT_ERR_ARG)                         # no direction
    all_four(0, C.byref(desc(flags=2)), abi.SRT_ERR_ARG)                     # a flag bit that is not SRT_AO_SKIP_SELF
    all_four(0, C.byref(desc(flags=abi.SRT_AO_SKIP_SELF | (1 << 31))), abi.SRT_ERR_ARG)
    all_four(0, C.byref(desc()), abi.SRT_ERR_ARG, rays_=False)               # NULL rays with n > 0
    all_four(0, C.byref(desc(k=abi.SRT_AO_DIRS_MAX + 1)), abi.SRT_ERR_LIMIT)
    all_four(0, C.byref(desc(k=1024)), abi.SRT_ERR_LIMIT, n_=1 << 22)        # n * n_dirs == 2^32
    d = desc()
    for a in ((None, tp), (hp, None)):
        assert L.srt_ao_hits(ds.h, n, rp, a[0], a[1], 0, C.byref(d), None, C.byref(out), None) == abi.SRT_ERR_ARG
        assert L.srt_ao_hits_device(ds.h, n, r.ctypes.data, 0 if a[0] is None else hit.ctypes.data, 0 if a[1] is None else t.ctypes.data, 0, C.byref(d), None, 0,
                                    C.byref(out)) == abi.SRT_ERR_ARG
    assert L.srt_ao_rays(None, n, rp, None, 0, C.byref(d), None, hp, tp, C.byref(out), None) == abi.SRT_ERR_ARG
    assert (hit == -9).all() and (bits(t) == bits(np.float32(-9.0))).all() and (cnt == 77).all() and (bits(val) == bits(np.float32(-9.0))).all() and (words == 77).all(), \
        "an error touched an output"
    # n == 0
    assert L.srt_ao_rays(ds.h, 0, None, None, 0, C.byref(d), None, None, None, C.byref(out), None) == abi.SRT_OK
    assert L.srt_ao_hits(ds.h, 0, None, None, None, 0, C.byref(d), None, C.byref(out), None) == abi.SRT_OK
    # out NULL or empty: srt_ao_hits does nothing, srt_ao_rays is srt_trace_rays_masked without bary
    st = abi.Stats()
    for o_ in (None, C.byref(abi.AoOut())):
        assert L.srt_ao_hits(ds.h, n, rp, hp, tp, 0, C.byref(d), None, o_, None) == abi.SRT_OK and (cnt == 77).all()
        assert L.srt_ao_rays(ds.h, n, rp, None, abi.SRT_FLAG_COUNT_WORK, C.byref(d), None, hp, tp, o_, C.byref(st)) == abi.SRT_OK
        tr = ds.trace_rays(r, want=("hit_id", "t"), ray_mask=True, count=True)
        assert np.array_equal(hit, tr["hit_id"]) and np.array_equal(bits(t), bits(tr["t"])) and (cnt == 77).all()
        assert all(getattr(st, k) == tr["stats"][k] for k in PRIMARY_KEYS + ("hit_rays", "primary_rays")) and st.node_tests_shadow == 0 and st.shadow_rays == 0
        hit[:] = -9; t[:] = -9.0
    hidden = abi.visibility((2, 0, ALL_ONES))      # (a primary mask with out NULL: no object carries a table, so every object is seen)
    assert L.srt_ao_rays(ds.h, n, rp, None, 0, C.byref(d), C.byref(hidden), hp, tp, None, None) == abi.SRT_OK and np.array_equal(hit, tr["hit_id"])
    with pytest.raises(srt.SrtError):
        ds.ao_rays(rays[:n], DIRS, smooth=True)
    # the handle still answers
    check(ds.ao_rays(rays, DIRS, t_max=60.0), c.reference(t_max=60.0), "after the errors")
    ds.close()


# ---- 9. the device forms and hipGraph capture, in a process of their own ---------------------------------------------------------------
@gpu
def test_device_case_batch_against_the_yardstick(srt, oracle):
    """The batch tests/ao_device_case.py compares the _device forms with: the host form on it, against the yardstick."""
    import ao_device_case as case
    flat, rays = case.batch()
    want = ar.Case(oracle, flat, rays, case.DIRS).reference(t_max=case.T_MAX, skip_self=True)
    assert 0 < (want["n_occluded"] > 0).sum() < (want["hit_id"] >= 0).sum()
    ds = srt.DeviceScene(flat)
    check(ds.ao_rays(rays, case.DIRS, t_max=case.T_MAX, skip_self=True), want, "device-case batch", n_dirs=case.DIRS.shape[0])
    ds.close()


@gpu
def test_device_forms_and_graph_capture():
    r = subprocess.run([sys.executable, os.path.join(HERE, "ao_device_case.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ao device case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
