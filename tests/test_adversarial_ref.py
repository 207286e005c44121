"""CPU: the ray batches of tests/adversarial.py reach the cases they are aimed at, on the yardsticks alone -- before
tests/test_gpu_adversarial_queries.py puts them to the device.  Every count is printed, then asserted."""
import numpy as np
import pytest

import adversarial as adv
import ray_range_ref as rr
import refract_ref as rf
import surface_ref as sf
import tree_shapes as ts
import visibility_ref as vr

bits = sf.bits
NONE = np.zeros((0, 3), np.float32)


def test_the_batches_are_what_they_say():
    for seed in adv.SEEDS:
        r, cls = adv.rays(seed)
        flat = adv.scene(seed)[0]
        assert r.shape[0] <= 600 and r.shape[0] % 64 and set(cls.tolist()) == set(range(8)) and (np.diff(cls) >= 0).all()
        assert not (np.signbit(r[:, 3:6]) & (r[:, 3:6] == 0)).any(), "a -0 direction component"
        assert (cls == adv.NONFINITE).sum() == 8 and np.array_equal(~adv.finite(r), cls == adv.NONFINITE)
        a = r[cls == adv.A]
        assert (a[:, 0:3] == 0).all() and (a[:, 3] == 0).any() and (a[:, 4] == 0).any() and (a[:, 5] == adv.FOCAL).all()
        c = r[cls == adv.C]
        assert ((c[:, 3] == 0) & (c[:, 4] == 0)).sum() * 2 == c.shape[0]                  # half of them axis-aligned
        assert not r.flags.writeable and flat.n_objects == 6 == adv.REFLECTANCE.size
        assert bool(np.any(flat.tri_normals)) == (seed == 4)                               # the host builder leaves zero normals
        assert adv.lower_copy_objects(seed) == ([1], [1, 2])                                   # objects are listed in reverse: obj4, obj3


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_walks_reach_the_cases(oracle, seed):
    flat = adv.scene(seed)[0]
    r, cls = adv.rays(seed)
    c = adv.candidates(oracle, seed)
    hit, t = rr.closest(c)
    count = {}
    ab = cls <= adv.B
    count["hit share of A and B"] = round(float((hit[ab] >= 0).mean()), 4)
    tied, low_obj = adv.nearest_ties(flat, c)
    count["rays whose nearest t is shared by two objects"] = int(tied.sum())
    # hide the object of the lower id: the copy in a later object wins at the same t
    table = vr.hidden(flat)[0]
    ray_mask = np.array([vr.hidden(flat, int(k))[1] if k >= 0 else vr.ALL for k in low_obj], np.uint32)
    h2, t2 = vr.closest(c, flat, ray_mask, table)
    moved = tied & (h2 >= 0) & (h2 != hit) & (bits(t2 + np.float32(0.0)) == bits(t + np.float32(0.0)))
    count["of those, hiding the lower id's object hands the hit to another object at the same t"] = int(moved.sum())
    assert (flat.tri_obj[h2[moved]] != low_obj[moved]).all() and (h2[moved] > hit[moved]).all()
    # class C: both triangles of a quad (one object, both flat in z) at the same t
    flat_z = (adv.points_of(flat)[:, :, 2] == adv.points_of(flat)[:, :1, 2]).all(axis=1)
    with np.errstate(invalid="ignore"):
        fin = (c.t != -np.inf) & (c.t < np.inf) & flat_z[c.tri] & (cls[c.ray] == adv.C)
    key = np.stack([c.ray[fin], flat.tri_obj[c.tri[fin]].astype(np.int64), bits(c.t[fin] + np.float32(0.0)).astype(np.int64)], axis=1)
    _, n_same = np.unique(key, axis=0, return_counts=True)
    count["class C rays (ray, object) pairs with both triangles of a quad at one t"] = int((n_same >= 2).sum())
    count["class E candidates with t == 0"] = int(((c.t == 0) & (cls[c.ray] == adv.E)).sum())
    # class F: the triangles the ray lies in the plane of are reached (their leaf is walked) and the triangle test calls them parallel
    P = adv.points_of(flat)
    oz, dz, oy, dy = r[c.ray, 2], r[c.ray, 5], r[c.ray, 1], r[c.ray, 4]
    in_plane = (cls[c.ray] == adv.F) & (((dz == 0) & (P[c.tri, :, 2] == oz[:, None]).all(axis=1)) | ((dy == 0) & (oy == 0) & (P[c.tri, :, 1] == 0).all(axis=1)))
    count["class F (ray, in-plane triangle) candidates"] = int(in_plane.sum())
    count["of those, -inf"] = int((in_plane & (c.t == -np.inf)).sum())
    n_in = np.bincount(c.ray[in_plane], minlength=r.shape[0])
    n_in_miss = np.bincount(c.ray[in_plane & (c.t == -np.inf)], minlength=r.shape[0])
    count["class F rays all of whose in-plane candidates are -inf"] = int(((n_in > 0) & (n_in == n_in_miss)).sum())
    nan_rays = np.unique(c.ray[np.isnan(c.t)])
    count["rays with a NaN candidate"] = (int(nan_rays.size), sorted(set(cls[nan_rays].tolist())))
    count["class G hits"] = int((hit[cls == adv.G] >= 0).sum())
    # the oracle's own walk of every finite ray agrees with the candidate yardstick
    ok = adv.finite(r)
    oh, ot, _, _ = ts.oracle_rays(oracle, flat, r[ok])
    assert np.array_equal(oh, hit[ok]) and np.array_equal(bits(ot), bits(t[ok]))
    for k, v in count.items():
        print(f"seed {seed}: {k}: {v}")
    assert 0.2 < count["hit share of A and B"] < 0.8
    assert count["rays whose nearest t is shared by two objects"] >= 20
    assert count["of those, hiding the lower id's object hands the hit to another object at the same t"] >= 10
    assert count["class C rays (ray, object) pairs with both triangles of a quad at one t"] >= 1
    assert count["class E candidates with t == 0"] >= 1
    assert count["class F rays all of whose in-plane candidates are -inf"] >= 1
    assert nan_rays.size >= 1 and set(cls[nan_rays].tolist()) <= {adv.F, adv.NONFINITE}
    assert count["class G hits"] >= 1
    # the interval batch: every kind is there, and the closed points sit on tied rays
    tr, kind = adv.intervals(oracle, seed)
    print(f"seed {seed}: interval kinds", np.bincount(kind, minlength=7).tolist(), "closed points on tied rays", int((tied & (kind == 2)).sum()))
    assert (np.bincount(kind, minlength=7) >= 10).all() and (tied & (kind == 2)).sum() >= 10
    # the K-nearest merge: rows of 16 slots in which four or more hold one t from different objects
    import ray_multi_ref as rm
    _, mh, mt = rm.multi(c, 16)
    key = bits(mt + np.float32(0.0))
    four = sum(1 for i in range(mh.shape[0]) if max((np.unique(flat.tri_obj[mh[i][(mh[i] >= 0) & (key[i] == k)]]).size for k in np.unique(key[i][mh[i] >= 0])), default=0) >= 4)
    print(f"seed {seed}: rows of the 16 nearest with one t from four or more objects: {four}")
    assert four >= 1
    h3, _ = rr.closest(c, tr)
    second = (kind == 0) & (hit >= 0)
    assert (h3[second] >= 0).sum() >= 10 and np.array_equal(h3[tied & (kind == 2)], hit[tied & (kind == 2)])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_paths_reach_the_cases(oracle, seed):
    flat = adv.scene(seed)[0]
    r, cls = adv.rays(seed)
    _, is_dup, lowest = adv.duplicates(seed)
    memo = adv.memo(oracle, seed)
    segs, kinds = rf.trace(oracle, flat, r, NONE, adv.DEPTH, np.zeros(flat.n_objects, np.float32), bounce_t_min=adv.BOUNCE_T_MIN, cands=memo)
    assert len(segs) == 3
    on_dup = (segs[0].hit >= 0) & is_dup[np.maximum(segs[0].hit, 0)]
    # the candidates of the segment-1 rays that start on a duplicated triangle: the copies of that triangle among them
    idx = np.flatnonzero(on_dup)
    c = memo(segs[1].rays[idx])
    copy = lowest[c.tri] == lowest[segs[0].hit[idx]][c.ray]
    with np.errstate(invalid="ignore"):
        real = copy & (c.t != -np.inf) & (c.t < np.inf)
        below, inside = real & (c.t < np.float32(adv.BOUNCE_T_MIN)), real & ~(c.t < np.float32(adv.BOUNCE_T_MIN))
    count = {"segment-1 rays that start on a duplicated triangle": int(idx.size),
             "copies of their own triangle met below bounce_t_min (not found again)": int(below.sum()),
             "copies met at or above bounce_t_min (in range)": int(inside.sum()),
             "segment-1 hits": int((segs[1].hit >= 0).sum()), "segment-2 hits": int((segs[2].hit >= 0).sum())}
    for k, v in count.items():
        print(f"seed {seed}: {k}: {v}")
    assert idx.size >= 1 and count["segment-2 hits"] >= 1
    # exactly as bounce_t_min dictates: no winner of segment 1 is a copy met below it, and a copy in range loses only to something nearer
    win_t = segs[1].t[idx][c.ray]
    assert not (below & (c.tri == segs[1].hit[idx][c.ray])).any()
    with np.errstate(invalid="ignore"):
        assert (win_t[inside] <= c.t[inside]).all()
    assert below.sum() + inside.sum() >= 1
    # under glass the two later copies' objects transmit: some ray enters, and some later segment leaves or is totally reflected
    segs_g, kinds_g = rf.trace(oracle, flat, r, NONE, adv.DEPTH, adv.glass_ior(seed), bounce_t_min=adv.BOUNCE_T_MIN, cands=memo)
    kc = rf.kind_counts(kinds_g)
    print(f"seed {seed}: kinds under glass", kc)
    assert kc[0]["enter"] + kc[0]["leave"] >= 10 and kc[0]["mirror"] >= 10
