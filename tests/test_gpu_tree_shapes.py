"""GPU (-m gpu): every device walk on trees the layout contract admits and the host mirror's builder never makes -- the families of
tests/tree_shapes.py: leaves of up to 31 triangles (the sliced push of the query walk, the any-hit walks), combs of height 255 and 256
(the pose refit's top part, its limit), objects whose root is a leaf at the counts where the tile kernels' root mask and root groups
change (5, 17, 32, 33, 300), node arrays in any order, boxes that stick out of their parents or cut through their triangles, ties.
tests/test_tree_shapes_ref.py shows on the CPU that each family reaches the path it is for.

Everything is compared with the oracle on the same flat scene at the bars the suite already has: hit ids and t bit for bit, colours
through gpu_frames.compare_exact against the oracle run with the device's pow, work counts equal."""
import numpy as np
import pytest

import gpu_frames as gf
import pose_ref
import ray_range_ref as rr
import shade_query_ref as sq
import tree_shapes as ts
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
VARIANTS = (0, 3, 6, 10, 21, 22, 23, 41)
WORK = ("node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def check_frame(srt, oracle, ds, flat, p, what, count=False):
    """A render of `p` on `ds` against the oracle on `flat`."""
    o = ds.render(p)
    c = oracle.render(flat, p, pow="device")
    gf.compare_exact(srt, o, c, gf.owned(p), flat, p, what)
    if count:
        for k in WORK:
            assert o["stats"][k] == c["stats"][k], (what, k, o["stats"][k], c["stats"][k])
        assert c["stats"]["node_tests_primary"] > 0
    return o, c


def check_closest(o, hit, t, what):
    bad = o["hit_id"] != hit
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} hit ids differ, first at ray {int(np.flatnonzero(bad)[0])}"
    assert np.array_equal(bits(o["t"]), bits(t)), f"{what}: t differs"


# ---- renders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.FAMILIES)
def test_renders(srt, oracle, name):
    """Variants 0, 0 counting, 3, 6, 10, 21, 22, 23 and 41 at 1 and 9 light samples, and the shipped pipeline in camera mode."""
    flat = ts.family(name)
    ds = srt.DeviceScene(flat)
    pipes = set()
    for L in (1, 9):
        for v in VARIANTS:
            o, c = check_frame(srt, oracle, ds, flat, ts.frame_params(L, flags=v << 8), f"{name} L {L} variant {v}")
            pipes.add(ds.pipeline)
        check_frame(srt, oracle, ds, flat, ts.frame_params(L, flags=abi.SRT_FLAG_COUNT_WORK), f"{name} L {L} counting", count=True)
        check_frame(srt, oracle, ds, flat, ts.frame_params(L, camera=True), f"{name} L {L} camera")
        pipes.add(ds.pipeline)
        assert 0.1 <= (c["hit_id"] >= 0).mean() <= 0.9
    print(name, "overlap estimate", round(ds.overlap_estimate, 1), "pipelines", sorted(pipes))
    if name == "sliced":
        check_frame(srt, oracle, ds, flat, ts.frame_params(9, flags=abi.SRT_FLAG_SMOOTH_NORMALS), "sliced smooth")
    ds.close()


@pytest.mark.parametrize("name", ts.FAMILIES)
def test_batch_over_shared_handles(srt, oracle, name):
    """srt_render_device_batch over three handles of srt_scene_share, each frame with its own light, at 1 and at 16 samples: bitwise the
    single renders (which are the oracle's), padding and guard rows untouched."""
    flat = ts.family(name)
    L_ = srt.load()
    first = srt.DeviceScene(flat)
    handles = [first.share() for _ in range(3)]
    solo = first.share()
    first.close()
    try:
        for n_lights in (1, 16):
            ps = [ts.frame_params(n_lights, light=(ts.LIGHT[0] + 40.0 * k, ts.LIGHT[1], ts.LIGHT[2] - 30.0 * k)) for k in range(3)]
            bufs = [gf.PinnedFrame(L_, h.rows(p), h.cols(p)) for h, p in zip(handles, ps)]
            try:
                srt.FrameBatch(handles, ps, *[[b.ptrs[k] for b in bufs] for k in range(4)]).render()
                stats = [h.sync() for h in handles]
                for k, (h, p, b, st) in enumerate(zip(handles, ps, bufs, stats)):
                    what = f"{name} L {n_lights} frame {k}"
                    b.check_untouched(gf.owned(p), what)
                    got = b.out()
                    want, _ = check_frame(srt, oracle, solo, flat, p, what + " alone")
                    assert np.array_equal(got["hit_id"], want["hit_id"]) and np.array_equal(bits(got["t"]), bits(want["t"])), what
                    assert np.array_equal(bits(got["rgb_linear"]), bits(want["rgb_linear"])) and np.array_equal(got["rgb8"], want["rgb8"]), what
                    for key in ("primary_rays", "hit_rays", "shadow_rays", "rows"):
                        assert st[key] == want["stats"][key], (what, key)
                    if solo.overlap_estimate <= 150.0:
                        assert "(batched)" in h.pipeline, (what, h.pipeline)
            finally:
                for b in bufs:
                    b.free()
    finally:
        for h in handles + [solo]:
            h.close()


# ---- queries ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ts.FAMILIES)
def test_queries(srt, oracle, name):
    """srt_trace_rays with bary, plain and counting (node and triangle tests the oracle's: a sliced leaf counts its node once);
    srt_occluded with skipped objects, -1 and n_objects among them; both _range forms on a mixed interval batch."""
    r = ts.reference(oracle, name)
    flat, rays = r["flat"], r["rays"]
    n = rays.shape[0]
    c = rr.candidates(oracle, flat, rays)
    bary = rr.want_bary(oracle, flat, rays, r["ray_hit"], r["ray_t"])
    ds = srt.DeviceScene(flat)
    for count in (False, True):
        o = ds.trace_rays(rays, count=count)
        check_closest(o, r["ray_hit"], r["ray_t"], f"{name} count {count}")
        assert np.array_equal(bits(o["bary"]), bits(bary)), name
        st = o["stats"]
        assert st["primary_rays"] == n and st["hit_rays"] == int((r["ray_hit"] >= 0).sum())
        want = (r["ray_node_tests"], r["ray_tri_tests"]) if count else (0, 0)
        assert (st["node_tests_primary"], st["tri_tests_primary"]) == want, (name, count, st, want)
    skip = np.random.default_rng(8).integers(-1, flat.n_objects + 1, n).astype(np.int32)
    skip[:4] = (-1, flat.n_objects, 0, flat.n_objects - 1)
    assert np.array_equal(ds.occluded(rays, skip), rr.occluded(c, flat, None, skip)), name
    assert np.array_equal(ds.occluded(rays), rr.occluded(c, flat)), name
    assert 0 < rr.occluded(c, flat, None, skip).sum() <= rr.occluded(c, flat).sum() < n
    tr, kind, hit0 = rr.mixed_intervals(c, 17)
    want_hit, want_t = rr.closest(c, tr)
    second = (kind == 0) & (hit0 >= 0)
    assert (want_hit[second] >= 0).sum() >= 5 and (want_hit[second] != hit0[second]).all()
    for count in (False, True):
        o = ds.trace_rays(rays, count=count, t_range=tr)
        check_closest(o, want_hit, want_t, f"{name} range count {count}")
        assert np.array_equal(bits(o["bary"]), bits(rr.want_bary(oracle, flat, rays, want_hit, want_t))), name
        want = (r["ray_node_tests"], r["ray_tri_tests"]) if count else (0, 0)
        assert (o["stats"]["node_tests_primary"], o["stats"]["tri_tests_primary"]) == want, (name, count)
    assert np.array_equal(ds.occluded(rays, skip, t_range=tr), rr.occluded(c, flat, tr, skip)), name
    assert np.array_equal(ds.occluded(rays, t_range=tr), rr.occluded(c, flat, tr)), name
    ds.close()


@pytest.mark.parametrize("name", ts.FAMILIES)
def test_shade_rays(srt, oracle, name):
    """srt_shade_rays at 1, 9 and 65 light samples, flat and (where the family has normals) smooth: every ray its own 1 x 1 oracle frame
    with the device's pow, compared as one row of pixels; the shadow phase walks the big leaves."""
    r = ts.reference(oracle, name)
    flat, rays = r["flat"], r["rays"]
    n = rays.shape[0]
    own = np.arange(n, dtype=np.int64).reshape(1, n)
    ds = srt.DeviceScene(flat)
    for n_lights in (1, 9, 65):
        lights = abi.light_staircase(np.asarray(ts.LIGHT, np.float32), n_lights)
        for flags in ((0, abi.SRT_FLAG_SMOOTH_NORMALS) if flat.tri_normals is not None else (0,)):
            what = f"{name} L {n_lights} flags {flags}"
            hit, t, lin, rgb8 = sq.oracle_shade(oracle, flat, rays, lights, flags=flags)
            assert np.array_equal(hit, r["ray_hit"])
            if n_lights == 1 and flags == 0:
                in_shadow, lit = sq.shadow_share(oracle, flat, rays[hit >= 0], lights[0])
                print(what, "hits in shadow", int(in_shadow.sum()), "lit", int(lit.sum()))
                assert lit.sum() >= 5 and (in_shadow.sum() >= 5 or name.startswith("comb")), "(a comb is one sheet: little shades it)"
            p = sq.shade_params(lights, flags=flags)
            o = ds.shade_rays(rays, p)
            n_hit = int((hit >= 0).sum())
            c = dict(hit_id=hit.reshape(1, n), t=t.reshape(1, n), rgb_linear=lin.reshape(1, n, 3), rgb8=rgb8.reshape(1, n, 3),
                     stats=dict(primary_rays=n, hit_rays=n_hit, shadow_rays=n_hit * n_lights))
            got = {k: (v if k == "stats" else v.reshape((1,) + v.shape)) for k, v in o.items()}
            gf.compare_exact(srt, got, c, own, flat, p, what)
    ds.close()


# ---- pose ------------------------------------------------------------------------------------------------------------------------
def turn(centre, axis, deg):
    """A rigid turn about a point: translate(centre) * rotate * translate(-centre), column-major."""
    a = np.radians(deg)
    u = np.asarray(axis, np.float64); u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = np.asarray(centre, np.float64) - R @ np.asarray(centre, np.float64)
    return np.ascontiguousarray(M.T.reshape(16), np.float32)


def poses(flat):
    """Identity; a rigid turn per object about its own centre (an empty object: about the origin); one sheared matrix for all."""
    nO = flat.n_objects
    ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (nO, 1))
    rigid = ident.copy()
    for k in range(nO):
        P = flat.tri_points[flat.tri_obj == k][..., :3].reshape(-1, 3)
        rigid[k] = turn(P.mean(0) if len(P) else (0.0, 0.0, 0.0), (0.3 + 0.1 * (k % 5), 1.0, 0.2 * (k % 3)), 20.0 + 7.0 * (k % 11))
    shear = np.array([1.0, 0.1, 0.0, 0.0,   0.25, 0.9, 0.05, 0.0,   -0.1, 0.0, 1.1, 0.0,   3.0, -4.0, 10.0, 1.0], np.float32)
    return (("identity", ident), ("rigid", rigid), ("shear", np.tile(shear, (nO, 1))))


def same_bytes(got, want, what):
    for k in ("nodes", "wide", "root_nodes", "tris", "tris_o"):
        a, b = got[k].view(np.uint8), want[k].view(np.uint8)
        assert a.shape == b.shape and np.array_equal(a, b), f"{what}: {k}: {int((got[k] != want[k]).any(1).sum())} of {got[k].shape[0]} records differ"


@pytest.mark.parametrize("name", ts.POSED)
def test_pose(srt, oracle, name):
    """One pose source, three poses.  After each the node, wide and root records are, byte for byte, those of a scene created from
    pose_ref's posed flat scene, and a render and a closest-hit query are the oracle's on that flat scene."""
    flat = ts.family(name)
    rays = ts.ray_batch(name)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    seen = []
    for what, mats in poses(flat):
        what = f"{name} {what}"
        ds.pose(mats)
        want = pose_ref.pose_flat(flat, mats)
        fresh = srt.DeviceScene(want)
        same_bytes(ds.records(), fresh.records(), what)
        fresh.close()
        o, c = check_frame(srt, oracle, ds, want, ts.frame_params(2, flags=abi.SRT_FLAG_COUNT_WORK), what, count=True)
        check_frame(srt, oracle, ds, want, ts.frame_params(9), what)
        seen.append(c["hit_id"])
        hit, t, n_node, n_tri = ts.oracle_rays(oracle, want, rays)
        q = ds.trace_rays(rays, count=True)
        check_closest(q, hit, t, what)
        assert (q["stats"]["node_tests_primary"], q["stats"]["tri_tests_primary"]) == (n_node, n_tri), what
        assert (c["hit_id"] >= 0).sum() >= 100, what
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2]), "the poses move what the frame sees"
    ds.close()


def test_comb256_is_beyond_the_pose_limit(srt, oracle):
    """A tree of height 256 creates, renders and answers queries like any other; srt_scene_set_pose_source refuses it with SRT_ERR_LIMIT,
    a pose without a source is SRT_ERR_ARG, and the scene renders the same frame afterwards."""
    flat = ts.family("comb256")
    ds = srt.DeviceScene(flat)
    p = ts.frame_params(2)
    before, _ = check_frame(srt, oracle, ds, flat, p, "comb256")
    with pytest.raises(srt.SrtError) as e:
        ds.set_pose_source()
    assert e.value.code == abi.SRT_ERR_LIMIT
    with pytest.raises(srt.SrtError) as e:
        ds.pose(np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1)))
    assert e.value.code == abi.SRT_ERR_ARG
    after, _ = check_frame(srt, oracle, ds, flat, p, "comb256 after the refused calls")
    for k in ("hit_id", "rgb8"):
        assert np.array_equal(before[k], after[k])
    assert np.array_equal(bits(before["rgb_linear"]), bits(after["rgb_linear"]))
    fresh = srt.DeviceScene(flat)
    same_bytes(ds.records(), fresh.records(), "comb256 after the refused calls")
    fresh.close(); ds.close()


# ---- srt_scene_update between shapes ---------------------------------------------------------------------------------------------
def test_update_between_shapes(srt, oracle):
    """srt_scene_update with the same counts and another node order (shuffled), then other boxes (shrunk), then another tree (sliced's
    triangles hung into combs): records and frames follow the new scene."""
    sliced = ts.family("sliced")
    objs = ts.sliced_objects()
    combs = ts.flat_scene([dict(o, shape=("left_comb", "zigzag", "right_comb")[k]) for k, o in enumerate(objs)])
    assert combs.n_nodes == sliced.n_nodes and not np.array_equal(combs.tri_points, sliced.tri_points), "same counts, another visit order"
    ds = srt.DeviceScene(sliced)
    p = ts.frame_params(2)
    check_frame(srt, oracle, ds, sliced, p, "sliced")
    for name, flat in (("shuffled", ts.family("shuffled")), ("shrunk", ts.family("shrunk")), ("combs", combs), ("sliced", sliced)):
        ds.update(flat); ds.sync()
        fresh = srt.DeviceScene(flat)
        same_bytes(ds.records(), fresh.records(), "update to " + name)
        fresh.close()
        check_frame(srt, oracle, ds, flat, p, "update to " + name)
        r = ts.reference(oracle, name) if name != "combs" else None
        if r is not None:
            check_closest(ds.trace_rays(r["rays"]), r["ray_hit"], r["ray_t"], "update to " + name)
    ds.close()
