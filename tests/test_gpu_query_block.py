"""GPU (-m gpu): the host forms of the query calls share ONE device block per handle, cut afresh by every call (srt_hip.hip,
query_round_trip).  One handle on cubes4_a0 goes through five call kinds in turn at 257, 1 and 65 rays -- the block's layout changes with
every call, and what an earlier, longer call left in it lies under the pieces of the next --, first with every output, then with every
second output left out.  Every result is pinned bit for bit by the yardstick of its call (ray_range_ref, ray_multi_ref, surface_ref,
point_ref), computed once at 257 and cut to the first n: a ray's result does not depend on its neighbours."""
import functools

import numpy as np
import pytest

import golden_util as gu
import point_ref as pr
import ray_multi_ref as rm
import ray_query_ref as rq
import ray_range_ref as rr
import surface_ref as sf
import visibility_ref as vr

pytestmark = pytest.mark.gpu
COUNTS = (257, 1, 65)
N, K = max(COUNTS), 3
bits = sf.bits
TRACE = ("hit_id", "t", "bary")
MULTI = ("n_hits", "hit_id", "t", "bary")
SURFACE = ("hit_id", "t", "obj", "point", "normal", "color", "material", "bounce")


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@functools.lru_cache(maxsize=None)
def reference():
    """Computed once and never changed: the scene, N rays and N points with what each call brings, and what the yardsticks say of them."""
    from oracle import pyoracle
    flat = gu.GoldenScene("cubes4_a0").flat
    rays = rq.unrelated_rays(flat, N, seed=11)
    c = rr.candidates(pyoracle, flat, rays)
    tr = rr.mixed_intervals(c, 12)[0]
    i = np.arange(N)
    table = (np.uint32(1) << np.arange(flat.n_objects, dtype=np.uint32)).astype(np.uint32)      # object k has bit k
    masks = np.array([vr.ALL & ~1, vr.ALL, vr.ALL & ~2, 0], np.uint32)[i % 4]
    skip = (i % (flat.n_objects + 1) - 1).astype(np.int32)
    hit, t = rr.closest(vr.visible(c, flat, masks, table), tr)
    trace = dict(hit_id=hit, t=t, bary=rr.want_bary(pyoracle, flat, rays, hit, t))
    n_hits, mhit, mt = rm.multi(c, K)
    multi = dict(n_hits=n_hits, hit_id=mhit, t=mt, bary=rm.multi_bary(pyoracle, flat, rays, mhit, mt))
    P = np.ascontiguousarray(flat.tri_points, np.float32)[..., :3].reshape(-1, 3)
    ext = float(np.linalg.norm(P.max(0) - P.min(0)))
    rng = np.random.default_rng(13)
    pts = np.where((i % 2 == 0)[:, None], P[rng.integers(0, len(P), N)] + rng.normal(0.0, 0.01 * ext, (N, 3)),
                   P.min(0) + (P.max(0) - P.min(0)) * rng.uniform(-0.3, 1.3, (N, 3))).astype(np.float32)
    rad = (ext * 10.0 ** rng.uniform(-2.0, 0.0, N)).astype(np.float32)
    rad[::5] = np.inf
    pmask = np.array([vr.ALL, 1, 2 | 4, 0, 8], np.uint32)[i % 5]
    return dict(flat=flat, rays=rays, tr=tr, table=table, masks=masks, skip=skip, pts=pts, rad=rad, pmask=pmask, trace=trace,
                unmasked=rr.closest(c, tr)[0], unbounded=rr.closest(c)[0], occ=rr.occluded(c, flat, tr, skip), multi=multi, surface=sf.surface_rays(pyoracle, flat, rays),
                points=pr.closest_points(flat, pts, rad, point_mask=pmask, obj_mask=table))


def same(got, want, keys, n, what):
    """`got` holds the arrays `keys` and stats, nothing else; each equals the first n rows of the yardstick's: ints by value, floats by bits."""
    assert set(got) == set(keys) | {"stats"}, (what, sorted(got))
    for k in keys:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k][:n])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if w.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        bad = np.flatnonzero((g != w).reshape(n, -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs in {bad.size} of {n} rows, first at row {int(bad[0])}: got {got[k][bad[0]]}, want {want[k][bad[0]]}"


def test_call_kinds_interleaved_on_one_handle(srt):
    r = reference()
    rays, tr, pts = r["rays"], r["tr"], r["pts"]
    # the batch says something: every call kind has hits and misses, the masks and the intervals change winners, rows of the multi call are short
    assert (r["unmasked"][:65] != r["trace"]["hit_id"][:65]).any() and (r["unbounded"][:65] != r["unmasked"][:65]).any()
    for hit in (r["trace"]["hit_id"], r["surface"]["hit_id"], r["points"]["tri"]):
        assert 0 < (hit[:65] >= 0).sum() < 65 and 0 < (hit >= 0).sum() < N
    assert 0 < r["occ"][:65].sum() < 65 and (r["multi"]["n_hits"] > K).any() and ((r["multi"]["n_hits"] > 0) & (r["multi"]["n_hits"] < K)).any()
    for call in ("trace", "multi", "surface", "points"):      # no NaN in a yardstick: bit for bit below means what it says
        assert not any(np.isnan(a).any() for a in r[call].values() if getattr(a, "dtype", None) == np.float32), call
    ds = srt.DeviceScene(r["flat"])
    ds.set_object_masks(r["table"])
    for every in (1, 2):      # all outputs, then every second one left out
        trace, multi, surface, points = TRACE[::every], MULTI[::every], SURFACE[::every], pr.SAME_KEYS[::every]
        for n in COUNTS:
            what = f"{n} rays, every {every}. output"
            same(ds.trace_rays(rays[:n], want=trace, t_range=tr[:n], ray_mask=r["masks"][:n]), r["trace"], trace, n, what + ", trace_rays")
            occ = ds.occluded(rays[:n], r["skip"][:n], t_range=tr[:n])
            assert occ.dtype == np.uint8 and np.array_equal(occ, r["occ"][:n]), what + ", occluded"
            same(ds.trace_rays_multi(rays[:n], K, want=multi), r["multi"], multi, n, what + ", trace_rays_multi")
            same(ds.surface_rays(rays[:n], want=surface), r["surface"], surface, n, what + ", surface_rays")
            same(ds.closest_points(pts[:n], radius=r["rad"][:n], point_mask=r["pmask"][:n], want=points), r["points"], points, n, what + ", closest_points")
    ds.close()
