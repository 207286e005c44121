"""Run by tests/test_gpu_ray_range.py in its own process (torch initialises HIP first): the device entry points of the ray queries with
a t interval on torch tensors.  `device`: a second stream, results equal to the host forms', the identities, a t_range pointer that is
only float-aligned, a shared handle.  `graph`: one range call of each kind captured into a hipGraph and replayed once."""
import sys
import numpy as np

from query_device_common import INF, QUERY_FILL, UNBOUNDED, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import ray_query_ref as rq

N = 257
TRACE = ("hit_id", "t", "bary")


def setup():
    """cubes4_a40, N unrelated rays, one interval per ray around the ray's own first hit (kinds dealt round robin), and what the host
    forms -- pinned against the yardstick by the tests that call this -- give for them (the occlusion bytes under `occluded`)."""
    c = open_case("cubes4_a40")
    g = c.g
    ds = lib.DeviceScene(g.flat)
    rays = rq.unrelated_rays(g.flat, N, seed=5)
    plain = ds.trace_rays(rays)
    t1 = np.where(plain["hit_id"] >= 0, plain["t"], np.float32(50.0)).astype(np.float32)
    kind = np.arange(N) % 4
    tr = np.empty((N, 2), np.float32)
    tr[:, 0] = np.select([kind == 0, kind == 1, kind == 2], [np.nextafter(t1, INF), 0.0, t1], t1 * np.float32(0.5))
    tr[:, 1] = np.select([kind == 0, kind == 1, kind == 2], [INF, np.nextafter(t1, -INF), t1], t1 * np.float32(1.5))
    skip = np.random.default_rng(1).integers(-1, g.flat.n_objects, N).astype(np.int32)
    host = ds.trace_rays(rays, t_range=tr)
    occ = ds.occluded(rays, skip, t_range=tr)
    assert not np.array_equal(host["hit_id"], plain["hit_id"]) and (host["hit_id"] >= 0).sum() > N // 4
    assert not np.array_equal(occ, ds.occluded(rays, skip)) and 0 < occ.sum() < N
    out = Outputs(c.dev, {"hit_id": ((N,), np.int32), "t": ((N,), np.float32), "bary": ((N, 3), np.float32), "occluded": ((N,), np.uint8)}, QUERY_FILL)
    d_rays, d_tr, d_skip = c.put(rays, tr, skip)

    def both(h, tr_ptr, stream, count=False):
        h.trace_rays_device(N, d_rays.data_ptr(), stream=stream, count=count, t_range=tr_ptr, **out.ptrs(keys=TRACE))
        h.occluded_device(N, d_rays.data_ptr(), out.t["occluded"].data_ptr(), skip_obj=d_skip.data_ptr(), stream=stream, t_range=tr_ptr)
    return c, ds, rays, skip, d_tr, plain, dict(host, occluded=occ), out, both


def device_case():
    c, ds, rays, skip, d_tr, plain, host, out, both = setup()
    dev, side = c.dev, c.side
    assert d_tr.data_ptr() % 8 == 0
    for count in (False, True):
        both(ds, d_tr.data_ptr(), side.cuda_stream, count)
        side.synchronize()
        out.same(host, f"second stream, counting {count}")
    both(ds, d_tr.data_ptr(), 0)                               # NULL stream = the scene's own stream
    ds.occluded(rays, skip)                                    # (a host call on the same stream waits for it)
    out.same(host, "own stream")
    odd = float_aligned(dev, d_tr)                             # the same intervals 4 bytes further: the narrow loads
    both(ds, odd.data_ptr(), side.cuda_stream)
    side.synchronize()
    out.same(host, "float-aligned t_range")
    # the identities, device forms: a NULL t_range and the three intervals that bound nothing give the unbounded calls' bits
    plain = dict(plain, occluded=ds.occluded(rays, skip))
    for pair in UNBOUNDED:
        d_id = None if pair is None else c.put(np.tile(np.array(pair, np.float32), (N, 1)))[0]
        both(ds, None if d_id is None else d_id.data_ptr(), side.cuda_stream)
        side.synchronize()
        out.same(plain, f"identity {pair}")

    def shared(sh):
        both(sh, d_tr.data_ptr(), side.cuda_stream)
        side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)
    print("ray range device case: ok")


def graph_case():
    c, ds, rays, skip, d_tr, plain, host, out, both = setup()
    captured(lambda stream: both(ds, d_tr.data_ptr(), stream), out, host, "replay", [(out, ("hit_id", "occluded"))], replays=1)
    print("ray range graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
