"""Run by tests/test_gpu_surface.py in its own process (torch initialises HIP first): srt_surface_rays_device / srt_surface_hits_device on
torch tensors.
`device`: a second stream and the scene's own; results equal to the host entry point's (which tests/test_gpu_surface.py pins against
tests/surface_ref.py on the same batch); each output alone, the others NULL; rays and t_range at an address that is only float-aligned;
a permuted batch; a handle of srt_scene_share; a render beside the queries keeps its pixels, statistics and pipeline string.
`graph`: both _device forms, without SRT_FLAG_COUNT_WORK, captured into a hipGraph and replayed to the same bits."""
import sys
import numpy as np
import torch

from query_device_common import Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import abi, lib
import ray_query_ref as rq
import shade_range_ref as sr

SCENE, N, SEED = "cubes4_a40", 257, 5
FIELDS = tuple(abi.SURFACE_FIELDS)
SPEC = {k: ((N,) if c == 1 else (N, c), ty) for k, (ty, c) in abi.SURFACE_FIELDS.items()}      # the fields hold -7, the hit's id and t their own sentinels
HIT_SPEC = {"hit_id": ((N,), np.int32, -5), "t": ((N,), np.float32, -1.0)}


def batch(flat):
    """The rays of the case (tests/test_gpu_surface.py pins the host form on the same batch)."""
    return rq.unrelated_rays(flat, N, seed=SEED)


def setup():
    c = open_case(SCENE)
    ds = lib.DeviceScene(c.g.flat)
    rays = batch(c.g.flat)
    plain = ds.surface_rays(rays)
    tr = sr.device_case_intervals(plain["hit_id"], plain["t"])
    host = ds.surface_rays(rays, t_range=tr)
    assert not np.array_equal(host["hit_id"], plain["hit_id"]) and (host["hit_id"] >= 0).sum() > N // 4
    return c, ds, rays, tr, plain, host


def alone(k):
    """Output k asked for alone: the fields not asked for keep their sentinel (what same() looks at, and what of it is untouched)."""
    return dict(keys=(k,) + FIELDS, untouched=tuple(f for f in FIELDS if f != k))


def device_case():
    c, ds, rays, tr, plain, host = setup()
    dev, side = c.dev, c.side
    d_rays, d_tr, d_hit, d_t = c.put(rays, tr, host["hit_id"], host["t"])
    assert d_rays.data_ptr() % 8 == 0 and d_tr.data_ptr() % 8 == 0
    out = Outputs(dev, {**HIT_SPEC, **SPEC}, -7)
    frame = c.render(ds)
    for count in (False, True):
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), count=count, **out.ptrs())
        side.synchronize()
        out.same(host, f"second stream, counting {count}")
    # NULL stream = the scene's own; no interval
    ds.surface_rays_device(N, d_rays.data_ptr(), **out.ptrs())
    assert ds.trace_rays(rays[:4])["hit_id"].shape == (4,)     # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(plain, "own stream, no interval")
    # each output alone, the others NULL; then none of the surface (the call is the closest-hit query)
    for k in ("hit_id", "t") + FIELDS:
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs(keys=(k,)))
        side.synchronize()
        out.same(host, f"only {k}", **alone(k))
    for k in FIELDS:
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=(k,)))
        side.synchronize()
        out.same(host, f"surface_hits, only {k}", **alone(k))
    ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr())
    side.synchronize()
    # rays and t_range 4 bytes further: the narrow loads
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)
    for r, t_, what in ((odd_rays, d_tr, "float-aligned rays"), (d_rays, odd_tr, "float-aligned t_range"), (odd_rays, odd_tr, "float-aligned rays and t_range")):
        ds.surface_rays_device(N, r.data_ptr(), stream=side.cuda_stream, t_range=t_.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(host, what)
    for r, what in ((d_rays, "surface_hits"), (odd_rays, "surface_hits, float-aligned rays")):
        ds.surface_hits_device(N, r.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=FIELDS))
        side.synchronize()
        out.same(host, what, keys=FIELDS)
    # a ray's row depends on the ray and its interval alone
    perm = np.random.default_rng(13).permutation(N)
    d_pr, d_pt = c.put(rays[perm], tr[perm])
    ds.surface_rays_device(N, d_pr.data_ptr(), stream=side.cuda_stream, t_range=d_pt.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same({k: host[k][perm] for k in out.t}, "permuted")

    def shared(sh):
        sh.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)

    # a render beside the queries: pending on torch's stream while both queries run on the second one
    def queries():
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), count=True, **out.ptrs())
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=FIELDS))
    frame.pending_beside("surface queries", side, queries)
    out.same(host, "beside a pending render")
    frame.after()
    print("surface device case: ok")


def graph_case():
    c, ds, rays, tr, plain, host = setup()
    d_rays, d_tr, d_hit, d_t = c.put(rays, tr, host["hit_id"], host["t"])
    out, out2 = Outputs(c.dev, {**HIT_SPEC, **SPEC}, -7), Outputs(c.dev, SPEC, -7)

    def both(stream):
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=stream, t_range=d_tr.data_ptr(), **out.ptrs())
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=stream, **out2.ptrs())
    captured(both, (out, out2), (host, host), ("surface_rays, replay {rep}", "surface_hits, replay {rep}"), [(out, ("hit_id",)), (out2, ("obj",))])
    print("surface graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
