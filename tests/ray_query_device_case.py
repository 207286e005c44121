"""Run by tests/test_gpu_ray_query.py in its own process (torch initialises HIP first): the device entry points of the ray queries
on torch tensors.  `device`: a second stream, results equal to the host entry points', renders before and after untouched.
`graph`: srt_trace_rays_device captured into a hipGraph and replayed."""
import sys
import numpy as np
import torch

from query_device_common import W, H, FOCAL, QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import ray_query_ref as rq

TRACE = ("hit_id", "t", "bary")


def setup():
    c = open_case("ground_bunny")
    ds = lib.DeviceScene(c.g.flat)
    rays = rq.frame_rays(W, H, rq.SHEAR, FOCAL)
    host = ds.trace_rays(rays)
    assert 0.1 < (host["hit_id"] >= 0).mean() < 0.9
    return c, ds, rays, host


def outputs(dev, n, m=None):
    """The closest-hit outputs of n rays and, with m, the occlusion bytes of m shadow rays."""
    spec = {"hit_id": ((n,), np.int32), "t": ((n,), np.float32), "bary": ((n, 3), np.float32)}
    return Outputs(dev, spec if m is None else dict(spec, occluded=((m,), np.uint8)), QUERY_FILL)


def device_case():
    c, ds, rays, host = setup()
    dev, g, side = c.dev, c.g, c.side
    n = rays.shape[0]
    # shadow rays of the frame, for the occlusion entry point
    sel = host["hit_id"] >= 0
    sray = rq.shadow_rays(rays[sel], host["t"][sel], g.light)
    skip = g.flat.tri_obj[host["hit_id"][sel]].astype(np.int32)
    occ_host = ds.occluded(sray, skip)
    d_rays, d_sray, d_skip = c.put(rays, sray, skip)
    m = sray.shape[0]
    frame = c.render(ds)
    out = outputs(dev, n, m)
    want = dict(host, occluded=occ_host)
    for rep in range(2):
        def queries():
            ds.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs(keys=TRACE))
            ds.occluded_device(m, d_sray.data_ptr(), out.t["occluded"].data_ptr(), skip_obj=d_skip.data_ptr(), stream=side.cuda_stream)
        frame.pending_beside(rep, side, queries)
        out.same(want, f"second stream, rep {rep}")
    frame.after()
    # NULL stream = the scene's own stream; outputs may be NULL one by one
    ds.trace_rays_device(n, d_rays.data_ptr(), **out.ptrs(keys=("hit_id",)))
    ds.trace_rays_device(n, d_rays.data_ptr(), **out.ptrs(keys=("t", "bary")))
    assert np.array_equal(ds.occluded(sray, skip), occ_host)   # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(host, "own stream", keys=TRACE)
    odd = float_aligned(dev, d_rays)
    ds.trace_rays_device(n, odd.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=TRACE))
    side.synchronize()
    out.same(host, "float-aligned rays", keys=TRACE)

    def shared(sh):
        sh.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("hit_id",)))
        side.synchronize()
        assert np.array_equal(out.t["hit_id"].cpu().numpy(), host["hit_id"])
    through_shared_handle(ds, shared)
    print("ray query device case: ok")


def graph_case():
    c, ds, rays, host = setup()
    n = rays.shape[0]
    d_rays, = c.put(rays)
    out = outputs(c.dev, n)
    captured(lambda stream: ds.trace_rays_device(n, d_rays.data_ptr(), stream=stream, **out.ptrs(keys=TRACE)), out, host, "replay {rep}", [(out, ("hit_id",))])
    print("ray query graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
