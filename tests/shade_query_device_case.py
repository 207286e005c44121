"""Run by tests/test_gpu_shade_query.py in its own process (torch initialises HIP first): srt_shade_rays_device on torch tensors.
`device`: a second stream, results equal to the host entry point's, the light table changed between two calls on one stream, renders
before and after untouched.  `graph`: the call captured into a hipGraph -- one launch on one stream -- and replayed."""
import sys
import numpy as np
import torch

from query_device_common import W, H, FOCAL, QUERY_FILL, Outputs, bits, captured, float_aligned, open_case, shade_spec, through_shared_handle
from simple_raytracer_amd import abi, lib
import ray_query_ref as rq
import shade_query_ref as sq


def setup():
    c = open_case("ground_bunny")
    g = c.g
    ds = lib.DeviceScene(g.flat)
    rays = rq.frame_rays(W, H, rq.SHEAR, FOCAL)
    tables = [sq.lights_for("ground_bunny", g.light, 3), abi.light_staircase(g.light, 3)]
    params = [sq.shade_params(t) for t in tables]
    host = [ds.shade_rays(rays, p) for p in params]
    assert 0.1 < (host[0]["hit_id"] >= 0).mean() < 0.9
    assert not np.array_equal(bits(host[0]["rgb_linear"]), bits(host[1]["rgb_linear"])), "the two light tables give different colours"
    return c, ds, rays, params, host


def device_case():
    c, ds, rays, params, host = setup()
    dev, side = c.dev, c.side
    n = rays.shape[0]
    d_rays, = c.put(rays)
    frame = c.render(ds)
    out = Outputs(dev, shade_spec(n), QUERY_FILL)
    for rep in range(2):
        def queries():
            q = params[0]
            q.flags = abi.SRT_FLAG_COUNT_WORK if rep == 1 else 0
            ds.shade_rays_device(n, d_rays.data_ptr(), q, stream=side.cuda_stream, **out.ptrs())
            q.flags = 0
        frame.pending_beside(rep, side, queries)
        out.same(host[0], f"second stream, rep {rep}")
    frame.after()
    # the light table changes between two calls on one stream: each call sees its own (the second upload is ordered behind the first query)
    other = Outputs(dev, shade_spec(n), QUERY_FILL)
    ds.shade_rays_device(n, d_rays.data_ptr(), params[0], stream=side.cuda_stream, **out.ptrs())
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=side.cuda_stream, **other.ptrs())
    side.synchronize()
    out.same(host[0], "first table"); other.same(host[1], "second table")
    # NULL stream = the scene's own stream; outputs may be NULL one by one; the table of the call before is not sent again
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], **out.ptrs(keys=("hit_id", "rgb8")))
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], **out.ptrs(keys=("t", "rgb_linear")))
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1])
    assert ds.trace_rays(rays[:4])["hit_id"].shape == (4,)     # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(host[1], "own stream")
    odd = float_aligned(dev, d_rays)
    ds.shade_rays_device(n, odd.data_ptr(), params[0], stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(host[0], "float-aligned rays")

    def shared(sh):      # (a light table of its own)
        sh.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(host[1], "shared handle")
    through_shared_handle(ds, shared)
    print("shade query device case: ok")


def graph_case():
    c, ds, rays, params, host = setup()           # (the host call with params[1] was the last: its table is on the device)
    n = rays.shape[0]
    d_rays, = c.put(rays)
    out = Outputs(c.dev, shade_spec(n), QUERY_FILL)
    captured(lambda stream: ds.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=stream, **out.ptrs()), out, host[1], "replay {rep}", [(out, ("hit_id",))])
    print("shade query graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
