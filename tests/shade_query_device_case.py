"""Run by tests/test_gpu_shade_query.py in its own process (torch initialises HIP first): srt_shade_rays_device on torch tensors.
`device`: a second stream, results equal to the host entry point's, the light table changed between two calls on one stream, renders
before and after untouched.  `graph`: the call captured into a hipGraph -- one launch on one stream -- and replayed."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
import shade_query_ref as sq                   # noqa: E402
from query_device_common import W, H, FOCAL, bits, UntouchedRender, float_aligned, through_shared_handle      # noqa: E402


def setup():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    rays = rq.frame_rays(W, H, rq.SHEAR, FOCAL)
    tables = [sq.lights_for("ground_bunny", g.light, 3), abi.light_staircase(g.light, 3)]
    params = [sq.shade_params(t) for t in tables]
    host = [ds.shade_rays(rays, p) for p in params]
    assert 0.1 < (host[0]["hit_id"] >= 0).mean() < 0.9
    assert not np.array_equal(bits(host[0]["rgb_linear"]), bits(host[1]["rgb_linear"])), "the two light tables give different colours"
    return dev, g, ds, rays, params, host


class Outputs:
    def __init__(self, dev, n):
        self.hit = torch.empty((n,), dtype=torch.int32, device=dev); self.t = torch.empty((n,), dtype=torch.float32, device=dev)
        self.lin = torch.empty((n, 3), dtype=torch.float32, device=dev); self.rgb8 = torch.empty((n, 3), dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        self.hit.fill_(-5); self.t.fill_(-1.0); self.lin.fill_(-1.0); self.rgb8.fill_(7)
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(hit_id=self.hit.data_ptr(), t=self.t.data_ptr(), rgb_linear=self.lin.data_ptr(), rgb8=self.rgb8.data_ptr())

    def same(self, host, what):
        assert np.array_equal(self.hit.cpu().numpy(), host["hit_id"]), (what, "hit ids")
        assert np.array_equal(bits(self.t.cpu().numpy()), bits(host["t"])), (what, "t")
        assert np.array_equal(bits(self.lin.cpu().numpy()), bits(host["rgb_linear"])), (what, "rgb_linear")
        assert np.array_equal(self.rgb8.cpu().numpy(), host["rgb8"]), (what, "rgb8")


def device_case():
    dev, g, ds, rays, params, host = setup()
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays).to(dev)
    frame = UntouchedRender(dev, g, ds)
    side = torch.cuda.Stream(device=dev)
    out = Outputs(dev, n)
    for rep in range(2):
        def queries():
            q = params[0]
            q.flags = abi.SRT_FLAG_COUNT_WORK if rep == 1 else 0
            ds.shade_rays_device(n, d_rays.data_ptr(), q, stream=side.cuda_stream, **out.ptrs())
            q.flags = 0
        frame.pending_beside(rep, side, queries)
        out.same(host[0], f"second stream, rep {rep}")
        out.reset()
    frame.after()
    # the light table changes between two calls on one stream: each call sees its own (the second upload is ordered behind the first query)
    other = Outputs(dev, n)
    ds.shade_rays_device(n, d_rays.data_ptr(), params[0], stream=side.cuda_stream, **out.ptrs())
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=side.cuda_stream, **other.ptrs())
    side.synchronize()
    out.same(host[0], "first table"); other.same(host[1], "second table")
    out.reset(); other.reset()
    # NULL stream = the scene's own stream; outputs may be NULL one by one; the table of the call before is not sent again
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], hit_id=out.hit.data_ptr(), rgb8=out.rgb8.data_ptr())
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1], t=out.t.data_ptr(), rgb_linear=out.lin.data_ptr())
    ds.shade_rays_device(n, d_rays.data_ptr(), params[1])
    assert ds.trace_rays(rays[:4])["hit_id"].shape == (4,)     # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(host[1], "own stream")
    out.reset()
    odd = float_aligned(dev, d_rays)
    ds.shade_rays_device(n, odd.data_ptr(), params[0], stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(host[0], "float-aligned rays")
    out.reset()

    def shared(sh):      # (a light table of its own)
        sh.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(host[1], "shared handle")
    through_shared_handle(ds, shared)
    print("shade query device case: ok")


def graph_case():
    dev, g, ds, rays, params, host = setup()      # (the host call with params[1] was the last: its table is on the device)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays).to(dev)
    out = Outputs(dev, n)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        ds.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=torch.cuda.current_stream().cuda_stream, **out.ptrs())
    torch.cuda.synchronize()
    assert (out.hit.cpu().numpy() == -5).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host[1], f"replay {rep}")
        out.reset()
    print("shade query graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
