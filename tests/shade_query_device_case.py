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

W, H, FOCAL = 192, 108, 40.0
STAT_KEYS = ("primary_rays", "hit_rays", "shadow_rays", "node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow", "rows")
bits = sq.bits


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
    p = g.params(W, H, 2, flags=abi.SRT_FLAG_COUNT_WORK)
    fhit = torch.zeros((H, W), dtype=torch.int32, device=dev); flin = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
    cur = torch.cuda.current_stream().cuda_stream

    def render():
        fhit.fill_(-5); flin.zero_(); torch.cuda.synchronize()
        ds.render_device(p, stream=cur, hit_id=fhit.data_ptr(), rgb_linear=flin.data_ptr())
        st = ds.sync()
        torch.cuda.synchronize()
        return fhit.cpu().numpy().copy(), flin.cpu().numpy().copy(), {k: st[k] for k in STAT_KEYS}, ds.pipeline

    base = [render(), render()]                                # both alternating counter sets
    assert base[0][2] == base[1][2] and base[0][2]["node_tests_primary"] > 0
    side = torch.cuda.Stream(device=dev)
    out = Outputs(dev, n)
    for rep in range(2):
        # a render is enqueued, the query runs on a second stream while it is pending, then srt_sync: the render's statistics
        fhit.fill_(-5); flin.zero_(); torch.cuda.synchronize()
        ds.render_device(p, stream=cur, hit_id=fhit.data_ptr(), rgb_linear=flin.data_ptr())
        q = params[0]
        q.flags = abi.SRT_FLAG_COUNT_WORK if rep == 1 else 0
        ds.shade_rays_device(n, d_rays.data_ptr(), q, stream=side.cuda_stream, **out.ptrs())
        q.flags = 0
        pipe = ds.pipeline
        st = ds.sync()
        side.synchronize(); torch.cuda.synchronize()
        assert {k: st[k] for k in STAT_KEYS} == base[0][2], (rep, st, base[0][2])
        assert pipe == base[0][3] == ds.pipeline
        assert np.array_equal(fhit.cpu().numpy(), base[0][0]) and np.array_equal(bits(flin.cpu().numpy()), bits(base[0][1])), rep
        out.same(host[0], f"second stream, rep {rep}")
        out.reset()
    after = render()
    assert after[2] == base[0][2] and np.array_equal(after[0], base[0][0]) and np.array_equal(bits(after[1]), bits(base[0][1]))
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
    # rays that are only float-aligned take the narrow loads: same results
    odd = torch.empty(n * 6 + 1, dtype=torch.float32, device=dev)
    odd[1:].copy_(d_rays.reshape(-1))
    assert odd[1:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    ds.shade_rays_device(n, odd[1:].data_ptr(), params[0], stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(host[0], "float-aligned rays")
    out.reset()
    # through a shared handle: the one copy of the records, a light table of its own
    sh = ds.share()
    sh.shade_rays_device(n, d_rays.data_ptr(), params[1], stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(host[1], "shared handle")
    assert sh.device_bytes == ds.device_bytes
    sh.close()
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
