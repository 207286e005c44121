"""Run by tests/test_gpu_shade_range.py in its own process (torch initialises HIP first): srt_shade_rays_range_device on torch tensors.
`device`: a second stream and the scene's own, results equal to the host entry point's (which the tests that call this pin against the
yardstick), a t_range pointer that is only float-aligned, a permuted batch, the identities, two handles of srt_scene_share.
`graph`: the call captured into a hipGraph -- one launch on one stream, the light table already resident -- and replayed."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import shade_query_ref as sq                   # noqa: E402
import shade_range_ref as sr                   # noqa: E402
from query_device_common import bits, float_aligned, through_shared_handle      # noqa: E402

N = sr.DEVICE_CASE_N
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def setup():
    """The batch of shade_range_ref.device_case_inputs / device_case_intervals and what the host forms give for it."""
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(sr.DEVICE_CASE_SCENE)
    ds = lib.DeviceScene(g.flat)
    rays, lights = sr.device_case_inputs(g.flat)
    p = sq.shade_params(lights)
    plain = ds.shade_rays(rays, p)
    tr = sr.device_case_intervals(plain["hit_id"], plain["t"])
    host = ds.shade_rays(rays, p, t_range=tr)              # (the last host call: its light table is on the device)
    assert not np.array_equal(host["hit_id"], plain["hit_id"]) and (host["hit_id"] >= 0).sum() > N // 4
    assert not np.array_equal(bits(host["rgb_linear"]), bits(plain["rgb_linear"]))
    return dev, g, ds, rays, tr, p, plain, host


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

    def same(self, host, what, order=None):
        pick = (lambda a: a) if order is None else (lambda a: a[order])
        assert np.array_equal(self.hit.cpu().numpy(), pick(host["hit_id"])), (what, "hit ids")
        assert np.array_equal(bits(self.t.cpu().numpy()), bits(pick(host["t"]))), (what, "t")
        assert np.array_equal(bits(self.lin.cpu().numpy()), bits(pick(host["rgb_linear"]))), (what, "rgb_linear")
        assert np.array_equal(self.rgb8.cpu().numpy(), pick(host["rgb8"])), (what, "rgb8")
        self.reset()


def device_case():
    dev, g, ds, rays, tr, p, plain, host = setup()
    d_rays, d_tr = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev)
    assert d_tr.data_ptr() % 8 == 0
    out = Outputs(dev, N)
    side = torch.cuda.Stream(device=dev)
    for count in (False, True):
        p.flags = abi.SRT_FLAG_COUNT_WORK if count else 0
        ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        p.flags = 0
        side.synchronize()
        out.same(host, f"second stream, counting {count}")
    # NULL stream = the scene's own stream; outputs may be NULL one by one, and all of them
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr(), hit_id=out.hit.data_ptr(), rgb8=out.rgb8.data_ptr())
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr(), t=out.t.data_ptr(), rgb_linear=out.lin.data_ptr())
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr())
    assert ds.trace_rays(rays[:4])["hit_id"].shape == (4,)     # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(host, "own stream")
    odd = float_aligned(dev, d_tr)                             # the same intervals 4 bytes further: the narrow loads
    ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=odd.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "float-aligned t_range")
    odd_rays = float_aligned(dev, d_rays)
    ds.shade_rays_device(N, odd_rays.data_ptr(), p, stream=side.cuda_stream, t_range=odd.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "float-aligned rays and t_range")
    # a ray's result depends on the ray and its interval alone: the batch in another order
    perm = np.random.default_rng(13).permutation(N)
    d_pr, d_pt = torch.from_numpy(np.ascontiguousarray(rays[perm])).to(dev), torch.from_numpy(np.ascontiguousarray(tr[perm])).to(dev)
    torch.cuda.synchronize()
    ds.shade_rays_device(N, d_pr.data_ptr(), p, stream=side.cuda_stream, t_range=d_pt.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "permuted", perm)
    # the identities, device form: a NULL t_range and the three intervals that bound nothing give srt_shade_rays' bytes
    for pair in (None, (0.0, INF), (-INF, INF), (NAN, NAN)):
        d_id = None if pair is None else torch.from_numpy(np.tile(np.array(pair, np.float32), (N, 1))).to(dev)
        torch.cuda.synchronize()
        ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=None if d_id is None else d_id.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(plain, f"identity {pair}")

    def shared(sh):                                            # two handles of srt_scene_share, each with its own light table
        sh2 = ds.share()
        other = Outputs(dev, N)
        p2 = sq.shade_params(abi.light_staircase(g.light, 3))
        want2 = ds.shade_rays(rays, p2, t_range=tr)
        assert not np.array_equal(bits(want2["rgb_linear"]), bits(host["rgb_linear"]))
        sh.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        sh2.shade_rays_device(N, d_rays.data_ptr(), p2, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **other.ptrs())
        side.synchronize()
        out.same(host, "shared handle"); other.same(want2, "second shared handle, its own table")
        sh2.close()
    through_shared_handle(ds, shared)
    print("shade range device case: ok")


def graph_case():
    dev, g, ds, rays, tr, p, plain, host = setup()             # (the host call with p was the last: its table is on the device)
    d_rays, d_tr = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev)
    out = Outputs(dev, N)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=torch.cuda.current_stream().cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
    torch.cuda.synchronize()
    assert (out.hit.cpu().numpy() == -5).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host, f"replay {rep}")
    print("shade range graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
