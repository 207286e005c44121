"""Run by tests/test_gpu_ray_query.py in its own process (torch initialises HIP first): the device entry points of the ray queries
on torch tensors.  `device`: a second stream, results equal to the host entry points', renders before and after untouched.
`graph`: srt_trace_rays_device captured into a hipGraph and replayed."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
from query_device_common import W, H, FOCAL, bits, UntouchedRender, float_aligned, through_shared_handle      # noqa: E402


def setup():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    rays = rq.frame_rays(W, H, rq.SHEAR, FOCAL)
    host = ds.trace_rays(rays)
    assert 0.1 < (host["hit_id"] >= 0).mean() < 0.9
    return dev, g, ds, rays, host


def outputs(dev, n):
    return (torch.full((n,), -5, dtype=torch.int32, device=dev), torch.full((n,), -1.0, dtype=torch.float32, device=dev),
            torch.full((n, 3), -1.0, dtype=torch.float32, device=dev))


def same(host, hit, t, bary, what):
    assert np.array_equal(hit.cpu().numpy(), host["hit_id"]), (what, "hit ids")
    assert np.array_equal(bits(t.cpu().numpy()), bits(host["t"])), (what, "t")
    assert np.array_equal(bits(bary.cpu().numpy()), bits(host["bary"])), (what, "bary")


def device_case():
    dev, g, ds, rays, host = setup()
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays).to(dev)
    # shadow rays of the frame, for the occlusion entry point
    sel = host["hit_id"] >= 0
    sray = rq.shadow_rays(rays[sel], host["t"][sel], g.light)
    skip = g.flat.tri_obj[host["hit_id"][sel]].astype(np.int32)
    occ_host = ds.occluded(sray, skip)
    d_sray, d_skip = torch.from_numpy(sray).to(dev), torch.from_numpy(skip).to(dev)
    m = sray.shape[0]
    frame = UntouchedRender(dev, g, ds)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    hit, t, bary = outputs(dev, n)
    occ = torch.full((m,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):
        def queries():
            ds.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), count=(rep == 1))
            ds.occluded_device(m, d_sray.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=side.cuda_stream)
        frame.pending_beside(rep, side, queries)
        same(host, hit, t, bary, f"second stream, rep {rep}")
        assert np.array_equal(occ.cpu().numpy(), occ_host), rep
        hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); occ.fill_(7)
    frame.after()
    # NULL stream = the scene's own stream; outputs may be NULL one by one
    torch.cuda.synchronize()
    ds.trace_rays_device(n, d_rays.data_ptr(), hit_id=hit.data_ptr())
    ds.trace_rays_device(n, d_rays.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr())
    assert np.array_equal(ds.occluded(sray, skip), occ_host)   # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    same(host, hit, t, bary, "own stream")
    odd = float_aligned(dev, d_rays)
    hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); torch.cuda.synchronize()
    ds.trace_rays_device(n, odd.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr())
    side.synchronize()
    same(host, hit, t, bary, "float-aligned rays")
    hit.fill_(-5); torch.cuda.synchronize()

    def shared(sh):
        sh.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr())
        side.synchronize()
        assert np.array_equal(hit.cpu().numpy(), host["hit_id"])
    through_shared_handle(ds, shared)
    print("ray query device case: ok")


def graph_case():
    dev, g, ds, rays, host = setup()
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays).to(dev)
    hit, t, bary = outputs(dev, n)
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        ds.trace_rays_device(n, d_rays.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr())
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == -5).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        same(host, hit, t, bary, f"replay {rep}")
        hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); torch.cuda.synchronize()
    print("ray query graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
