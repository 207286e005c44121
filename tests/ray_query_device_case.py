"""Run by tests/test_gpu_ray_query.py in its own process (torch initialises HIP first): the device entry points of the ray queries
on torch tensors.  `device`: a second stream, results equal to the host entry points', renders before and after untouched.
`graph`: srt_trace_rays_device captured into a hipGraph and replayed."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402

W, H, FOCAL = 192, 108, 40.0
STAT_KEYS = ("primary_rays", "hit_rays", "shadow_rays", "node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow", "rows")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    hit, t, bary = outputs(dev, n)
    occ = torch.full((m,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    for rep in range(2):
        # a render is enqueued, the queries run on a second stream while it is pending, then srt_sync: the render's statistics
        fhit.fill_(-5); flin.zero_(); torch.cuda.synchronize()
        ds.render_device(p, stream=cur, hit_id=fhit.data_ptr(), rgb_linear=flin.data_ptr())
        ds.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), count=(rep == 1))
        ds.occluded_device(m, d_sray.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=side.cuda_stream)
        pipe = ds.pipeline
        st = ds.sync()
        side.synchronize(); torch.cuda.synchronize()
        assert {k: st[k] for k in STAT_KEYS} == base[0][2], (rep, st, base[0][2])
        assert pipe == base[0][3] == ds.pipeline
        assert np.array_equal(fhit.cpu().numpy(), base[0][0]) and np.array_equal(bits(flin.cpu().numpy()), bits(base[0][1])), rep
        same(host, hit, t, bary, f"second stream, rep {rep}")
        assert np.array_equal(occ.cpu().numpy(), occ_host), rep
        hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); occ.fill_(7)
    after = render()
    assert after[2] == base[0][2] and np.array_equal(after[0], base[0][0]) and np.array_equal(bits(after[1]), bits(base[0][1]))
    # NULL stream = the scene's own stream; outputs may be NULL one by one
    torch.cuda.synchronize()
    ds.trace_rays_device(n, d_rays.data_ptr(), hit_id=hit.data_ptr())
    ds.trace_rays_device(n, d_rays.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr())
    assert np.array_equal(ds.occluded(sray, skip), occ_host)   # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    same(host, hit, t, bary, "own stream")
    # rays that are only float-aligned take the narrow loads: same results
    odd = torch.empty(n * 6 + 1, dtype=torch.float32, device=dev)
    odd[1:].copy_(d_rays.reshape(-1))
    assert odd[1:].data_ptr() % 8 == 4
    hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); torch.cuda.synchronize()
    ds.trace_rays_device(n, odd[1:].data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr())
    side.synchronize()
    same(host, hit, t, bary, "float-aligned rays")
    # through a shared handle: the one copy of the records
    sh = ds.share()
    hit.fill_(-5); torch.cuda.synchronize()
    sh.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr())
    side.synchronize()
    assert np.array_equal(hit.cpu().numpy(), host["hit_id"])
    assert sh.device_bytes == ds.device_bytes
    sh.close()
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
