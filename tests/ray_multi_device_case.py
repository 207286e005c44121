"""Run by tests/test_gpu_ray_multi.py in its own process (torch initialises HIP first): srt_trace_rays_multi_device on torch tensors.
A second stream, results equal to the host form's (which the parent pins against the yardstick), rays and t_range at addresses that are
only float-aligned, the scene's own stream, a counting call, a shared handle, and one call captured into a hipGraph and replayed twice.
Exits non-zero on the first mismatch."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
from query_device_common import bits, float_aligned, through_shared_handle      # noqa: E402

N, K = 257, 4
INF = np.float32(np.inf)


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("cubes4_a40")
    ds = lib.DeviceScene(g.flat)
    rays = rq.unrelated_rays(g.flat, N, seed=5)
    plain = ds.trace_rays(rays)
    t1 = np.where(plain["hit_id"] >= 0, plain["t"], np.float32(50.0)).astype(np.float32)
    kind = np.arange(N) % 4                    # from the second hit on; nothing; the first hit alone; around the first hit
    tr = np.empty((N, 2), np.float32)
    tr[:, 0] = np.select([kind == 0, kind == 1, kind == 2], [np.nextafter(t1, INF), 0.0, t1], t1 * np.float32(0.5))
    tr[:, 1] = np.select([kind == 0, kind == 1, kind == 2], [INF, np.nextafter(t1, -INF), t1], t1 * np.float32(1.5))
    host, open_ = ds.trace_rays_multi(rays, K, t_range=tr), ds.trace_rays_multi(rays, K)
    assert (host["n_hits"] > 0).sum() > N // 4 and not np.array_equal(host["hit_id"], open_["hit_id"]) and (open_["n_hits"] >= K).any() and (open_["n_hits"] == 0).any()

    d_rays, d_tr = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev)
    assert d_rays.data_ptr() % 8 == 0 and d_tr.data_ptr() % 8 == 0
    cnt = torch.full((N,), 99, dtype=torch.int32, device=dev); hit = torch.full((N, K), -5, dtype=torch.int32, device=dev)
    t = torch.full((N, K), -1.0, dtype=torch.float32, device=dev); bary = torch.full((N, K, 3), -1.0, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def call(h, r_ptr, tr_ptr, stream, count=False):
        h.trace_rays_multi_device(N, r_ptr, K, stream=stream, n_hits=cnt.data_ptr(), hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), count=count,
                                  t_range=tr_ptr)

    def same(want, what):
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), want["n_hits"]), (what, "n_hits")
        assert np.array_equal(hit.cpu().numpy(), want["hit_id"]), (what, "hit ids")
        assert np.array_equal(bits(t.cpu().numpy()), bits(want["t"])), (what, "t")
        assert np.array_equal(bits(bary.cpu().numpy()), bits(want["bary"])), (what, "bary")
        cnt.fill_(99); hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0)
        torch.cuda.synchronize()

    for count in (False, True):
        call(ds, d_rays.data_ptr(), d_tr.data_ptr(), side.cuda_stream, count)
        side.synchronize()
        same(host, f"second stream, counting {count}")
    call(ds, d_rays.data_ptr(), None, side.cuda_stream)
    side.synchronize()
    same(open_, "NULL t_range")
    call(ds, d_rays.data_ptr(), d_tr.data_ptr(), 0)            # NULL stream = the scene's own stream
    ds.occluded(rays)                                          # (a host call on the same stream waits for it)
    same(host, "own stream")
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)      # 4 bytes further: the narrow loads
    call(ds, odd_rays.data_ptr(), odd_tr.data_ptr(), side.cuda_stream)
    side.synchronize()
    same(host, "float-aligned rays and t_range")
    # only some outputs
    ds.trace_rays_multi_device(N, d_rays.data_ptr(), K, stream=side.cuda_stream, t=t.data_ptr(), t_range=d_tr.data_ptr())
    side.synchronize()
    assert np.array_equal(bits(t.cpu().numpy()), bits(host["t"])) and (hit.cpu().numpy() == -5).all() and (cnt.cpu().numpy() == 99).all()
    t.fill_(-1.0); torch.cuda.synchronize()

    def shared(sh):
        call(sh, d_rays.data_ptr(), d_tr.data_ptr(), side.cuda_stream)
        side.synchronize()
        same(host, "shared handle")
    through_shared_handle(ds, shared)

    # one call captured into a graph (one launch, nothing allocated or copied), replayed twice
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        call(ds, d_rays.data_ptr(), d_tr.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == -5).all() and (cnt.cpu().numpy() == 99).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        same(host, f"replay {rep}")
    print("ray multi device case: ok")


if __name__ == "__main__":
    main()
