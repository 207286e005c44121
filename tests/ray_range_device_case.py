"""Run by tests/test_gpu_ray_range.py in its own process (torch initialises HIP first): the device entry points of the ray queries with
a t interval on torch tensors.  `device`: a second stream, results equal to the host forms', the identities, a t_range pointer that is
only float-aligned, a shared handle.  `graph`: one range call of each kind captured into a hipGraph and replayed once."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
from query_device_common import bits, float_aligned, through_shared_handle      # noqa: E402

N = 257
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def setup():
    """cubes4_a40, N unrelated rays, one interval per ray around the ray's own first hit (kinds dealt round robin), and what the host
    forms -- pinned against the yardstick by the tests that call this -- give for them."""
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("cubes4_a40")
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
    return dev, g, ds, rays, tr, skip, plain, host, occ


def outputs(dev):
    return (torch.full((N,), -5, dtype=torch.int32, device=dev), torch.full((N,), -1.0, dtype=torch.float32, device=dev),
            torch.full((N, 3), -1.0, dtype=torch.float32, device=dev), torch.full((N,), 7, dtype=torch.uint8, device=dev))


def same(want, want_occ, out, what):
    hit, t, bary, occ = out
    assert np.array_equal(hit.cpu().numpy(), want["hit_id"]), (what, "hit ids")
    assert np.array_equal(bits(t.cpu().numpy()), bits(want["t"])), (what, "t")
    assert np.array_equal(bits(bary.cpu().numpy()), bits(want["bary"])), (what, "bary")
    assert np.array_equal(occ.cpu().numpy(), want_occ), (what, "occluded")
    hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); occ.fill_(7)
    torch.cuda.synchronize()


def device_case():
    dev, g, ds, rays, tr, skip, plain, host, occ_host = setup()
    d_rays, d_tr, d_skip = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev), torch.from_numpy(skip).to(dev)
    assert d_tr.data_ptr() % 8 == 0
    out = outputs(dev)
    hit, t, bary, occ = out
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def both(h, tr_ptr, stream, count=False):
        h.trace_rays_device(N, d_rays.data_ptr(), stream=stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), count=count, t_range=tr_ptr)
        h.occluded_device(N, d_rays.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=stream, t_range=tr_ptr)
    for count in (False, True):
        both(ds, d_tr.data_ptr(), side.cuda_stream, count)
        side.synchronize()
        same(host, occ_host, out, f"second stream, counting {count}")
    both(ds, d_tr.data_ptr(), 0)                               # NULL stream = the scene's own stream
    ds.occluded(rays, skip)                                    # (a host call on the same stream waits for it)
    same(host, occ_host, out, "own stream")
    odd = float_aligned(dev, d_tr)                             # the same intervals 4 bytes further: the narrow loads
    both(ds, odd.data_ptr(), side.cuda_stream)
    side.synchronize()
    same(host, occ_host, out, "float-aligned t_range")
    # the identities, device forms: a NULL t_range and the three intervals that bound nothing give the unbounded calls' bits
    occ_plain = ds.occluded(rays, skip)
    for pair in (None, (0.0, INF), (-INF, INF), (NAN, NAN)):
        d_id = None if pair is None else torch.from_numpy(np.tile(np.array(pair, np.float32), (N, 1))).to(dev)
        torch.cuda.synchronize()
        both(ds, None if d_id is None else d_id.data_ptr(), side.cuda_stream)
        side.synchronize()
        same(plain, occ_plain, out, f"identity {pair}")

    def shared(sh):
        both(sh, d_tr.data_ptr(), side.cuda_stream)
        side.synchronize()
        same(host, occ_host, out, "shared handle")
    through_shared_handle(ds, shared)
    print("ray range device case: ok")


def graph_case():
    dev, g, ds, rays, tr, skip, plain, host, occ_host = setup()
    d_rays, d_tr, d_skip = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev), torch.from_numpy(skip).to(dev)
    out = outputs(dev)
    hit, t, bary, occ = out
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        cur = torch.cuda.current_stream().cuda_stream
        ds.trace_rays_device(N, d_rays.data_ptr(), stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), t_range=d_tr.data_ptr())
        ds.occluded_device(N, d_rays.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=cur, t_range=d_tr.data_ptr())
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == -5).all() and (occ.cpu().numpy() == 7).all(), "a captured launch does not run"
    gph.replay(); torch.cuda.synchronize()
    same(host, occ_host, out, "replay")
    print("ray range graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
