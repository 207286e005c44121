"""Run by tests/test_gpu_surface.py in its own process (torch initialises HIP first): srt_surface_rays_device / srt_surface_hits_device on
torch tensors.
`device`: a second stream and the scene's own; results equal to the host entry point's (which tests/test_gpu_surface.py pins against
tests/surface_ref.py on the same batch); each output alone, the others NULL; rays and t_range at an address that is only float-aligned;
a permuted batch; a handle of srt_scene_share; a render beside the queries keeps its pixels, statistics and pipeline string.
`graph`: both _device forms, without SRT_FLAG_COUNT_WORK, captured into a hipGraph and replayed to the same bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
import shade_range_ref as sr                   # noqa: E402
from query_device_common import bits, UntouchedRender, float_aligned, through_shared_handle      # noqa: E402

SCENE, N, SEED = "cubes4_a40", 257, 5
FIELDS = tuple(abi.SURFACE_FIELDS)


def batch(flat):
    """The rays of the case (tests/test_gpu_surface.py pins the host form on the same batch)."""
    return rq.unrelated_rays(flat, N, seed=SEED)


def setup():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(SCENE)
    ds = lib.DeviceScene(g.flat)
    rays = batch(g.flat)
    plain = ds.surface_rays(rays)
    tr = sr.device_case_intervals(plain["hit_id"], plain["t"])
    host = ds.surface_rays(rays, t_range=tr)
    assert not np.array_equal(host["hit_id"], plain["hit_id"]) and (host["hit_id"] >= 0).sum() > N // 4
    return dev, g, ds, rays, tr, plain, host


class Outputs:
    def __init__(self, dev, n):
        self.hit = torch.empty((n,), dtype=torch.int32, device=dev); self.t = torch.empty((n,), dtype=torch.float32, device=dev)
        self.f = {k: torch.empty((n,) if c == 1 else (n, c), dtype=torch.int32 if ty is np.int32 else torch.float32, device=dev)
                  for k, (ty, c) in abi.SURFACE_FIELDS.items()}
        self.reset()

    def reset(self):
        self.hit.fill_(-5); self.t.fill_(-1.0)
        for k, v in self.f.items():
            v.fill_(-7)
        torch.cuda.synchronize()

    def ptrs(self, only=None):
        d = {k: v.data_ptr() for k, v in self.f.items() if only is None or k in only}
        if only is None or "hit_id" in only: d["hit_id"] = self.hit.data_ptr()
        if only is None or "t" in only: d["t"] = self.t.data_ptr()
        return d

    def fields(self, only=None):
        return {k: v.data_ptr() for k, v in self.f.items() if only is None or k in only}

    def same(self, host, what, order=None, only=None, hits=True):
        pick = (lambda a: a) if order is None else (lambda a: a[order])
        if hits and (only is None or "hit_id" in only):
            assert np.array_equal(self.hit.cpu().numpy(), pick(host["hit_id"])), (what, "hit ids")
        if hits and (only is None or "t" in only):
            assert np.array_equal(bits(self.t.cpu().numpy()), bits(pick(host["t"]))), (what, "t")
        for k, v in self.f.items():
            got = v.cpu().numpy()
            if only is not None and k not in only:
                assert (got == -7).all(), (what, k, "an output that was not asked for was written")
                continue
            want = pick(host[k])
            assert np.array_equal(got, want) if k == "obj" else np.array_equal(bits(got), bits(want)), (what, k)
        self.reset()


def device_case():
    dev, g, ds, rays, tr, plain, host = setup()
    d_rays, d_tr = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev)
    assert d_rays.data_ptr() % 8 == 0 and d_tr.data_ptr() % 8 == 0
    d_hit, d_t = torch.from_numpy(host["hit_id"]).to(dev), torch.from_numpy(host["t"]).to(dev)
    out = Outputs(dev, N)
    side = torch.cuda.Stream(device=dev)
    frame = UntouchedRender(dev, g, ds)
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
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs(only=(k,)))
        side.synchronize()
        out.same(host, f"only {k}", only=(k,))
    for k in FIELDS:
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.fields(only=(k,)))
        side.synchronize()
        out.same(host, f"surface_hits, only {k}", only=(k,), hits=False)
    ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr())
    side.synchronize()
    # rays and t_range 4 bytes further: the narrow loads
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)
    for r, t_, what in ((odd_rays, d_tr, "float-aligned rays"), (d_rays, odd_tr, "float-aligned t_range"), (odd_rays, odd_tr, "float-aligned rays and t_range")):
        ds.surface_rays_device(N, r.data_ptr(), stream=side.cuda_stream, t_range=t_.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(host, what)
    for r, what in ((d_rays, "surface_hits"), (odd_rays, "surface_hits, float-aligned rays")):
        ds.surface_hits_device(N, r.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.fields())
        side.synchronize()
        out.same(host, what, hits=False)
    # a ray's row depends on the ray and its interval alone
    perm = np.random.default_rng(13).permutation(N)
    d_pr, d_pt = torch.from_numpy(np.ascontiguousarray(rays[perm])).to(dev), torch.from_numpy(np.ascontiguousarray(tr[perm])).to(dev)
    torch.cuda.synchronize()
    ds.surface_rays_device(N, d_pr.data_ptr(), stream=side.cuda_stream, t_range=d_pt.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "permuted", perm)

    def shared(sh):
        sh.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)

    # a render beside the queries: pending on torch's stream while both queries run on the second one
    def queries():
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=side.cuda_stream, t_range=d_tr.data_ptr(), count=True, **out.ptrs())
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=side.cuda_stream, **out.fields())
    frame.pending_beside("surface queries", side, queries)
    out.same(host, "beside a pending render")
    frame.after()
    print("surface device case: ok")


def graph_case():
    dev, g, ds, rays, tr, plain, host = setup()
    d_rays, d_tr = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev)
    d_hit, d_t = torch.from_numpy(host["hit_id"]).to(dev), torch.from_numpy(host["t"]).to(dev)
    out, out2 = Outputs(dev, N), Outputs(dev, N)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        cur = torch.cuda.current_stream().cuda_stream
        ds.surface_rays_device(N, d_rays.data_ptr(), stream=cur, t_range=d_tr.data_ptr(), **out.ptrs())
        ds.surface_hits_device(N, d_rays.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), stream=cur, **out2.fields())
    torch.cuda.synchronize()
    assert (out.hit.cpu().numpy() == -5).all() and (out2.f["obj"].cpu().numpy() == -7).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host, f"surface_rays, replay {rep}"); out2.same(host, f"surface_hits, replay {rep}", hits=False)
    print("surface graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
