"""Run by tests/test_gpu_ao.py in its own process (torch initialises HIP first): the _device forms of the ambient-occlusion calls on torch
tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_ao.py pins against tests/ao_ref.py on the same batch);
rays at an address that is only float-aligned; a shared handle; a render pending on another stream stays untouched; both calls captured
into one hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import ao_ref as ar                            # noqa: E402
import golden_util as gu                       # noqa: E402
from query_device_common import UntouchedRender, bits, float_aligned, through_shared_handle      # noqa: E402

SCENE, T_MAX = "cubes4_a40", 60.0
DIRS = ar.directions(40)                       # two words a row, a partial chunk


def batch():
    """(flat, rays): every other ray of the lamp case's frame."""
    flat, rays = ar.case_rays(SCENE)
    return flat, np.ascontiguousarray(rays[::2])


class Outputs:
    def __init__(self, dev, n, words):
        self.hit = torch.empty(n, dtype=torch.int32, device=dev); self.t = torch.empty(n, dtype=torch.float32, device=dev)
        self.cnt = torch.empty(n, dtype=torch.int32, device=dev); self.ao = torch.empty(n, dtype=torch.float32, device=dev)
        self.words = torch.empty((n, words), dtype=torch.int32, device=dev)
        self.fill()

    def fill(self):
        self.hit.fill_(-5); self.t.fill_(-1.0); self.cnt.fill_(-5); self.ao.fill_(-1.0); self.words.fill_(-5)
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(n_occluded=self.cnt.data_ptr(), ao=self.ao.data_ptr(), occ_bits=self.words.data_ptr())

    def untouched(self):
        return (self.cnt.cpu().numpy() == -5).all() and (self.words.cpu().numpy() == -5).all() and (self.hit.cpu().numpy() == -5).all()

    def same(self, want, what, hits=True):
        if hits:
            assert np.array_equal(self.hit.cpu().numpy(), want["hit_id"]), (what, "hit ids")
            assert np.array_equal(bits(self.t.cpu().numpy()), bits(want["t"])), (what, "t")
        assert np.array_equal(self.cnt.cpu().numpy().view(np.uint32), want["n_occluded"]), (what, "n_occluded")
        assert np.array_equal(bits(self.ao.cpu().numpy()), bits(want["ao"])), (what, "ao")
        assert np.array_equal(self.words.cpu().numpy().view(np.uint32), want["occ_bits"]), (what, "occ_bits")
        self.fill()


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(SCENE)
    flat, rays = batch()
    n, k = rays.shape[0], DIRS.shape[0]
    ds = lib.DeviceScene(flat)
    host = ds.ao_rays(rays, DIRS, t_max=T_MAX, skip_self=True)
    assert 0 < (host["n_occluded"] > 0).sum() < (host["hit_id"] >= 0).sum()
    d_rays, d_dirs = torch.from_numpy(rays).to(dev), torch.from_numpy(DIRS).to(dev)
    d_hit, d_t = torch.from_numpy(host["hit_id"]).to(dev), torch.from_numpy(host["t"]).to(dev)
    out, out_h = Outputs(dev, n, (k + 31) // 32), Outputs(dev, n, (k + 31) // 32)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def both(handle, r, stream, count=False):
        handle.ao_rays_device(n, r.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, hit_id=out.hit.data_ptr(), t=out.t.data_ptr(),
                              **out.ptrs())
        handle.ao_hits_device(n, r.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **out_h.ptrs())

    def same(what):
        out.same(host, what); out_h.same(host, what + ", ao_hits", hits=False)

    render = UntouchedRender(dev, g, ds)
    for count in (False, True):
        render.pending_beside(count, side, lambda: both(ds, d_rays, side.cuda_stream, count))
        same(f"second stream beside a pending render, counting {count}")
    render.after()
    both(ds, float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
    same("rays only float-aligned")
    through_shared_handle(ds, lambda sh: (both(sh, d_rays, side.cuda_stream), side.synchronize()))
    same("a shared handle")
    # both calls in one captured graph, replayed twice
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        both(ds, d_rays, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.untouched() and out_h.cnt.cpu().numpy().min() == -5, "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        same(f"replay {rep}")
    render.after()
    ds.close()
    print("ao device case: ok")


if __name__ == "__main__":
    main()
