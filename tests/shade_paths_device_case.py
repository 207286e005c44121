"""Run by tests/test_gpu_shade_paths.py in its own process (torch initialises HIP first): srt_shade_paths_device on torch tensors -- a
second stream; results equal to the host entry point's (which tests/test_gpu_shade_paths.py pins against tests/shade_path_ref.py on the
same batch); rays and t_range at an address that is only float-aligned; a handle of srt_scene_share; a render beside the call keeps its
pixels, statistics and pipeline string; the single launch captured into a hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import ray_query_ref as rq                     # noqa: E402
import shade_path_ref as sp                    # noqa: E402
import shade_query_ref as sq                   # noqa: E402
from query_device_common import bits, UntouchedRender, float_aligned, through_shared_handle      # noqa: E402

SCENE, N, DEPTH = "cubes4_a40", 257, 3
TORCH = {np.int32: torch.int32, np.float32: torch.float32}


class Outputs:
    def __init__(self, dev):
        self.t = {"rgb_linear": torch.empty((N, 3), dtype=torch.float32, device=dev), "rgb8": torch.empty((N, 3), dtype=torch.uint8, device=dev)}
        for k, (ty, c) in abi.PATH_FIELDS.items():
            self.t["seg_" + k] = torch.empty((DEPTH, N) if c == 1 else (DEPTH, N, c), dtype=TORCH[ty], device=dev)
        self.reset()

    def reset(self):
        for v in self.t.values():
            v.fill_(7)
        torch.cuda.synchronize()

    def ptrs(self):
        return {k: v.data_ptr() for k, v in self.t.items()}

    def same(self, host, what):
        for k, v in self.t.items():
            got, want = v.cpu().numpy(), host[k]
            assert np.array_equal(bits(got), bits(want)) if want.dtype == np.float32 else np.array_equal(got, want), (what, k)
        self.reset()


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(SCENE)
    ds = lib.DeviceScene(g.flat)
    rays = rq.unrelated_rays(g.flat, N)
    lights = sq.lights_for(SCENE, g.light, 3)
    refl = np.float32(sp.REFLECTANCE)
    p = sq.shade_params(lights)
    plain = ds.shade_rays(rays, p)
    tr = np.where((plain["hit_id"] >= 0)[:, None], np.stack([plain["t"] * np.float32(0.5), plain["t"] * np.float32(1.5)], axis=1), np.float32([0.0, np.inf])).astype(np.float32)
    host = ds.shade_paths(rays, p, DEPTH, refl, sp.BOUNCE_T_MIN, t_range=tr)
    assert (host["seg_hit_id"][1] >= 0).sum() > 4
    d_rays, d_tr, d_refl = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev), torch.from_numpy(refl).to(dev)
    out = Outputs(dev)
    side = torch.cuda.Stream(device=dev)
    frame = UntouchedRender(dev, g, ds)

    def call(h, r, t_, stream):
        h.shade_paths_device(N, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sp.BOUNCE_T_MIN, t_range=t_.data_ptr(), stream=stream, **out.ptrs())

    call(ds, d_rays, d_tr, side.cuda_stream); side.synchronize()
    out.same(host, "second stream")
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)
    for r, t_, what in ((odd_rays, d_tr, "float-aligned rays"), (d_rays, odd_tr, "float-aligned t_range"), (odd_rays, odd_tr, "float-aligned rays and t_range")):
        call(ds, r, t_, side.cuda_stream); side.synchronize()
        out.same(host, what)

    def shared(sh):
        call(sh, d_rays, d_tr, side.cuda_stream); side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)

    frame.pending_beside("shade_paths", side, lambda: call(ds, d_rays, d_tr, side.cuda_stream))
    out.same(host, "beside a pending render")
    frame.after()

    # the light table is on the device: the call is one launch, and may be captured
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        call(ds, d_rays, d_tr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out.t["seg_hit_id"].cpu().numpy() == 7).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host, f"replay {rep}")
    print("shade paths device case: ok")


if __name__ == "__main__":
    main()
