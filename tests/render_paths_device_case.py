"""Run by tests/test_gpu_render_paths.py in its own process (torch initialises HIP first): srt_render_paths_device on torch tensors -- a
second stream; results equal to the host entry point's (which tests/test_gpu_render_paths.py pins against the yardstick); a tile share whose
padding keeps the tensors' fill; a handle of srt_scene_share; a render beside the call keeps its pixels, statistics and pipeline string; the
single launch captured into a hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import render_paths_ref as rp                  # noqa: E402
import shade_path_ref as sp                    # noqa: E402
import shade_query_ref as sq                   # noqa: E402
from query_device_common import bits, UntouchedRender, through_shared_handle      # noqa: E402

SCENE, DEPTH, FILL = "ground_bunny", 3, 7
TORCH = {np.int32: torch.int32, np.float32: torch.float32}


class Outputs:
    def __init__(self, dev, rows, cols):
        self.t = {"rgb_linear": torch.empty((rows, cols, 3), dtype=torch.float32, device=dev), "rgb8": torch.empty((rows, cols, 3), dtype=torch.uint8, device=dev)}
        for k, (ty, c) in abi.PATH_FIELDS.items():
            self.t["seg_" + k] = torch.empty((DEPTH, rows, cols) if c == 1 else (DEPTH, rows, cols, c), dtype=TORCH[ty], device=dev)
        self.reset()

    def reset(self):
        for v in self.t.values():
            v.fill_(FILL)
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
    lights = sq.lights_for(SCENE, g.light, 3)
    refl = np.float32(sp.REFLECTANCE[:2])
    d_refl = torch.from_numpy(refl).to(dev)
    side = torch.cuda.Stream(device=dev)
    frame = UntouchedRender(dev, g, ds)

    for what, kw in (("whole frame", {}), ("spp 4", dict(spp=4)), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=3))):
        p = rp.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(p, DEPTH, refl, sp.BOUNCE_T_MIN, fill=FILL)
        assert (host["seg_hit_id"][1][rp.owned(p) >= 0] >= 0).sum() > 20
        out = Outputs(dev, ds.rows(p), ds.cols(p))

        def call(h, stream):
            h.render_paths_device(p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sp.BOUNCE_T_MIN, stream=stream, **out.ptrs())

        call(ds, side.cuda_stream); side.synchronize()
        out.same(host, what + ", second stream")

        def shared(sh):
            call(sh, side.cuda_stream); side.synchronize()
            out.same(host, what + ", shared handle")
        through_shared_handle(ds, shared)

        frame.pending_beside("render_paths", side, lambda: call(ds, side.cuda_stream))
        out.same(host, what + ", beside a pending render")
        frame.after()

        # the light table is on the device: the call is one launch, and may be captured
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, capture_error_mode="thread_local"):
            call(ds, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (out.t["seg_hit_id"].cpu().numpy() == FILL).all(), "a captured launch does not run"
        for rep in range(2):
            gph.replay(); torch.cuda.synchronize()
            out.same(host, what + f", replay {rep}")
    print("render paths device case: ok")


if __name__ == "__main__":
    main()
