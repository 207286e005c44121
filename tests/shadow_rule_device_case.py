"""Run by tests/test_gpu_shadow_rule.py in its own process (torch initialises HIP first): srt_shade_paths_shadow_device and
srt_render_paths_shadow_device on torch tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_shadow_rule.py
pins against tests/shadow_rule_ref.py on the same cases); rays at an address that is only float-aligned; each single launch captured
into a hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import render_paths_ref as rpr                 # noqa: E402
import shade_query_ref as sq                   # noqa: E402
import shadow_rule_ref as sh                   # noqa: E402
from query_device_common import bits, float_aligned      # noqa: E402

SCENE, DEPTH, FILL = "cubes4_a40", sh.DEPTH, 7
TORCH = {np.int32: torch.int32, np.float32: torch.float32}


class Outputs:
    def __init__(self, dev, shape):
        self.t = {"rgb_linear": torch.empty(shape + (3,), dtype=torch.float32, device=dev), "rgb8": torch.empty(shape + (3,), dtype=torch.uint8, device=dev)}
        for k, (ty, c) in abi.PATH_FIELDS.items():
            self.t["seg_" + k] = torch.empty((DEPTH,) + shape + (() if c == 1 else (c,)), dtype=TORCH[ty], device=dev)
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


def captured(call, out, host, what):
    """The launch captured into a graph (it does not run), then replayed twice: the eager bits."""
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out.t["seg_hit_id"].cpu().numpy() == FILL).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host, f"{what}, replay {rep}")


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    flat, rays, lights, refl = sh.lamp_case(SCENE)
    n = rays.shape[0]
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl = torch.from_numpy(rays).to(dev), torch.from_numpy(refl).to(dev)
    side = torch.cuda.Stream(device=dev)
    plain = ds.shade_paths(rays, p, DEPTH, refl, sh.BOUNCE_T_MIN)
    for label, rule in (("SELF", sh.SELF), ("ENDED", sh.ENDED)):
        host = ds.shade_paths(rays, p, DEPTH, refl, sh.BOUNCE_T_MIN, shadow=rule)
        assert (host["rgb8"] != plain["rgb8"]).any()
        out = Outputs(dev, (n,))

        def call(r, stream):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sh.BOUNCE_T_MIN, stream=stream, shadow=rule, **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        odd = float_aligned(dev, d_rays)
        call(odd, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}")

    for what, kw in (("whole frame", {}), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=2))):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, sh.BOUNCE_T_MIN, fill=FILL, shadow=sh.SELF)
        out = Outputs(dev, (ds.rows(fp), ds.cols(fp)))

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sh.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}")
    ds.close()
    print("shadow rule device case: ok")


if __name__ == "__main__":
    main()
