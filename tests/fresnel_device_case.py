"""Run by tests/test_gpu_fresnel.py in its own process (torch initialises HIP first): the _device forms of the Fresnel path calls on torch
tensors -- a second stream, results equal to the host forms' (which tests/test_gpu_fresnel.py pins against tests/fresnel_ref.py on the
same case), the side rays' rows included; rays at an address that is only float-aligned; a NULL f0 in the device form is the _refract
call and leaves the side rows alone; a handle of srt_scene_share; a render pending on another stream stays untouched; one launch of
srt_shade_paths_fresnel_device and one of srt_render_paths_fresnel_device captured into a hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import fresnel_ref as fr                       # noqa: E402
import golden_util as gu                       # noqa: E402
import refract_ref as rf                       # noqa: E402
import render_paths_ref as rpr                 # noqa: E402
import shade_path_ref as sp                    # noqa: E402
import shade_query_ref as sq                   # noqa: E402
import shadow_rule_ref as sh                   # noqa: E402
from query_device_common import bits, float_aligned, UntouchedRender, through_shared_handle      # noqa: E402

SCENE, DEPTH, FILL = "cubes4_a40", 3, 7
TORCH = {np.int32: torch.int32, np.float32: torch.float32}
SIDE_ARG = {"side_hit_id": "side_hit_id", "side_t": "side_t", "side_rgb_linear": "side_rgb_linear", "fresnel": "side_fresnel"}      # result key -> argument


class Outputs:
    def __init__(self, dev, shape):
        self.t = {"rgb_linear": torch.empty(shape + (3,), dtype=torch.float32, device=dev), "rgb8": torch.empty(shape + (3,), dtype=torch.uint8, device=dev)}
        for k, (ty, c) in abi.PATH_FIELDS.items():
            self.t["seg_" + k] = torch.empty((DEPTH,) + shape + (() if c == 1 else (c,)), dtype=TORCH[ty], device=dev)
        for k, (ty, c) in abi.FRESNEL_FIELDS.items():
            self.t["fresnel" if k == "fresnel" else "side_" + k] = torch.empty((DEPTH,) + shape + (() if c == 1 else (c,)), dtype=TORCH[ty], device=dev)
        self.reset()

    def reset(self):
        for v in self.t.values():
            v.fill_(FILL)
        torch.cuda.synchronize()

    def ptrs(self):
        return {SIDE_ARG.get(k, k): v.data_ptr() for k, v in self.t.items()}

    def same(self, host, what, untouched=()):
        for k, v in self.t.items():
            got = v.cpu().numpy()
            if k in untouched:
                assert (got == FILL).all(), (what, k, "written")
                continue
            want = host[k]
            assert np.array_equal(bits(got), bits(want)) if want.dtype == np.float32 else np.array_equal(got, want), (what, k)
        self.reset()


def captured(call, out, host, what):
    """The launch captured into a graph (it does not run), then replayed twice: the eager bits."""
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (out.t["seg_hit_id"].cpu().numpy() == FILL).all() and (out.t["side_hit_id"].cpu().numpy() == FILL).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        out.same(host, f"{what}, replay {rep}")


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    flat, rays, lights, refl = sp.frame_case(SCENE)
    n = rays.shape[0]
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl, d_ior, d_f0 = (torch.from_numpy(a).to(dev) for a in (rays, refl, ior, f0))
    side = torch.cuda.Stream(device=dev)
    frame = UntouchedRender(dev, gu.GoldenScene(SCENE), ds)
    want_all = sp.ALL_KEYS + fr.SIDE_KEYS
    glass = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, ior=ior)
    for label, rule in (("no rule", None), ("SELF", sh.SELF)):
        host = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior, fresnel=f0, want=want_all)
        assert (host["side_hit_id"] >= 0).any() and (host["rgb8"] != glass["rgb8"]).any()
        out = Outputs(dev, (n,))

        def call(h, r, stream, table=d_f0.data_ptr()):
            h.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=rule, ior=d_ior.data_ptr(),
                                 fresnel=table, **out.ptrs())

        call(ds, d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(ds, float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        call(ds, d_rays, side.cuda_stream, 0); side.synchronize()
        out.same(ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior), f"paths, {label}, a NULL f0", untouched=fr.SIDE_KEYS)

        def shared(h):
            call(h, d_rays, side.cuda_stream); side.synchronize()
            out.same(host, f"paths, {label}, shared handle")
        through_shared_handle(ds, shared)
        frame.pending_beside("fresnel paths", side, lambda: call(ds, d_rays, side.cuda_stream))
        out.same(host, f"paths, {label}, beside a pending render")
        frame.after()
        captured(lambda stream: call(ds, d_rays, stream), out, host, f"paths, {label}")

    for what, kw in (("whole frame", {}), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=2))):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, rf.BOUNCE_T_MIN, fill=FILL, shadow=sh.SELF, ior=ior, fresnel=f0, want=want_all)
        assert (host["side_hit_id"][rpr.owned(fp)[None].repeat(DEPTH, 0) >= 0] >= 0).any()
        out = Outputs(dev, (ds.rows(fp), ds.cols(fp)))

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, ior=d_ior.data_ptr(),
                                   fresnel=d_f0.data_ptr(), **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}")
    ds.close()
    print("fresnel device case: ok")


if __name__ == "__main__":
    main()
