"""Run by tests/test_gpu_refract.py in its own process (torch initialises HIP first): the _device forms of the refracting path calls on
torch tensors -- a second stream, results equal to the host forms' (which tests/test_gpu_refract.py pins against tests/refract_ref.py on
the same case); a NULL table in the device form is the _masked call; one launch of srt_shade_paths_refract_device and one of
srt_render_paths_refract_device captured into a hipGraph (a single node each) and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import refract_ref as rf                       # noqa: E402
import render_paths_ref as rpr                 # noqa: E402
import shade_path_ref as sp                    # noqa: E402
import shade_query_ref as sq                   # noqa: E402
import shadow_rule_ref as sh                   # noqa: E402
from query_device_common import float_aligned            # noqa: E402
from shadow_rule_device_case import DEPTH, Outputs, captured    # noqa: E402

SCENE = "cubes4_a40"


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    flat, rays, lights, refl = sp.frame_case(SCENE)
    n = rays.shape[0]
    ior = rf.case_ior(flat)
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl, d_ior = torch.from_numpy(rays).to(dev), torch.from_numpy(refl).to(dev), torch.from_numpy(ior).to(dev)
    side = torch.cuda.Stream(device=dev)
    mirror = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN)
    for label, rule in (("no rule", None), ("SELF", sh.SELF)):
        host = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior)
        assert (host["seg_hit_id"][1] != mirror["seg_hit_id"][1]).any() and (host["rgb8"] != mirror["rgb8"]).any()
        out = Outputs(dev, (n,))

        def call(r, stream, table=d_ior.data_ptr()):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=rule, ior=table,
                                  **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        call(d_rays, side.cuda_stream, 0); side.synchronize()
        out.same(ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule), f"paths, {label}, a NULL table")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}")

    for what, kw in (("whole frame", {}), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=2))):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, rf.BOUNCE_T_MIN, fill=7, shadow=sh.SELF, ior=ior)
        out = Outputs(dev, (ds.rows(fp), ds.cols(fp)))

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, ior=d_ior.data_ptr(), **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}")
    ds.close()
    print("refract device case: ok")


if __name__ == "__main__":
    main()
