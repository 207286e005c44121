#!/usr/bin/env python3
"""examples/mirror_device.py's picture in ONE call: the K3 scene (bunny on its ground slab) seen through the frame's camera rays,
every ray followed through `depth` segments (the primary hit and depth - 1 mirror bounces) by srt_shade_paths_device, each hit shaded,
the bounces mixed by the objects' reflectance, the finished linear picture written -- where mirror_device.py takes a render, two
surface queries, two shaded queries and torch kernels for the intervals and the mix.  Depth 3 is mirror_device.py's two bounces.
At depth 3 the per-segment rows are also checked against the chain of existing device calls.
Usage: python examples/mirror_path.py [out.bmp [width height [depth]]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import display_tone, write_bmp, N_LIGHTS, T_MIN      # noqa: E402
from mirror_device import REFLECTANCE          # noqa: E402


def main():
    a = sys.argv[1:]
    out = a[0] if a else "mirror_path.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    depth = int(a[3]) if len(a) >= 4 else 3
    n = W * H
    focal = float(np.float32(400.0 * W / 1920.0))
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    p_rays = abi.make_params(1, 1, abi.light_staircase(g.light, N_LIGHTS))      # lights, literals, flags: the frame fields are ignored
    refl = torch.tensor(REFLECTANCE, dtype=torch.float32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    with torch.cuda.stream(side):
        rays0 = torch.zeros((H, W, 6), dtype=torch.float32, device=dev)
        rays0[..., 3] = (int(-W / 2) + torch.arange(W, device=dev)).float()[None, :]
        rays0[..., 4] = (int(-H / 2) + torch.arange(H, device=dev)).float()[:, None]
        rays0[..., 5] = focal
        rays0 = rays0.reshape(n, 6)
        lin, hit, obj, seg_lin, seg_rays = f32(n, 3), i32(depth, n), i32(depth, n), f32(depth, n, 3), f32(depth, n, 6)
        ds.shade_paths_device(n, rays0.data_ptr(), p_rays, depth, reflectance=refl.data_ptr(), bounce_t_min=T_MIN, stream=cur, rgb_linear=lin.data_ptr(),
                              seg_hit_id=hit.data_ptr(), seg_obj=obj.data_ptr(), seg_rgb_linear=seg_lin.data_ptr(), seg_rays=seg_rays.data_ptr())
        if depth == 3:      # the chain of existing device calls gives the same rows
            ray, tr = rays0, None
            for b in range(depth):
                h, o_, c, nxt = i32(n), i32(n), f32(n, 3), f32(n, 6)
                ds.shade_rays_device(n, ray.data_ptr(), p_rays, stream=cur, hit_id=h.data_ptr(), rgb_linear=c.data_ptr(), t_range=tr.data_ptr() if tr is not None else None)
                ds.surface_rays_device(n, ray.data_ptr(), stream=cur, obj=o_.data_ptr(), bounce=nxt.data_ptr(), t_range=tr.data_ptr() if tr is not None else None)
                side.synchronize()
                assert torch.equal(h, hit[b]) and torch.equal(o_, obj[b]) and torch.equal(c.view(torch.int32), seg_lin[b].view(torch.int32)), f"segment {b} differs from the chain"
                assert torch.equal(ray.view(torch.int32), seg_rays[b].view(torch.int32)), f"the ray of segment {b} differs from the chain"
                tr = f32(n, 2)
                tr[:, 0] = torch.where(o_ >= 0, T_MIN, 1.0)
                tr[:, 1] = torch.where(o_ >= 0, float("inf"), 0.0)
                ray = nxt
    side.synchronize()
    rgb8 = display_tone(lin.cpu().numpy())
    rgb8[hit[0].cpu().numpy() < 0] = np.array(abi.REFERENCE_BACKGROUND, np.uint8)
    write_bmp(out, rgb8.reshape(H, W, 3))
    counts = [int((hit[b] >= 0).sum()) for b in range(min(depth, 3))] + [0] * (3 - min(depth, 3))
    print(f"{out}: {W}x{H}, {counts[0]} pixels on a surface, {counts[1]} mirrored rays see the scene, {counts[2]} see it again after the second bounce")
    ds.close()


if __name__ == "__main__":
    main()
