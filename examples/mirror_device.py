#!/usr/bin/env python3
"""examples/mirror.py's picture with TWO bounces, composed entirely on torch device tensors: the K3 scene (bunny on its ground slab)
rendered in camera mode; srt_surface_hits_device turns the frame's own hit_id / t and camera rays into the surface under every pixel
and its mirrored ray; srt_shade_rays_range_device says what colour comes back along that ray; srt_surface_rays_device finds what the
mirrored ray meets and mirrors it once more; a last srt_shade_rays_range_device shades the second bounce.  The caller keeps no copy of
the triangles, computes no normal and orients none; nothing but the finished picture goes back through the host.
A mirrored ray starts AT the hit point -- the origin is not moved -- and its interval (T_MIN, +inf) keeps it off the surface it starts
on; a pixel without a hit carries the interval (1, 0), a miss by definition.
Usage: python examples/mirror_device.py [out.bmp [width height]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import display_tone, write_bmp, N_LIGHTS, T_MIN      # noqa: E402

REFLECTANCE = (0.6, 0.25)      # object 0 of the scene is the slab, object 1 the bunny


def main():
    a = sys.argv[1:]
    out = a[0] if a else "mirror_device.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    n = W * H
    focal = float(np.float32(400.0 * W / 1920.0))
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    lights = abi.light_staircase(g.light, N_LIGHTS)
    p_rays = abi.make_params(1, 1, lights)                 # lights, literals, flags: the frame fields are ignored
    refl = torch.tensor(REFLECTANCE, dtype=torch.float32, device=dev)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    with torch.cuda.stream(side):
        # the frame, in camera mode with the identity matrix: rays leave the origin with direction (i, j, focal)
        hit0, t0, lin0 = i32(n), f32(n), f32(n, 3)
        eye = np.eye(4, dtype=np.float32).reshape(-1)
        ds.render_device(abi.make_params(W, H, lights, focal=focal, ray_matrix=eye, flags=abi.SRT_FLAG_NO_TIMING), stream=cur, hit_id=hit0.data_ptr(), t=t0.data_ptr(),
                         rgb_linear=lin0.data_ptr())
        rays0 = torch.zeros((H, W, 6), dtype=torch.float32, device=dev)
        rays0[..., 3] = (int(-W / 2) + torch.arange(W, device=dev)).float()[None, :]
        rays0[..., 4] = (int(-H / 2) + torch.arange(H, device=dev)).float()[:, None]
        rays0[..., 5] = focal
        rays0 = rays0.reshape(n, 6)

        def interval(obj):
            """(T_MIN, +inf) where there is a surface to leave, (1, 0) -- a miss -- where there is none."""
            tr = f32(n, 2)
            tr[:, 0] = torch.where(obj >= 0, T_MIN, 1.0)
            tr[:, 1] = torch.where(obj >= 0, float("inf"), 0.0)
            return tr

        # bounce 1: the surface under the frame's own hits (no walk), its mirrored ray, the colour that comes back along it
        obj0, ray1 = i32(n), f32(n, 6)
        ds.surface_hits_device(n, rays0.data_ptr(), hit0.data_ptr(), t0.data_ptr(), stream=cur, obj=obj0.data_ptr(), bounce=ray1.data_ptr())
        tr1 = interval(obj0)
        lin1 = f32(n, 3)
        ds.shade_rays_device(n, ray1.data_ptr(), p_rays, stream=cur, rgb_linear=lin1.data_ptr(), t_range=tr1.data_ptr())
        # bounce 2: what the mirrored ray meets, mirrored again
        obj1, ray2 = i32(n), f32(n, 6)
        ds.surface_rays_device(n, ray1.data_ptr(), stream=cur, obj=obj1.data_ptr(), bounce=ray2.data_ptr(), t_range=tr1.data_ptr())
        tr2 = interval(obj1)
        hit2, lin2 = i32(n), f32(n, 3)
        ds.shade_rays_device(n, ray2.data_ptr(), p_rays, stream=cur, hit_id=hit2.data_ptr(), rgb_linear=lin2.data_ptr(), t_range=tr2.data_ptr())
        # mix from the far end: a surface shows its own colour and, by its object's reflectance, what its mirrored ray sees
        k1 = torch.where((obj1 >= 0) & (hit2 >= 0), refl[obj1.clamp(min=0).long()], 0.0)[:, None]
        c1 = (1.0 - k1) * lin1 + k1 * lin2
        k0 = torch.where((obj0 >= 0) & (obj1 >= 0), refl[obj0.clamp(min=0).long()], 0.0)[:, None]
        lin = (1.0 - k0) * lin0 + k0 * c1
    side.synchronize()
    rgb8 = display_tone(lin.cpu().numpy())
    rgb8[hit0.cpu().numpy() < 0] = np.array(abi.REFERENCE_BACKGROUND, np.uint8)
    write_bmp(out, rgb8.reshape(H, W, 3))
    print(f"{out}: {W}x{H}, {int((obj0 >= 0).sum())} pixels on a surface, {int((obj1 >= 0).sum())} mirrored rays see the scene, "
          f"{int((hit2 >= 0).sum())} see it again after the second bounce")
    ds.close()


if __name__ == "__main__":
    main()
