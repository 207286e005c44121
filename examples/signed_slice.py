#!/usr/bin/env python3
"""A SIGNED distance-field slice through a closed mesh (the horse of tests/golden/meshes), on torch device tensors: the slice of
examples/distance_slice.py with a sign.  A grid of points in the plane z = the horse's middle, srt_signed_points_device for all of them
in one launch -- srt_nearest_points' distance, no radius to choose, and the sign by winding along the header's three directions
(include/srt_signed.h) --, and a picture of the signed distance: iso-bands every BAND units, warm inside, cold outside, the surface itself
white.  The points are made on the device and the picture is made there; nothing but the finished picture goes back through the host.
The mesh is closed and its normals point out, which is what the sign is defined for; the bunny of the other examples has holes.
Usage: python examples/signed_slice.py [out.bmp [width height]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import build, host, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import scenes                                  # noqa: E402
from mirror import write_bmp                   # noqa: E402

BAND = 0.1                                     # of the slice's half width


def horse():
    """The flat scene of the horse alone, through the host mirror's builder."""
    build.build_host()
    m = gu.load_mesh("horse")
    recipe = scenes.Recipe()
    recipe.load("horse", "horse"); recipe.bvh("horse")
    recipe.light = (0.0, 0.0, 0.0)
    return host.build_flat_scene(recipe, {"horse": m["points"] if isinstance(m, dict) else m})


def main():
    a = sys.argv[1:]
    out = a[0] if a else "signed_slice.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    n = W * H
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    flat = horse()
    ds = lib.DeviceScene(flat)
    P = np.ascontiguousarray(flat.tri_points, np.float32)[..., :3].reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    mid, half = (lo + hi) / 2, 0.6 * float(max(hi[0] - lo[0], (hi[1] - lo[1]) * W / H))
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        x = mid[0] + (torch.arange(W, device=dev).float() + 0.5 - W / 2) * (2 * half / W)
        y = mid[1] + (torch.arange(H, device=dev).float() + 0.5 - H / 2) * (2 * half / W)
        pts = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.full((H, W), float(mid[2]), device=dev)], dim=2).reshape(n, 3).contiguous()
        sdist = torch.empty(n, dtype=torch.float32, device=dev)
        inside = torch.empty(n, dtype=torch.uint8, device=dev)
        ds.signed_points_device(n, pts.data_ptr(), stream=side.cuda_stream, sdist=sdist.data_ptr(), inside=inside.data_ptr())
        dist = sdist.abs() / half
        shade = 1.0 - 0.7 * dist.clamp(max=1.0)
        band = ((dist / BAND).floor() % 2 == 0).float() * 0.15
        grey = (shade - band).clamp(0.0, 1.0)
        warm = torch.stack([0.5 * grey + 0.5, 0.7 * grey, 0.4 * grey], dim=1)
        cold = torch.stack([0.5 * grey, 0.7 * grey, 0.6 * grey + 0.4], dim=1)
        rgb = torch.where((sdist < 0)[:, None], warm, cold)
        rgb = torch.where((dist < 0.004)[:, None], torch.ones_like(rgb), rgb)
        rgb8 = (rgb * 255.0 + 0.5).to(torch.uint8)
    side.synchronize()
    write_bmp(out, rgb8.cpu().numpy().reshape(H, W, 3))                     # (rows run along +y, as a rendered frame's do)
    print(f"{out}: {W}x{H} points in the plane z = {mid[2]:.3g} of a closed mesh of {flat.n_tris} triangles, {int(inside.sum())} of them inside; "
          f"signed distance from {float(sdist.min()):.4g} to {float(sdist.max()):.4g}")
    ds.close()


if __name__ == "__main__":
    main()
