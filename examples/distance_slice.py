#!/usr/bin/env python3
"""A distance-field slice through the K3 scene (bunny on its ground slab), on torch device tensors: a grid of points in the plane
z = the bunny's middle, srt_closest_points_device for all of them in one launch, and a picture of the unsigned distance to the nearest
surface -- iso-bands every BAND units, darker with distance, the surface itself white; points farther than RADIUS from everything are the
background.  The points are made on the device and the squared distances are turned into the picture there; nothing but the finished
picture goes back through the host.  The radius is what keeps the query fast: it never shrinks during the walk (include/srt_points.h).
A second launch with a point mask of 1 (the ground carries bit 2 only) shows the slice of the bunny alone in the right half.
Usage: python examples/distance_slice.py [out.bmp [width height]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import write_bmp                   # noqa: E402

RADIUS, BAND = 60.0, 10.0


def main():
    a = sys.argv[1:]
    out = a[0] if a else "distance_slice.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    n = W * H
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    ds = lib.DeviceScene(flat)
    ds.set_object_masks(np.uint32([2, 1]))                 # object 0 is the slab, object 1 the bunny
    bunny = np.ascontiguousarray(flat.tri_points, np.float32)[flat.tri_obj == 1][..., :3].reshape(-1, 3)
    lo, hi = bunny.min(0), bunny.max(0)
    mid, half = (lo + hi) / 2, 0.75 * float(max(hi[0] - lo[0], (hi[1] - lo[1]) * W / H))
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        x = mid[0] + (torch.arange(W, device=dev).float() + 0.5 - W / 2) * (2 * half / W)
        y = mid[1] + (torch.arange(H, device=dev).float() + 0.5 - H / 2) * (2 * half / W)
        pts = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.full((H, W), float(mid[2]), device=dev)], dim=2).reshape(n, 3).contiguous()
        rad = torch.full((n,), RADIUS, dtype=torch.float32, device=dev)
        only_bunny = torch.ones(n, dtype=torch.int32, device=dev)
        d2 = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2)]
        tri = torch.empty(n, dtype=torch.int32, device=dev)
        ds.closest_points_device(n, pts.data_ptr(), radius=rad.data_ptr(), stream=side.cuda_stream, tri=tri.data_ptr(), dist2=d2[0].data_ptr())
        ds.closest_points_device(n, pts.data_ptr(), radius=rad.data_ptr(), point_mask=only_bunny.data_ptr(), stream=side.cuda_stream, dist2=d2[1].data_ptr())
        left = (torch.arange(n, device=dev) % W < W // 2)
        dist = torch.sqrt(torch.where(left, d2[0], d2[1]))                 # +inf where nothing lies within RADIUS
        found = torch.isfinite(dist)
        shade = 1.0 - 0.8 * (dist / RADIUS).clamp(max=1.0)
        band = ((dist / BAND).floor() % 2 == 0).float() * 0.15
        grey = torch.where(dist < 0.6, torch.ones_like(dist), (shade - band).clamp(0.0, 1.0))
        rgb = torch.stack([grey, grey, 0.6 * grey + 0.4], dim=1)
        rgb = torch.where(found[:, None], rgb, torch.tensor(abi.REFERENCE_BACKGROUND, dtype=torch.float32, device=dev)[None, :3] / 255.0)
        rgb8 = (rgb * 255.0 + 0.5).to(torch.uint8)
    side.synchronize()
    write_bmp(out, rgb8.cpu().numpy().reshape(H, W, 3))                     # (rows run along +y, as a rendered frame's do)
    on_bunny = int((torch.from_numpy(flat.tri_obj.astype(np.int64)).to(dev)[tri.clamp(min=0).long()][tri >= 0] == 1).sum())
    print(f"{out}: {W}x{H} points in the plane z = {mid[2]:.1f}, {int((tri >= 0).sum())} within {RADIUS:g} of a surface, {on_bunny} of them nearest to the bunny; "
          f"right half: the bunny alone, {int(torch.isfinite(d2[1]).sum())} within {RADIUS:g}")
    ds.close()


if __name__ == "__main__":
    main()
