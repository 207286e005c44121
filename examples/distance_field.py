#!/usr/bin/env python3
"""An UNBOUNDED distance-field slice through the K3 scene (bunny on its ground slab), on torch device tensors: examples/distance_slice.py
without its RADIUS.  A grid of points in the plane z = the bunny's middle, four times as wide as the bunny, so that most of them are far
from every surface; srt_nearest_points_device for all of them in one launch with no radius chosen -- every point finds its nearest
triangle, and pays for the neighbourhood of the answer: the bound of the walk shrinks to the best distance found so far
(include/srt_nearest.h).  The picture: iso-bands every BAND units, darker with distance, the surface itself white.  The points are made on
the device and the squared distances are turned into the picture there.
Usage: python examples/distance_field.py [out.bmp [width height]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import write_bmp                   # noqa: E402

BAND = 10.0


def main():
    a = sys.argv[1:]
    out = a[0] if a else "distance_field.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    n = W * H
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    flat = gu.GoldenScene("ground_bunny").flat
    ds = lib.DeviceScene(flat)
    bunny = np.ascontiguousarray(flat.tri_points, np.float32)[flat.tri_obj == 1][..., :3].reshape(-1, 3)
    lo, hi = bunny.min(0), bunny.max(0)
    mid, half = (lo + hi) / 2, 2.0 * float(max(hi[0] - lo[0], (hi[1] - lo[1]) * W / H))
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        x = mid[0] + (torch.arange(W, device=dev).float() + 0.5 - W / 2) * (2 * half / W)
        y = mid[1] + (torch.arange(H, device=dev).float() + 0.5 - H / 2) * (2 * half / W)
        pts = torch.stack([x[None, :].expand(H, W), y[:, None].expand(H, W), torch.full((H, W), float(mid[2]), device=dev)], dim=2).reshape(n, 3).contiguous()
        d2 = torch.empty(n, dtype=torch.float32, device=dev)
        tri = torch.empty(n, dtype=torch.int32, device=dev)
        ds.nearest_points_device(n, pts.data_ptr(), stream=side.cuda_stream, tri=tri.data_ptr(), dist2=d2.data_ptr())      # no radius
        dist = torch.sqrt(d2)
        shade = 1.0 - 0.8 * (dist / dist.max()).clamp(max=1.0)
        band = ((dist / BAND).floor() % 2 == 0).float() * 0.15
        grey = torch.where(dist < 0.6, torch.ones_like(dist), (shade - band).clamp(0.0, 1.0))
        rgb8 = (torch.stack([grey, grey, 0.6 * grey + 0.4], dim=1) * 255.0 + 0.5).to(torch.uint8)
    side.synchronize()
    write_bmp(out, rgb8.cpu().numpy().reshape(H, W, 3))                     # (rows run along +y, as a rendered frame's do)
    assert int((tri >= 0).sum()) == n                                      # without a radius every point finds a triangle
    on_bunny = int((torch.from_numpy(flat.tri_obj.astype(np.int64)).to(dev)[tri.long()] == 1).sum())
    st = ds.nearest_points(pts[:: max(1, n // 4096)].cpu().numpy(), count=True, want=())["stats"]
    print(f"{out}: {W}x{H} points in the plane z = {mid[2]:.1f}, every one with its nearest triangle, {on_bunny} of them on the bunny; distances "
          f"{float(dist.min()):.3f} .. {float(dist.max()):.1f}; on a sample of {st['primary_rays']} points {st['tri_tests_primary'] / st['primary_rays']:.0f} "
          f"triangle tests a point of the scene's {flat.n_tris}")
    ds.close()


if __name__ == "__main__":
    main()
