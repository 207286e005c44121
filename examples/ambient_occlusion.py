#!/usr/bin/env python3
"""Ambient occlusion as a pass over a rendered frame (include/srt.h, "Ambient occlusion"), on device tensors.  The ground_bunny frame is
rendered once (srt_render_device: hit_id, t); the frame's own rays and those hits go to srt_ao_hits_device, which walks NO primary ray: per
hit it builds the tangent frame of the normal that faces the ray, turns a table of cosine-distributed directions (lib.ao_directions) into
it and counts the directions blocked within `radius` -- one launch, the AO rays never reach memory.  The image written is the ao value,
(n_dirs - n_occluded) / n_dirs, white = open; a pixel that hit nothing is 1.  With skip_self the bunny's own creases stay white and only
the contact shadow on the ground is left; the example prints both means.
Usage: python examples/ambient_occlusion.py [out.bmp [width height [n_dirs [radius]]]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import write_bmp                   # noqa: E402

T_MIN = 1e-3                                    # keeps an AO ray off the triangle it starts on


def main():
    a = sys.argv[1:]
    out = a[0] if a else "ambient_occlusion.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    K = int(a[3]) if len(a) >= 4 else 32
    radius = float(a[4]) if len(a) >= 5 else 60.0
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    p = g.params(W, H, 1, flags=abi.SRT_FLAG_NO_TIMING)
    cur = torch.cuda.current_stream().cuda_stream
    n = W * H
    hit = torch.empty(n, dtype=torch.int32, device=dev); t = torch.empty(n, dtype=torch.float32, device=dev)
    ds.render_device(p, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr())
    # the frame's rays as srt_render_device makes them without a matrix: origin 0, direction (i, j, focal), truncating -(float)W / 2
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    rays = torch.zeros((H, W, 6), dtype=torch.float32, device=dev)
    rays[..., 3] = (i0 + torch.arange(W, device=dev)).to(torch.float32)[None, :]
    rays[..., 4] = (j0 + torch.arange(H, device=dev)).to(torch.float32)[:, None]
    rays[..., 5] = float(p.focal)
    dirs = torch.from_numpy(lib.ao_directions(K)).to(dev)
    ao = {k: torch.empty(n, dtype=torch.float32, device=dev) for k in ("all", "skip_self")}
    cnt = torch.empty(n, dtype=torch.int32, device=dev)
    ds.ao_hits_device(n, rays.data_ptr(), hit.data_ptr(), t.data_ptr(), dirs.data_ptr(), K, T_MIN, radius, stream=cur, n_occluded=cnt.data_ptr(), ao=ao["all"].data_ptr())
    ds.ao_hits_device(n, rays.data_ptr(), hit.data_ptr(), t.data_ptr(), dirs.data_ptr(), K, T_MIN, radius, skip_self=True, stream=cur, ao=ao["skip_self"].data_ptr())
    # the same answer from the call that finds the hit itself: a render's hit_id / t are srt_trace_rays' bits
    again = torch.empty(n, dtype=torch.float32, device=dev)
    ds.ao_rays_device(n, rays.data_ptr(), dirs.data_ptr(), K, T_MIN, radius, stream=cur, ao=again.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), ao["all"].view(torch.int32))
    hits = hit >= 0
    print(f"{W}x{H}, {K} directions, radius {radius}: {int(hits.sum())} hits, {int((cnt > 0).sum())} with a blocked direction; "
          f"mean ao over the hits {float(ao['all'][hits].mean()):.4f}, with skip_self {float(ao['skip_self'][hits].mean()):.4f}")
    grey = (ao["all"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).reshape(H, W, 1).expand(H, W, 3)
    write_bmp(out, np.ascontiguousarray(grey.cpu().numpy()))
    print("wrote", out)
    ds.close()


if __name__ == "__main__":
    main()
