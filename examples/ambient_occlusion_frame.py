#!/usr/bin/env python3
"""Ambient occlusion as a pass over a rendered frame WITHOUT a ray array (include/srt.h, "Ambient occlusion in a frame"), on device
tensors.  The ground_bunny frame is rendered once (srt_render_device: hit_id, t); those hits go to srt_render_ao_hits_device with the
frame's own params -- the call makes the pixels' rays itself, so nothing is built in torch -- and with a 4 x 4 table of rotations
(lib.ao_rotations): the pixel at (x, y) turns the 16-direction table by entry (y % 4, x % 4), which turns the banding a small fixed table
shows into noise of period 4, and a 4 x 4 box blur of `ao` removes that noise.  Written: the blurred ao as a grey image, white = open.
The example also takes the call's own ao8 bytes (unblurred) and the bent normal, and prints how far the blur moves the picture from the
unrotated one.
Usage: python examples/ambient_occlusion_frame.py [out.bmp [width height [n_dirs [radius]]]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import write_bmp                   # noqa: E402

T_MIN = 1e-3                                    # keeps an AO ray off the triangle it starts on
TILE = 4


def box_blur(img, k):
    """The mean over k x k pixels around each pixel of a [H, W] tensor, edges replicated."""
    x = torch.nn.functional.pad(img[None, None], (k // 2, k - 1 - k // 2, k // 2, k - 1 - k // 2), mode="replicate")
    return torch.nn.functional.avg_pool2d(x, k, stride=1)[0, 0]


def main():
    a = sys.argv[1:]
    out = a[0] if a else "ambient_occlusion_frame.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    K = int(a[3]) if len(a) >= 4 else 16
    radius = float(a[4]) if len(a) >= 5 else 60.0
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    p = g.params(W, H, 1, flags=abi.SRT_FLAG_NO_TIMING)
    cur = torch.cuda.current_stream().cuda_stream
    hit = torch.empty((H, W), dtype=torch.int32, device=dev); t = torch.empty((H, W), dtype=torch.float32, device=dev)
    ds.render_device(p, stream=cur, hit_id=hit.data_ptr(), t=t.data_ptr())
    dirs = torch.from_numpy(lib.ao_directions(K)).to(dev)
    rot = torch.from_numpy(lib.ao_rotations(TILE, TILE)).to(dev)
    ao = {k: torch.empty((H, W), dtype=torch.float32, device=dev) for k in ("fixed", "turned")}
    ao8 = torch.empty((H, W), dtype=torch.uint8, device=dev)
    bent = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ds.render_ao_hits_device(p, hit.data_ptr(), t.data_ptr(), dirs.data_ptr(), K, t_min=T_MIN, t_max=radius, stream=cur, ao=ao["fixed"].data_ptr())
    ds.render_ao_hits_device(p, hit.data_ptr(), t.data_ptr(), dirs.data_ptr(), K, rot=rot.data_ptr(), rot_w=TILE, rot_h=TILE, t_min=T_MIN, t_max=radius, stream=cur,
                             ao=ao["turned"].data_ptr(), ao8=ao8.data_ptr(), bent=bent.data_ptr())
    # the same answer from the call that finds the hits itself: a render's hit_id / t are its own
    again = torch.empty((H, W), dtype=torch.float32, device=dev)
    ds.render_ao_device(p, dirs.data_ptr(), K, rot=rot.data_ptr(), rot_w=TILE, rot_h=TILE, t_min=T_MIN, t_max=radius, stream=cur, ao=again.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(again.view(torch.int32), ao["turned"].view(torch.int32))
    assert torch.equal(ao8, (ao["turned"] * 255.0 + 0.5).to(torch.int32).to(torch.uint8))
    smooth = {k: box_blur(v, TILE) for k, v in ao.items()}
    hits = hit >= 0
    levels = lambda v: int(torch.unique((v[hits] * 255.0 + 0.5).to(torch.uint8)).numel())
    up = bent / bent.norm(dim=2, keepdim=True).clamp_min(1e-20)
    print(f"{W}x{H}, {K} directions, radius {radius}: {int(hits.sum())} hits; grey levels over the hits: {levels(ao['fixed'])} with the fixed table, "
          f"{levels(smooth['turned'])} with the {TILE} x {TILE} rotations after the {TILE} x {TILE} blur; mean ao {float(ao['fixed'][hits].mean()):.4f} / "
          f"{float(smooth['turned'][hits].mean()):.4f}; mean bent normal over the hits {[round(float(c), 3) for c in up[hits].mean(dim=0)]}")
    grey = (smooth["turned"].clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).reshape(H, W, 1).expand(H, W, 3)
    write_bmp(out, np.ascontiguousarray(grey.cpu().numpy()))
    raw = os.path.splitext(out)[0] + "_ao8.bmp"      # the call's own bytes, before the blur
    write_bmp(raw, np.ascontiguousarray(ao8.reshape(H, W, 1).expand(H, W, 3).cpu().numpy()))
    print("wrote", out, "and", raw)
    ds.close()


if __name__ == "__main__":
    main()
