#!/usr/bin/env python3
"""examples/mirror_path.py's picture through srt_render_paths_device: the K3 scene (bunny on its ground slab), every pixel's ray followed
through `depth` segments, each hit shaded, the bounces mixed by the objects' reflectance -- with NO ray tensor: a pixel's ray is made on
the device, as a render makes it, so the call takes the frame machinery of a render.  To show that, the frame is rendered a second time as
two block_stride = 2 shares (the deal of a two-GPU split, here both on one device), and the assembled shares must equal the whole frame
bit for bit.
Usage: python examples/mirror_frame.py [out.bmp [width height [depth]]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import display_tone, write_bmp, N_LIGHTS, T_MIN      # noqa: E402
from mirror_device import REFLECTANCE          # noqa: E402

BLOCK_ROWS = 16


def main():
    a = sys.argv[1:]
    out = a[0] if a else "mirror_frame.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    depth = int(a[3]) if len(a) >= 4 else 3
    focal = float(np.float32(400.0 * W / 1920.0))
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    lights = abi.light_staircase(g.light, N_LIGHTS)
    refl = torch.tensor(REFLECTANCE, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)

    def render(p):
        rows, cols = ds.rows(p), ds.cols(p)
        lin = torch.empty((rows, cols, 3), dtype=torch.float32, device=dev)
        hit = torch.empty((depth, rows, cols), dtype=torch.int32, device=dev)
        ds.render_paths_device(p, depth, reflectance=refl.data_ptr(), bounce_t_min=T_MIN, stream=side.cuda_stream, rgb_linear=lin.data_ptr(), seg_hit_id=hit.data_ptr())
        return lin, hit

    with torch.cuda.stream(side):              # torch's own kernels on the stream the calls are enqueued on
        lin, hit = render(abi.make_params(W, H, lights, focal=focal))
        # the same frame as two shares of scanline blocks, assembled by the ownership rule of srt_params
        whole_lin, whole_hit = torch.empty_like(lin), torch.empty_like(hit)
        for first in range(2):
            kw = dict(block_rows=BLOCK_ROWS, block_first=first, block_stride=2)
            s_lin, s_hit = render(abi.make_params(W, H, lights, focal=focal, **kw))
            ys = torch.from_numpy(abi.rows_owned(H, BLOCK_ROWS, first, 2)).to(dev)
            whole_lin[ys], whole_hit[:, ys] = s_lin, s_hit
    side.synchronize()
    assert torch.equal(whole_lin.view(torch.int32), lin.view(torch.int32)) and torch.equal(whole_hit, hit), "the assembled shares differ from the whole frame"
    rgb8 = display_tone(lin.cpu().numpy().reshape(-1, 3))
    rgb8[hit[0].cpu().numpy().reshape(-1) < 0] = np.array(abi.REFERENCE_BACKGROUND, np.uint8)
    write_bmp(out, rgb8.reshape(H, W, 3))
    counts = [int((hit[b] >= 0).sum()) for b in range(min(depth, 3))] + [0] * (3 - min(depth, 3))
    print(f"{out}: {W}x{H}, {counts[0]} pixels on a surface, {counts[1]} mirrored rays see the scene, {counts[2]} see it again after the second bounce; "
          "two block_stride = 2 shares assemble to the same bits")
    ds.close()


if __name__ == "__main__":
    main()
