#!/usr/bin/env python3
"""A mesh that deforms on the device: the K3 scene (bunny on its ground slab), the bunny's welded vertices in a torch tensor, displaced
each frame by a travelling sine computed with torch ops, handed to srt_scene_refit_device -- which derives the triangle records and
refits every box of the hierarchy on the device -- and drawn with srt_render_device.  The tree keeps the shape it was built with, the
triangles their order.  After set-up (the scene, the index buffer, the rest positions) no geometry crosses PCIe: per frame the host
enqueues a few torch kernels, the refit's six launches and the render, all on one stream, and waits once at the end.
Usage: python examples/deform.py [out.bmp [width height [frames]]]     (needs a GPU; the last frame is written)"""
import os, sys, time
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "examples"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from mirror import write_bmp                   # noqa: E402

BUNNY = "./obj/stanford-bunny.obj"
AMPLITUDE, WAVELENGTH = 9.0, 70.0              # scene units: the bunny is about 230 high


def weld(points):
    """(verts n x 4, tri_vertex n_tris x 3): the distinct points of n_tris x 3 x 4, told apart by their bits."""
    u, inv = np.unique(np.ascontiguousarray(points, np.float32).reshape(-1, 4).view(np.uint32), axis=0, return_inverse=True)
    return np.ascontiguousarray(u).view(np.float32), np.ascontiguousarray(inv.reshape(-1, 3), np.uint32)


def main():
    a = sys.argv[1:]
    out = a[0] if a else "deform.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    frames = int(a[3]) if len(a) >= 4 else 48
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    # set-up: the scene, one vertex buffer for all objects (the slab's corners stay where they are), the index buffer
    verts, tri_vertex = weld(flat.tri_points)
    nV = verts.shape[0]
    ds = lib.DeviceScene(flat)
    ds.refit_prepare(tri_vertex, nV)
    moves = np.zeros(nV, bool); moves[tri_vertex[flat.tri_obj == flat.names.index(BUNNY)].reshape(-1)] = True
    rest = torch.from_numpy(verts).to(dev)                          # n_verts x 4, w = 1
    sway = torch.from_numpy(moves.astype(np.float32)).to(dev)
    top, bottom = float(verts[moves, 1].min()), float(verts[moves, 1].max())      # (y points down in the reference's frame)
    p = abi.make_params(W, H, abi.light_staircase(g.light, 2), focal=float(np.float32(400.0 * W / 1920.0)), flags=abi.SRT_FLAG_NO_TIMING)
    rgb8 = torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)
    hit = torch.empty((H, W), dtype=torch.int32, device=dev)
    cur_verts = rest.clone()
    side = torch.cuda.Stream(device=dev)

    def frame(k):
        """Everything on `side`: the wave runs up the bunny, the feet stay on the slab (the displacement grows with the height)."""
        phase = 2.0 * np.pi * k / 24.0
        height = (bottom - rest[:, 1]) / (bottom - top)
        cur_verts[:, 0] = rest[:, 0] + sway * AMPLITUDE * height * torch.sin(2.0 * np.pi * rest[:, 1] / WAVELENGTH + phase)
        ds.refit_device(cur_verts.data_ptr(), stride=4, n_verts=nV, stream=side.cuda_stream)
        ds.render_device(p, stream=side.cuda_stream, hit_id=hit.data_ptr(), rgb8=rgb8.data_ptr())

    with torch.cuda.stream(side):
        frame(0); frame(1)                                          # warm: workspace and lights are allocated, both counter sets used
        side.synchronize()
        t0 = time.perf_counter()
        for k in range(frames):
            frame(k)
        side.synchronize()
        dt = time.perf_counter() - t0
    write_bmp(out, rgb8.cpu().numpy())
    moved = float((cur_verts[:, 0] - rest[:, 0]).abs().max())
    print(f"{out}: {W}x{H}, {frames} frames of {flat.n_tris} triangles ({nV} vertices) deformed, refitted and drawn in {dt * 1e3:.1f} ms "
          f"({dt / frames * 1e3:.3f} ms a frame); the last frame moves a vertex by up to {moved:.2f}, {int((hit >= 0).sum())} pixels on a surface")
    ds.close()


if __name__ == "__main__":
    main()
