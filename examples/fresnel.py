#!/usr/bin/env python3
"""Fresnel split: the ground_bunny frame of examples/glass.py at depth 4, with and without the split (include/srt.h, "Fresnel split").  In
the refracting paths the whole weight of what follows a glass hit goes through the surface; with one more float per object, f0 -- the
reflectance at normal incidence, lib.schlick_f0(ior) for a dielectric -- the mirrored ray at every glass hit is walked once and shaded
once, and its colour enters the mix with Schlick's weight: about 4 % head-on, almost everything at grazing angles:
  glass       the bunny as glass of index 1.5: ior=(0, 1.5).  It bends light and reflects none.
  fresnel     the same glass with f0 = schlick_f0(ior) = (-1, 0.04): the ground is left alone, the bunny splits.
The example prints how many side rays were walked per segment and how many of them hit something, the range of the weight at the first
hit, and how many pixels the reflection changes.  With an output path it writes both frames side by side as a BMP.
Usage: python examples/fresnel.py [width height [out.bmp]]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
from glass import CAMERA, TARGET, BUNNY, REFLECTANCE, IOR, DEPTH, N_LIGHTS, look_at      # noqa: E402  (the frame of examples/glass.py)


def write_bmp(path, rgb8):
    """A bottom-up 24-bit BMP of an [H, W, 3] uint8 image."""
    h, w, _ = rgb8.shape
    row = (w * 3 + 3) & ~3
    body = np.zeros((h, row), np.uint8)
    body[:, :w * 3] = rgb8[::-1, :, ::-1].reshape(h, w * 3)
    head = b"BM" + np.uint32([54 + row * h, 0, 54, 40]).tobytes() + np.int32([w, h]).tobytes() + np.uint16([1, 24]).tobytes() + np.uint32([0, row * h, 2835, 2835, 0, 0]).tobytes()
    with open(path, "wb") as f:
        f.write(head + body.tobytes())


def main():
    a = sys.argv[1:]
    W, H = (int(a[0]), int(a[1])) if len(a) >= 2 else (640, 360)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    p = abi.make_params(W, H, abi.light_staircase(np.float32(g.light), N_LIGHTS), focal=72.0 * W / 64.0, ray_matrix=look_at(CAMERA, TARGET))
    refl, ior = np.float32(REFLECTANCE), np.float32(IOR)
    f0 = lib.schlick_f0(ior)
    glass = ds.render_paths(p, DEPTH, refl, want=("rgb8", "seg_obj"), ior=ior)                                            # srt_render_paths_refract
    split = ds.render_paths(p, DEPTH, refl, want=("rgb8", "seg_obj", "side_hit_id", "fresnel"), ior=ior, fresnel=f0)      # srt_render_paths_fresnel
    assert (glass["seg_obj"] == split["seg_obj"]).all(), "the split moved a path"
    print(f"{W}x{H}, depth {DEPTH}, {N_LIGHTS} light samples, ior {IOR}, f0 {tuple(float(v) for v in f0)}, reflectance {REFLECTANCE}")
    print(f"{'segment':>8s} {'side rays':>10s} {'that hit':>10s} {'F min':>8s} {'F max':>8s}")
    for b in range(DEPTH):
        F = split["fresnel"][b]
        walked = F > 0
        print(f"{b:8d} {int(walked.sum()):10d} {int((split['side_hit_id'][b] >= 0).sum()):10d} " + (f"{F[walked].min():8.4f} {F[walked].max():8.4f}" if walked.any() else f"{'-':>8s} {'-':>8s}"))
    changed = (glass["rgb8"] != split["rgb8"]).any(axis=-1)
    first = split["seg_obj"][0] == BUNNY
    print(f"pixels the reflection changes: {int(changed.sum())} of {int(first.sum())} that see the bunny first ({int((changed & ~first).sum())} elsewhere)")
    assert changed.any() and not (split["fresnel"][DEPTH - 1] != 0).any()
    if len(a) >= 3:
        write_bmp(a[2], np.concatenate([glass["rgb8"], split["rgb8"]], axis=1))
        print("wrote", a[2], "(left: glass, right: with the split)")
    ds.close()


if __name__ == "__main__":
    main()
