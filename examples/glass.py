#!/usr/bin/env python3
"""Refracting paths: the ground_bunny frame of srt_render_paths at depth 4, three ways (include/srt.h, "Refracting paths").  The path
calls take one float per object, ior: an object with ior > 0 is GLASS -- a ray that hits it goes on through the surface, bent by Snell's
law, where it would have been mirrored; reflectance[obj] weights what the next segment brings either way:
  mirror      the bunny as a mirror: srt_render_paths, no table.
  glass       the bunny as glass of index 1.5: ior=(0, 1.5).  Rays enter it, leave it on the far side (or are reflected back inside, when
              they meet the surface too flat) and show the ground behind it.  It still casts its shadow.
  no shadow   the same glass without a bit of vis->shadow (srt_scene_set_object_masks gives the objects their bits): a clear glass that
              lets the light through.
The example prints, per frame, how many paths reach the ground after the bunny (off it, or through it), how many pixels of the ground lie in
the bunny's shadow, and how many pixels change against the mirror frame.
Usage: python examples/glass.py [width height]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402

CAMERA, TARGET = (-334.0, 52.0, 221.0), (-84.0, 120.0, 241.0)
GROUND, BUNNY = 0, 1
REFLECTANCE = (0.0, 0.85)                       # a matt ground; most of what one sees on the bunny is what the next segment brings
IOR = (0.0, 1.5)                                # the ground is opaque, the bunny is glass
DEPTH, N_LIGHTS = 4, 4
ALL = 0xFFFFFFFF


def look_at(origin, target, up=(0.05, 0.1, 1.0)):
    """A camera-mode ray matrix (column-major: right, up, forward, origin)."""
    o = np.asarray(origin, np.float64)
    f = np.asarray(target, np.float64) - o; f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f); r /= np.linalg.norm(r)
    u = np.cross(f, r)
    M = np.zeros((4, 4)); M[0, :3] = r; M[1, :3] = u; M[2, :3] = f; M[3, :3] = o; M[3, 3] = 1.0
    return np.ascontiguousarray(M.reshape(-1), np.float32)


def main():
    a = sys.argv[1:]
    W, H = (int(a[0]), int(a[1])) if len(a) >= 2 else (640, 360)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    p = abi.make_params(W, H, abi.light_staircase(np.float32(g.light), N_LIGHTS), focal=72.0 * W / 64.0, ray_matrix=look_at(CAMERA, TARGET))
    refl, ior = np.float32(REFLECTANCE), np.float32(IOR)
    bit = lambda k: 1 << k
    render = lambda **kw: ds.render_paths(p, DEPTH, refl, want=("rgb8", "seg_obj", "seg_rgb_linear"), **kw)
    frames = {"mirror": render()}                                        # srt_render_paths: every hit bounces
    frames["glass"] = render(ior=ior)                                    # srt_render_paths_refract
    ds.set_object_masks(np.uint32([bit(GROUND), bit(BUNNY)]))
    frames["no shadow"] = render(ior=ior, visibility=(ALL, ALL, ALL & ~bit(BUNNY)))
    ds.set_object_masks(None)
    lit = frames["no shadow"]["seg_rgb_linear"][0]
    print(f"{W}x{H}, depth {DEPTH}, {N_LIGHTS} light samples, ior {IOR}, reflectance {REFLECTANCE}")
    print(f"{'frame':10s} {'bunny, then ground':>18s} {'ground in its shadow':>21s} {'pixels changed':>15s}")
    for name, f in frames.items():
        obj = f["seg_obj"]
        first = obj[0] == BUNNY
        through = np.zeros_like(first)
        inside = first.copy()
        for b in range(1, DEPTH):                                        # a path that stays with the bunny and then reaches the ground
            through |= inside & (obj[b] == GROUND)
            inside &= obj[b] == BUNNY
        shadowed = int(((obj[0] == GROUND) & (f["seg_rgb_linear"][0] != lit).any(axis=-1)).sum())
        changed = int((f["rgb8"] != frames["mirror"]["rgb8"]).any(axis=-1).sum())
        print(f"{name:10s} {int(through.sum()):18d} {shadowed:21d} {changed:15d}")
    glass, clear = frames["glass"], frames["no shadow"]
    assert (glass["seg_obj"] == clear["seg_obj"]).all(), "the shadow mask moved a path"
    assert (glass["rgb8"] != frames["mirror"]["rgb8"]).any() and (clear["rgb8"] != glass["rgb8"]).any()
    ds.close()


if __name__ == "__main__":
    main()
