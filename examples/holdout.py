#!/usr/bin/env python3
"""Visibility masks: the ground_bunny frame of srt_render_paths at depth 2 on a mirror ground, three ways (include/srt.h, "Visibility
masks").  Every object carries one bit of the scene's mask table (srt_scene_set_object_masks: the ground bit 0, the bunny bit 1), and
srt_render_paths_masked walks each ray KIND with a mask of its own -- visibility=(primary, bounce, shadow):
  holdout     the bunny hidden from the camera only: visibility=(~bunny, all, all).  No pixel sees it, the mirror ground still
              reflects it and it still casts its shadow.
  no shadow   the bunny seen and reflected, but left out of the shadow rays: visibility=(all, all, ~bunny).
  off         the bunny switched off for the frame by its OBJECT mask, 0: no upload, no second scene, the triangle ids of the ground unchanged.
The example prints, per frame, how many pixels see the bunny directly and in the mirror, and how many pixels change against the plain frame.
Usage: python examples/holdout.py [width height]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402

CAMERA, TARGET = (-334.0, 52.0, 221.0), (-84.0, 120.0, 241.0)
GROUND, BUNNY = 0, 1
REFLECTANCE = (0.6, 0.0)                        # a mirror ground, a matt bunny
DEPTH, N_LIGHTS = 2, 4
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
    refl = np.float32(REFLECTANCE)
    bit = lambda k: 1 << k
    table = np.uint32([bit(GROUND), bit(BUNNY)])
    no_bunny = ALL & ~bit(BUNNY)
    render = lambda vis: ds.render_paths(p, DEPTH, refl, want=("rgb8", "seg_obj"), visibility=vis)
    frames = {"plain": render(None)}                                     # srt_render_paths: no masks anywhere
    ds.set_object_masks(table)
    frames["holdout"] = render((no_bunny, ALL, ALL))
    frames["no shadow"] = render((ALL, ALL, no_bunny))
    ds.set_object_masks(np.uint32([bit(GROUND), 0]))                     # the bunny off: 8 bytes staged, nothing else touched
    frames["off"] = render((ALL, ALL, ALL))
    ds.set_object_masks(None)
    print(f"{W}x{H}, depth {DEPTH}, {N_LIGHTS} light samples")
    print(f"{'frame':10s} {'see the bunny':>14s} {'in the mirror':>14s} {'pixels changed':>15s}")
    for name, f in frames.items():
        direct, mirrored = int((f["seg_obj"][0] == BUNNY).sum()), int((f["seg_obj"][1] == BUNNY).sum())
        changed = int((f["rgb8"] != frames["plain"]["rgb8"]).any(axis=-1).sum())
        print(f"{name:10s} {direct:14d} {mirrored:14d} {changed:15d}")
    assert (frames["holdout"]["seg_obj"][0] != BUNNY).all() and (frames["off"]["seg_obj"] != BUNNY).all()
    ds.close()


if __name__ == "__main__":
    main()
