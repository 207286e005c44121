#!/usr/bin/env python3
"""Picking with a ray query: load the K3 scene (bunny over a ground slab), trace the ray under one pixel of the reference's camera
and print the object and triangle it hits.  Usage: python examples/pick.py [x y [width height]]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402


def main():
    a = [int(v) for v in sys.argv[1:]]
    W, H = (a[2], a[3]) if len(a) >= 4 else (1920, 1080)
    x, y = (a[0], a[1]) if len(a) >= 2 else (W // 2, H // 2)
    g = gu.GoldenScene("ground_bunny")
    ds = lib.DeviceScene(g.flat)
    # the reference's pixel ray (simple_raytracer.cpp:511-517): from the origin, direction (i, j, focal)
    ray = np.array([[0.0, 0.0, 0.0, x + int(-W / 2), y + int(-H / 2), 400.0]], np.float32)
    o = ds.trace_rays(ray)
    tri, t = int(o["hit_id"][0]), float(o["t"][0])
    if tri < 0:
        print(f"pixel ({x}, {y}) of {W}x{H}: nothing under it")
        return
    obj = int(g.flat.tri_obj[tri])
    point = ray[0, :3] + ray[0, 3:] * np.float32(t)
    print(f"pixel ({x}, {y}) of {W}x{H}: object {obj} ({g.flat.names[obj]}), triangle {tri}, t = {t:.6g}, at {point}, barycentrics {o['bary'][0]}")
    down = np.array([[point[0], point[1] - 1000.0, point[2], 0.0, 1.0, 0.0]], np.float32)      # +y is down in the reference's frame
    print("from 1000 above that point, the way down is", "blocked" if ds.occluded(down)[0] else "free")


if __name__ == "__main__":
    main()
