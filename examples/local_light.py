#!/usr/bin/env python3
"""A lamp INSIDE the scene: the four-cubes scene with a lamp in the gap between the cubes, rendered by srt_render_paths at depth 2, once
with the reference's shadow rule and once under a shadow rule (include/srt.h, "Shadow rays with an end").
The reference's shadow ray runs from the hit point towards the light with t unbounded and leaves the hit object's own tree out.  With a
lamp between objects that gives two wrong pictures: a cube on the FAR side of the lamp darkens the cube on the near side (the ray runs
on past the lamp and meets it), and the faces of a cube that look away from the lamp are lit through the cube.  shadow=(1e-3, 1.0, False)
ends every shadow ray at the lamp (t = 1 in units of lamp - hit point); shadow=(1e-3, 1.0, True) also walks the hit object's own tree,
from a little off the surface.  The example prints how many pixels each of the two changes.
Usage: python examples/local_light.py [width height]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402

LAMP = (-10.0, 0.0, 110.0)                       # in the gap between the cubes (they fill x -26 .. 26, |y| 5 .. 25, z 76 .. 124)
CAMERA, TARGET = (98.0, -28.0, 10.0), (-9.0, 0.0, 105.0)
REFLECTANCE = (0.6, 0.25, 0.4, 0.8)
DEPTH, N_LIGHTS = 2, 4


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
    g = gu.GoldenScene("cubes4_a40")
    ds = lib.DeviceScene(g.flat)
    p = abi.make_params(W, H, abi.light_staircase(np.float32(LAMP), N_LIGHTS), focal=135.0 * W / 48.0, ray_matrix=look_at(CAMERA, TARGET))
    refl = np.float32(REFLECTANCE)
    frames = {name: ds.render_paths(p, DEPTH, refl, want=("rgb8", "seg_hit_id"), shadow=rule)
              for name, rule in (("reference", None), ("ended", (1e-3, 1.0, False)), ("self", (1e-3, 1.0, True)))}
    seen = int((frames["reference"]["seg_hit_id"][0] >= 0).sum())
    changed = lambda x, y: int((frames[x]["rgb8"] != frames[y]["rgb8"]).any(axis=-1).sum())
    print(f"{W}x{H}, depth {DEPTH}, {N_LIGHTS} lamp samples, {seen} pixels see a cube")
    print(f"shadow rays that end at the lamp:  {changed('reference', 'ended')} pixels changed (occluders beyond the lamp no longer shadow)")
    print(f"... and self-shadowing:            {changed('ended', 'self')} more pixels changed (faces that look away from the lamp)")
    print(f"shadow=(1e-3, 1.0, True) against no rule: {changed('reference', 'self')} pixels changed")
    ds.close()


if __name__ == "__main__":
    main()
