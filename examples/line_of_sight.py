#!/usr/bin/env python3
"""Line of sight between pairs of points with srt_occluded_range: the four-cubes scene, sensors on a ring around it and targets in the
gaps between the cubes.  A pair (A, B) is the segment o = A, d = B - A, t in (0, 1): only what lies BETWEEN the two points blocks.
The unbounded srt_occluded answers another question -- is anything on the ray from A through B, at any distance -- and is printed
beside it.  For the blocked pairs srt_trace_rays_range names what stands in the way first, and where.
Usage: python examples/line_of_sight.py [sensors [targets]]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402


def main():
    a = [int(v) for v in sys.argv[1:]]
    n_sensors, n_targets = (a[0] if len(a) > 0 else 8), (a[1] if len(a) > 1 else 6)
    g = gu.GoldenScene("cubes4_a40")
    flat = g.flat
    P = flat.tri_points.reshape(-1, 3, 4)[..., :3].reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    c, r = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    ang = np.linspace(0.0, 2 * np.pi, n_sensors, endpoint=False)
    sensors = (c + r * np.stack([np.cos(ang), 0.3 * np.sin(2 * ang), np.sin(ang)], axis=1)).astype(np.float32)
    targets = (c + np.random.default_rng(4).uniform(-0.12, 0.12, (n_targets, 3)) * (hi - lo)).astype(np.float32)
    A = np.repeat(sensors, n_targets, axis=0)
    B = np.tile(targets, (n_sensors, 1))
    rays = np.concatenate([A, B - A], axis=1).astype(np.float32)
    n = rays.shape[0]
    segment = np.tile(np.float32([0.0, 1.0]), (n, 1))
    ds = lib.DeviceScene(flat)
    blocked = ds.occluded(rays, t_range=segment).astype(bool)
    on_the_ray = ds.occluded(rays).astype(bool)
    first = ds.trace_rays(rays, want=("hit_id", "t"), t_range=segment)
    assert np.array_equal(first["hit_id"] >= 0, blocked)            # a segment is blocked iff something is hit inside it
    print(f"{n_sensors} sensors x {n_targets} targets on {g.name}: {int((~blocked).sum())} of {n} pairs see each other; the unbounded query calls "
          f"{int((~on_the_ray).sum())} free ({int((on_the_ray & ~blocked).sum())} pairs have something BEHIND the target only)")
    print("sensor  " + " ".join(f"t{k:<2d}" for k in range(n_targets)) + "     (. free, # blocked, + free with something behind the target)")
    for s in range(n_sensors):
        row = slice(s * n_targets, (s + 1) * n_targets)
        print(f"{s:6d}  " + " ".join(" # " if b else (" + " if u else " . ") for b, u in zip(blocked[row], on_the_ray[row])))
    for k in np.flatnonzero(blocked)[:5]:
        tri, t = int(first["hit_id"][k]), float(first["t"][k])
        print(f"sensor {k // n_targets} -> target {k % n_targets}: blocked by object {int(flat.tri_obj[tri])} (triangle {tri}) at {t:.3f} of the way, {rays[k, :3] + rays[k, 3:] * np.float32(t)}")


if __name__ == "__main__":
    main()
