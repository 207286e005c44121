#!/usr/bin/env python3
"""Pose mode against the rebuilt scene, oracle against oracle (CPU only): for the K3 orbit poses of examples/frame_pipeline.py, how many
pixels of the pose-mode frame -- the tree built at frame 0, moved points, refitted boxes -- differ in rgb8 from the frame of the scene
REBUILT at that pose (what the reference would render).  Reported, not asserted: pose mode's parity statement is about the same flat
scene, and this is the honest number for a user who wants to know what keeping the tree costs in pixels.

    python tools/pose_vs_rebuild.py [--frames 1,4,8,12] [--width 1920] [--height 1080]"""
import argparse, os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, host      # noqa: E402
from oracle import pyoracle                     # noqa: E402
import golden_util as gu                        # noqa: E402
import pose_ref                                 # noqa: E402
import scenes                                   # noqa: E402

T = host.Transformation
LIGHT = [300.0, -600.0, -100.0, 1.0]


def placement(bunny, cube, extra=None):
    om = host.ObjectManager()
    om.add_object("bunny", bunny); om.add_object("cube", cube)
    om.setColor("bunny", (0.9, 0.9, 0.9)); om.setColor("cube", (0.2, 0.7, 0.3))
    om.transformTriangles("bunny", T.scaleObj(1500.0, 1500.0, 1500.0)); om.transformTriangles("bunny", T.rotateObjX(T.radians(180.0)))
    om.transformTriangles("bunny", T.changeObjPosition(20.0, 170.0, 300.0))
    om.transformTriangles("cube", T.scaleObj(400.0, 10.0, 400.0)); om.transformTriangles("cube", T.changeObjPosition(0.0, 130.0, 350.0))
    for name in ("bunny", "cube"):
        if extra is not None:
            om.transformTriangles(name, extra)
        om.createBoundingHierarchy(name)
    return om.flatten()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=lambda v: [int(x) for x in v.split(",")], default=[1, 4, 8, 12])
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    bunny, cube = gu.load_mesh("bunny"), gu.load_mesh("cube")
    flat0 = placement(bunny, cube)
    v0 = scenes.orbit_view_matrix(T, 0.0, 0.0, 0.0, 0.0)
    light_w = T.mul_vec4(v0, LIGHT)
    print(f"K3 orbit, {a.width}x{a.height}, 1 light sample: rgb8 pixels that differ, pose mode (tree of frame 0) against the scene rebuilt at the pose")
    for f in a.frames:
        inv = T.inverse(scenes.orbit_view_matrix(T, 0.0, 0.5 * f, 0.0, 0.0))
        m = T.mul(inv, v0)
        p = abi.make_params(a.width, a.height, abi.light_staircase(T.mul_vec4(inv, light_w)[:3], 1))
        posed = pyoracle.render(pose_ref.pose_flat(flat0, np.tile(m, (flat0.n_objects, 1))), p, pow="device")
        rebuilt = pyoracle.render(placement(bunny, cube, m), p, pow="device")
        d8 = int(np.any(posed["rgb8"] != rebuilt["rgb8"], axis=-1).sum())
        hit = int(((posed["hit_id"] >= 0) != (rebuilt["hit_id"] >= 0)).sum())
        tt = int((posed["t"].view(np.uint32) != rebuilt["t"].view(np.uint32)).sum())
        print(f"  frame {f:3d} ({0.5 * f:4.1f} deg): {d8} of {a.width * a.height} pixels differ in rgb8; hit / miss differs on {hit}, t bits on {tt}")


if __name__ == "__main__":
    main()
