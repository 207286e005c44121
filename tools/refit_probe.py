#!/usr/bin/env python3
"""What moving a scene's geometry costs on one GPU (DESIGN.md s5 "Refit from device points"): the K3 scene (bunny + ground), in ONE run,
  srt_scene_pose                          the yardstick: one matrix per object, six launches
  srt_scene_refit_device                  direct xyzw (16-byte loads), direct xyz, indexed xyz, indexed xyz with vertex normals
  tensor .cpu() + DeviceScene.update      the only route for vertices in device memory before the refit: device -> host -> records
                                          derived on the host -> upload.  The flat scene's BOXES ARE PRECOMPUTED here (a caller would
                                          have to refit them on the host per frame): the figure favours this route.
The device forms are timed with events on the stream the calls are enqueued on, --reps calls a window, after two warm-up calls of the
same form; the forms alternate within a round; per form the median of --rounds rounds with their minimum and maximum -- the spread the
ratios against pose (same run) are to be read against.  The host route ends in a device synchronise and is timed with the host clock.
Usage: python tools/refit_probe.py [--reps N] [--rounds R]     (needs a GPU)"""
import argparse, dataclasses, os, sys, time
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402
import pose_ref                                # noqa: E402
import refit_ref                               # noqa: E402


def timed(fn, reps, stream):
    """us a call: events on `stream`, the stream the calls are enqueued on."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn(); fn(); stream.synchronize()
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream); stream.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    verts, tv = refit_ref.weld(g.flat)
    nV = verts.shape[0]
    vn = verts[:, :3] - verts[:, :3].mean(0)
    vn = np.ascontiguousarray(vn / np.linalg.norm(vn, axis=1, keepdims=True), np.float32)
    flat = dataclasses.replace(g.flat, tri_normals=refit_ref.expand_normals(vn, tv))
    ds = lib.DeviceScene(flat)
    ds.set_pose_source(); ds.refit_prepare(tv, nV)
    side = torch.cuda.Stream(device=dev)
    cur = side.cuda_stream
    assert cur != 0
    mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1))
    d_p4 = torch.from_numpy(np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 4)).to(dev)      # n_tris x 3 points, xyzw
    d_p3 = d_p4[:, :3].contiguous()
    d_v3 = torch.from_numpy(np.ascontiguousarray(verts[:, :3])).to(dev)
    d_vn = torch.from_numpy(vn).to(dev)
    assert d_p4.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    forms = {
        "srt_scene_pose (yardstick)": lambda: ds.pose(mats, stream=cur),
        "refit direct xyzw": lambda: ds.refit_device(d_p4.data_ptr(), stride=4, stream=cur),
        "refit direct xyz": lambda: ds.refit_device(d_p3.data_ptr(), stride=3, stream=cur),
        "refit indexed xyz": lambda: ds.refit_device(d_v3.data_ptr(), stride=3, n_verts=nV, stream=cur),
        "refit indexed xyz + normals": lambda: ds.refit_device(d_v3.data_ptr(), stride=3, n_verts=nV, normals=d_vn.data_ptr(), stream=cur),
    }
    us = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, fn in forms.items():
            us[k].append(timed(fn, a.reps, side))
    # every form leaves the created scene's records (identity matrices, the scene's own points and normals)
    side.synchronize()
    fresh = lib.DeviceScene(flat)
    refit_ref.same_records(ds.records(), fresh.records(), "the probe's forms")
    # the host route, on a scene of its own (an update discards the preparation): boxes precomputed
    host_ms = []
    for _ in range(a.rounds):
        for rep in range(4):
            t0 = time.perf_counter()
            pts = d_p4.cpu().numpy().reshape(-1, 3, 4)
            fresh.update(dataclasses.replace(flat, tri_points=pts), stream=cur)
            side.synchronize()
            if rep:                                            # (the first of a round warms)
                host_ms.append((time.perf_counter() - t0) * 1e3)
    print(f"K3 ground_bunny: {flat.n_tris} triangles, {flat.n_nodes} nodes, {nV} welded vertices; {a.rounds} rounds of {a.reps} calls, forms alternating; "
          f"{torch.cuda.get_device_name(0)}")
    print(f"{'form':44s} {'median us':>10s} {'min':>9s} {'max':>9s} {'/ pose':>8s}")
    yard = float(np.median(us["srt_scene_pose (yardstick)"]))
    for k, v in us.items():
        print(f"{k:44s} {float(np.median(v)):10.2f} {min(v):9.2f} {max(v):9.2f} {float(np.median(v)) / yard:8.3f}")
    k = ".cpu() + update, BOXES PRECOMPUTED (host clock)"
    print(f"{k:44s} {float(np.median(host_ms)) * 1e3:10.2f} {min(host_ms) * 1e3:9.2f} {max(host_ms) * 1e3:9.2f} {float(np.median(host_ms)) * 1e3 / yard:8.3f}")
    print("pose's own spread (max - min) / median: " f"{(max(us['srt_scene_pose (yardstick)']) - min(us['srt_scene_pose (yardstick)'])) / yard:.3f}")
    ds.close(); fresh.close()


if __name__ == "__main__":
    main()
