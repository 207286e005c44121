"""Run by tests/test_gpu_signed.py in its own process (torch initialises HIP first): srt_signed_points_device on torch tensors, every
result against the yardstick (tests/sign_ref.py through test_gpu_signed.reference).
`device`: a second stream beside a pending render, the default table and a caller's table on the device, parity, outputs NULL one by
one, containment only, float-aligned pointers, masks, a shared handle.
`refit`: srt_scene_refit_device from a tensor, the call behind it on the same stream, against the yardstick on the moved flat scene.
`graph`: the call captured into a hipGraph and replayed twice."""
import sys
import numpy as np
import torch

from query_device_common import QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
from oracle import pyoracle
import point_ref as pr
import refit_ref
import sign_ref as sg
import test_gpu_nearest as tn
import test_gpu_signed as ts_

N = ts_.N
SIGN = ("sdist", "inside", "winding", "crossings")


def outputs(dev, n, nd):
    spec = {"sdist": ((n,), np.float32), "inside": ((n,), np.uint8), "winding": ((n, nd), np.int32), "crossings": ((n, nd), np.uint32),
            "tri": ((n,), np.int32), "dist2": ((n,), np.float32), "point": ((n, 3), np.float32), "vw": ((n, 2), np.float32), "region": ((n,), np.uint8)}
    return Outputs(dev, spec, QUERY_FILL)


def setup():
    c = open_case("ground_bunny")
    r = ts_.reference("ground_bunny")
    ds = lib.DeviceScene(r.flat)
    want = ts_.wanted(r, N, 3, False)
    sg.same(ds.signed_points(r.pts, radius=r.rad), want, "host form")
    return c, ds, r, want


def device_case():
    c, ds, r, want = setup()
    dev, side = c.dev, c.side
    pts, rad = r.pts, r.rad
    d_pts, d_rad, d_dirs = c.put(pts, rad, ts_.DIRS16)
    frame = c.render(ds)
    out = outputs(dev, N, 3)
    for rep in range(2):
        def queries():
            ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs())
        frame.pending_beside(rep, side, queries)
        out.same(want, f"second stream, rep {rep}")
    frame.after()
    # parity; the caller's table on the device, at 16 and (float-aligned) 2 directions, for the points the yardstick has them for
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), parity=True, stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(ts_.wanted(r, N, 3, True), "parity")
    m = r.most[16]
    odd_d = float_aligned(dev, d_dirs)
    for nd, table in ((16, d_dirs), (2, odd_d)):
        o = outputs(dev, m, nd)
        ds.signed_points_device(m, d_pts.data_ptr(), radius=d_rad.data_ptr(), dirs=table.data_ptr(), n_dirs=nd, stream=side.cuda_stream, **o.ptrs())
        side.synchronize()
        o.same(ts_.wanted(r, m, nd, False), f"{nd} directions from the device")
    # NULL stream = the scene's own stream; outputs NULL one by one; nothing wanted launches nothing; containment only
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("sdist", "winding", "tri", "vw")))
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("inside", "crossings", "dist2", "point", "region")))
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr())
    assert ds.signed_points(pts[:1], radius=rad[:1])["inside"][0] == want["inside"][0]      # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(want, "own stream, outputs in two calls")
    ds.signed_points_device(N, d_pts.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("inside",)))
    side.synchronize()
    out.same(want, "containment only", untouched=tuple(k for k in out.t if k != "inside"))
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=pr.SAME_KEYS))
    side.synchronize()
    out.same(want, "no sign output: srt_nearest_points", untouched=SIGN)
    # points, radii and masks at addresses that are only 4-byte aligned; fewer points than the buffers hold
    ones = torch.full((N,), -1, dtype=torch.int32, device=dev)
    odd_p, odd_r, odd_m = float_aligned(dev, d_pts), float_aligned(dev, d_rad), float_aligned(dev, ones)
    for k in (N, 65, 1):
        o = outputs(dev, k, 3)
        ds.signed_points_device(k, odd_p.data_ptr(), radius=odd_r.data_ptr(), point_mask=odd_m.data_ptr(), stream=side.cuda_stream, **o.ptrs())
        side.synchronize()
        o.same(ts_.wanted(r, k, 3, False), f"float-aligned, {k} points, masks of all ones")
    # masks on the device: the bunny hidden from every second point
    om = np.uint32([1, 2])
    ds.set_object_masks(om)
    pm = np.where(np.arange(N) % 2 == 0, 3, 1).astype(np.uint32)
    d_pm, = c.put(pm.view(np.int32))
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    masked = sg.signed_points(pyoracle, r.flat, pts, rad, point_mask=pm, obj_mask=om, counts=False)
    assert not np.array_equal(masked["crossings"], want["crossings"])
    out.same(masked, "a mask per point")

    def shared(sh):
        sh.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(masked, "shared handle: the one table")
    through_shared_handle(ds, shared)
    print("signed device case: ok")


def refit_case():
    c, ds, r, want = setup()
    side = c.side
    flat, pts, rad = r.flat, r.pts, r.rad
    moved = tn.moved_points(flat)
    d_pts, d_rad, d_moved = c.put(pts, rad, moved)
    out = outputs(c.dev, N, 3)
    ds.refit_prepare()
    ds.refit_device(d_moved.data_ptr(), stride=4, stream=side.cuda_stream)
    ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=True, **out.ptrs())
    side.synchronize()
    w = sg.signed_points(pyoracle, refit_ref.refit_flat(flat, moved), pts, rad, counts=False)
    assert not np.array_equal(w["crossings"], want["crossings"]) and not np.array_equal(w["dist2"], want["dist2"])
    out.same(w, "after the refit")
    sg.same(ds.signed_points(pts, radius=rad), w, "after the refit, host form")
    print("signed refit case: ok")


def graph_case():
    c, ds, r, want = setup()
    d_pts, d_rad = c.put(r.pts, r.rad)
    out = outputs(c.dev, N, 3)
    captured(lambda stream: ds.signed_points_device(N, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=stream, **out.ptrs()), out, want, "replay {rep}",
             [(out, ("inside", "tri"))])
    print("signed graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "refit": refit_case, "graph": graph_case}[sys.argv[1]]()
