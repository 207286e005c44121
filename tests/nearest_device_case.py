"""Run by tests/test_gpu_nearest.py in its own process (torch initialises HIP first): srt_nearest_points_device on torch tensors, every
result against srt_closest_points_device on the same handle and against the yardstick.
`device`: a second stream beside a pending render, no radius and radii, outputs NULL one by one, float-aligned pointers, masks, a shared
handle.
`refit`: srt_scene_refit_device from a tensor, both queries behind it on the same stream, against the yardstick on the moved flat scene.
`graph`: the call captured into a hipGraph and replayed."""
import sys
import numpy as np
import torch

from query_device_common import captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import point_ref as pr
import points_device_case as pc
import refit_ref
import test_gpu_nearest as tn
import test_gpu_points as tp


def setup():
    c = open_case("ground_bunny")
    flat, pts, rad, want = tp.case("ground_bunny")
    ds = lib.DeviceScene(flat)
    pr.same(ds.nearest_points(pts, radius=rad), want, "host form")
    return c, ds, flat, pts, rad, want


def device_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    frame = c.render(ds)
    out, ref = pc.outputs(dev, n), pc.outputs(dev, n)
    for rep in range(2):
        def queries():
            ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs())
        frame.pending_beside(rep, side, queries)
        out.same(want, f"second stream, rep {rep}")
    frame.after()
    # no radius: against srt_closest_points_device on the same stream
    ds.nearest_points_device(n, d_pts.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    ds.closest_points_device(n, d_pts.data_ptr(), stream=side.cuda_stream, **ref.ptrs())
    side.synchronize()
    unbounded = {k: ref.t[k].cpu().numpy() for k in pr.SAME_KEYS}
    assert (unbounded["tri"] >= 0).all()
    out.same(unbounded, "no radius")
    # NULL stream = the scene's own stream; outputs may be NULL one by one; nothing wanted launches nothing
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("tri", "vw")))
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("dist2", "point", "region")))
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr())
    assert ds.nearest_points(pts[:1], radius=rad[:1])["tri"][0] == want["tri"][0]      # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(want, "own stream, outputs in two calls")
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("region",)))
    side.synchronize()
    out.same(want, "one output", untouched=("tri", "dist2", "point", "vw"))
    # points, radii and masks at addresses that are only 4-byte aligned; fewer points than the buffers hold
    ones = torch.full((n,), -1, dtype=torch.int32, device=dev)
    odd_p, odd_r, odd_m = float_aligned(dev, d_pts), float_aligned(dev, d_rad), float_aligned(dev, ones)
    for m in (n, 65, 1):
        o = pc.outputs(dev, m)
        ds.nearest_points_device(m, odd_p.data_ptr(), radius=odd_r.data_ptr(), point_mask=odd_m.data_ptr(), stream=side.cuda_stream, **o.ptrs())
        side.synchronize()
        o.same(pr.first(want, m), f"float-aligned, {m} points, masks of all ones")
    # masks on the device: the bunny hidden from every second point
    om = np.uint32([1, 2])
    ds.set_object_masks(om)
    pm = np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.uint32)
    d_pm, = c.put(pm.view(np.int32))
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    masked = pr.closest_points(flat, pts, rad, point_mask=pm, obj_mask=om)
    assert not np.array_equal(masked["tri"], want["tri"])
    out.same(masked, "a mask per point")

    def shared(sh):
        sh.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(masked, "shared handle: the one table")
    through_shared_handle(ds, shared)
    print("nearest device case: ok")


def refit_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    moved = tn.moved_points(flat)
    d_pts, d_rad, d_moved = c.put(pts, rad, moved)
    out, ref = pc.outputs(dev, n), pc.outputs(dev, n)
    ds.refit_prepare()
    ds.refit_device(d_moved.data_ptr(), stride=4, stream=side.cuda_stream)
    ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=True, **out.ptrs())
    side.synchronize()
    w = pr.closest_points(refit_ref.refit_flat(flat, moved), pts, rad)
    assert not np.array_equal(w["dist2"], want["dist2"])
    out.same(w, "after the refit")
    ds.nearest_points_device(n, d_pts.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    ds.closest_points_device(n, d_pts.data_ptr(), stream=side.cuda_stream, **ref.ptrs())
    side.synchronize()
    out.same({k: ref.t[k].cpu().numpy() for k in pr.SAME_KEYS}, "after the refit, no radius")
    pr.same(ds.nearest_points(pts, radius=rad), w, "after the refit, host form")
    print("nearest refit case: ok")


def graph_case():
    c, ds, flat, pts, rad, want = setup()
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    out = pc.outputs(c.dev, n)
    captured(lambda stream: ds.nearest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=stream, **out.ptrs()), out, want, "replay {rep}",
             [(out, ("tri",))])
    print("nearest graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "refit": refit_case, "graph": graph_case}[sys.argv[1]]()
