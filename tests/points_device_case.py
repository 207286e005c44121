"""Run by tests/test_gpu_points.py in its own process (torch initialises HIP first): srt_closest_points_device on torch tensors.
`device`: a second stream beside a pending render, results equal to the host form's and to the yardstick's, outputs NULL one by one,
float-aligned pointers, a shared handle, masks, renders before and after untouched.
`refit`: srt_scene_refit_device from a tensor, the query behind it on the same stream, against the yardstick on the moved flat scene.
`graph`: the call captured into a hipGraph and replayed."""
import sys
import numpy as np
import torch

from query_device_common import QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import point_ref as pr
import refit_ref
import test_gpu_points as tp

KEYS = pr.SAME_KEYS


def setup():
    c = open_case("ground_bunny")
    flat, pts, rad, want = tp.case("ground_bunny")
    ds = lib.DeviceScene(flat)
    host = ds.closest_points(pts, radius=rad, count=True)
    pr.same(host, want, "host form")
    pr.same_counts(host["stats"], want, tp.N, "host form")
    return c, ds, flat, pts, rad, want


def outputs(dev, n):
    spec = {"tri": ((n,), np.int32), "dist2": ((n,), np.float32), "point": ((n, 3), np.float32), "vw": ((n, 2), np.float32), "region": ((n,), np.uint8)}
    return Outputs(dev, spec, QUERY_FILL)


def device_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    frame = c.render(ds)
    out = outputs(dev, n)
    for rep in range(2):
        def queries():
            ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs())
        frame.pending_beside(rep, side, queries)
        out.same(want, f"second stream, rep {rep}")
    frame.after()
    # NULL stream = the scene's own stream; outputs may be NULL one by one; nothing wanted launches nothing
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("tri", "vw")))
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=("dist2", "point", "region")))
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr())
    assert ds.closest_points(pts[:1], radius=rad[:1])["tri"][0] == want["tri"][0]      # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(want, "own stream, outputs in two calls")
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("region",)))
    side.synchronize()
    out.same(want, "one output", untouched=("tri", "dist2", "point", "vw"))
    # points, radii and masks at addresses that are only 4-byte aligned; fewer points than the buffers hold
    ones = torch.full((n,), -1, dtype=torch.int32, device=dev)
    odd_p, odd_r, odd_m = float_aligned(dev, d_pts), float_aligned(dev, d_rad), float_aligned(dev, ones)
    for m in (n, 65, 1):
        o = outputs(dev, m)
        ds.closest_points_device(m, odd_p.data_ptr(), radius=odd_r.data_ptr(), point_mask=odd_m.data_ptr(), stream=side.cuda_stream, **o.ptrs())
        side.synchronize()
        o.same(pr.first(want, m), f"float-aligned, {m} points, masks of all ones")
    # masks on the device: the bunny hidden from every second point
    om = np.uint32([1, 2])
    ds.set_object_masks(om)
    pm = np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.uint32)
    d_pm, = c.put(pm.view(np.int32))
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    masked = pr.closest_points(flat, pts, rad, point_mask=pm, obj_mask=om)
    assert not np.array_equal(masked["tri"], want["tri"])
    out.same(masked, "a mask per point")
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(want, "unmasked beside a table")

    def shared(sh):
        sh.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), point_mask=d_pm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(masked, "shared handle: the one table")
    through_shared_handle(ds, shared)
    print("points device case: ok")


def refit_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    moved = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4).copy()
    moved[..., 1] += np.float32(6.0) * np.sin(np.float32(0.05) * moved[..., 0])          # no matrix does this
    moved[..., 2] += np.float32(3.0)
    d_pts, d_rad, d_moved = c.put(pts, rad, moved)
    out = outputs(dev, n)
    ds.refit_prepare()
    ds.refit_device(d_moved.data_ptr(), stride=4, stream=side.cuda_stream)
    ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=True, **out.ptrs())
    side.synchronize()
    new = refit_ref.refit_flat(flat, moved)
    w = pr.closest_points(new, pts, rad)
    assert not np.array_equal(w["dist2"], want["dist2"])
    out.same(w, "after the refit")
    host = ds.closest_points(pts, radius=rad, count=True)
    pr.same(host, w, "after the refit, host form")
    pr.same_counts(host["stats"], w, n, "after the refit, host form")
    print("points refit case: ok")


def graph_case():
    c, ds, flat, pts, rad, want = setup()
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    out = outputs(c.dev, n)
    captured(lambda stream: ds.closest_points_device(n, d_pts.data_ptr(), radius=d_rad.data_ptr(), stream=stream, **out.ptrs()), out, want, "replay {rep}",
             [(out, ("tri",))])
    print("points graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "refit": refit_case, "graph": graph_case}[sys.argv[1]]()
