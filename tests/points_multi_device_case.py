"""Run by tests/test_gpu_points_multi.py in its own process (torch initialises HIP first): srt_closest_points_multi_device and
srt_nearest_points_multi_device on torch tensors, against tests/points_multi_ref.py.
`device`: a second stream beside a pending render, outputs NULL, float-aligned pointers, masks, a shared handle, renders untouched.
`refit`: srt_scene_refit_device from a tensor, both forms behind it on the same stream, against the yardstick on the moved flat scene.
`graph`: both calls captured into a hipGraph and replayed twice."""
import sys
import numpy as np
import torch

from query_device_common import QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import points_multi_ref as pm
import refit_ref
import test_gpu_nearest as tn
import test_gpu_points as tp

K = 5      # (the build of 8 slots, three of them unused)


def setup():
    c = open_case("ground_bunny")
    flat, pts, rad, _ = tp.case("ground_bunny")
    want = pm.closest_points_multi(flat, pts, K, rad)
    ds = lib.DeviceScene(flat)
    host = ds.closest_points_multi(pts, K, radius=rad, count=True)
    pm.same(host, want, "host form")
    pm.same_counts(host["stats"], want, tp.N, "host form")
    pm.same(ds.nearest_points_multi(pts, K, radius=rad), want, "host form, nearest")
    return c, ds, flat, pts, rad, want


def outputs(dev, n, k=K, nearest=False):
    spec = {"n_within": ((n,), np.uint32), "n_found": ((n,), np.uint32), "tri": ((n, k), np.int32), "dist2": ((n, k), np.float32),
            "point": ((n, k, 3), np.float32), "vw": ((n, k, 2), np.float32), "region": ((n, k), np.uint8)}
    if nearest:
        del spec["n_within"]
    return Outputs(dev, spec, QUERY_FILL)


def forms(ds, dev, n, k=K):
    """(the _device method, its Outputs) of the closest and of the nearest form."""
    return ((ds.closest_points_multi_device, outputs(dev, n, k)), (ds.nearest_points_multi_device, outputs(dev, n, k, True)))


def device_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    frame = c.render(ds)
    both = forms(ds, dev, n)
    for rep in range(2):
        def queries():
            for call, out in both:
                call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs())
        frame.pending_beside(rep, side, queries)
        for _, out in both:
            out.same(want, f"second stream, rep {rep}")
    frame.after()
    ones = torch.full((n,), -1, dtype=torch.int32, device=dev)
    odd_p, odd_r, odd_m = float_aligned(dev, d_pts), float_aligned(dev, d_rad), float_aligned(dev, ones)
    om = np.uint32([1, 2])
    each = np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.uint32)
    d_each, = c.put(each.view(np.int32))
    masked = pm.closest_points_multi(flat, pts, K, rad, point_mask=each, obj_mask=om)
    assert not np.array_equal(masked["tri"], want["tri"])
    cand = pm.candidates(flat, pts, rad)
    aligned = {(m, k): pm.first(pm.columns(cand, k), m) for m, k in ((n, 16), (65, 4), (1, K))}
    for call, out in both:
        # NULL stream = the scene's own stream; outputs may be NULL; nothing wanted launches nothing
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), **out.ptrs(keys=("n_within", "tri", "vw")))
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), **out.ptrs(keys=("n_found", "dist2", "point", "region")))
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr())
        assert ds.closest_points(pts[:1], radius=rad[:1])["tri"][0] == want["tri"][0, 0]      # (a host call on the same stream waits for it)
        torch.cuda.synchronize()
        out.same(want, "own stream, outputs in two calls")
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("n_found",)))
        side.synchronize()
        out.same(want, "one output", untouched=("n_within", "tri", "dist2", "point", "vw", "region"))
        # points, radii and masks at addresses that are only 4-byte aligned; fewer points than the buffers hold; every slot count
        for (m, k), w in aligned.items():
            o = outputs(dev, m, k, nearest=out is both[1][1])
            call(m, odd_p.data_ptr(), k, radius=odd_r.data_ptr(), point_mask=odd_m.data_ptr(), stream=side.cuda_stream, **o.ptrs())
            side.synchronize()
            o.same(w, f"float-aligned, {m} points, k {k}, masks of all ones")
    # masks on the device: the bunny hidden from every second point
    ds.set_object_masks(om)
    for call, out in both:
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), point_mask=d_each.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(masked, "a mask per point")
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(want, "unmasked beside a table")

    def shared(sh):
        for call, out in forms(sh, dev, n):
            call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), point_mask=d_each.data_ptr(), stream=side.cuda_stream, **out.ptrs())
            side.synchronize()
            out.same(masked, "shared handle: the one table")
    through_shared_handle(ds, shared)
    print("points multi device case: ok")


def refit_case():
    c, ds, flat, pts, rad, want = setup()
    dev, side = c.dev, c.side
    n = tp.N
    moved = tn.moved_points(flat)
    d_pts, d_rad, d_moved = c.put(pts, rad, moved)
    both = forms(ds, dev, n)
    ds.refit_prepare()
    ds.refit_device(d_moved.data_ptr(), stride=4, stream=side.cuda_stream)
    for call, out in both:
        call(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=side.cuda_stream, count=True, **out.ptrs())
    side.synchronize()
    w = pm.closest_points_multi(refit_ref.refit_flat(flat, moved), pts, K, rad)
    assert not np.array_equal(w["dist2"], want["dist2"])
    for _, out in both:
        out.same(w, "after the refit")
    host = ds.closest_points_multi(pts, K, radius=rad, count=True)
    pm.same(host, w, "after the refit, host form")
    pm.same_counts(host["stats"], w, n, "after the refit, host form")
    # no radius: the nearest form's columns are the closest form's, on the device
    (close, out), (near, nout) = both
    close(n, d_pts.data_ptr(), K, stream=side.cuda_stream, **out.ptrs())
    near(n, d_pts.data_ptr(), K, stream=side.cuda_stream, **nout.ptrs())
    side.synchronize()
    unbounded = {key: out.t[key].cpu().numpy().view(out.ty[key]) for key in pm.SAME_KEYS}
    assert (unbounded["n_found"] == K).all() and (unbounded["n_within"] == flat.n_tris).all()
    nout.same(unbounded, "after the refit, no radius")
    print("points multi refit case: ok")


def graph_case():
    c, ds, flat, pts, rad, want = setup()
    n = tp.N
    d_pts, d_rad = c.put(pts, rad)
    (close, out), (near, nout) = forms(ds, c.dev, n)

    def calls(stream):
        close(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=stream, **out.ptrs())
        near(n, d_pts.data_ptr(), K, radius=d_rad.data_ptr(), stream=stream, **nout.ptrs())
    captured(calls, (out, nout), (want, want), ("closest form, replay {rep}", "nearest form, replay {rep}"), [(out, ("tri",)), (nout, ("tri",))])
    print("points multi graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "refit": refit_case, "graph": graph_case}[sys.argv[1]]()
