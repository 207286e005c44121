"""Run by tests/test_gpu_segments.py in its own process (torch initialises HIP first): srt_closest_segments_device on torch tensors.
`device`: a second stream beside a pending render, results equal to the host form's and to the yardstick's, outputs NULL one by one,
float-aligned pointers with fewer segments than the buffers hold, a mask per segment, a shared handle, renders before and after untouched.
`refit`: srt_scene_refit_device from a tensor, the query behind it on the same stream, against the yardstick on the moved flat scene.
`graph`: the call captured into a hipGraph and replayed."""
import sys
import numpy as np
import torch

from query_device_common import QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import refit_ref
import segment_ref as sr
import test_gpu_segments as tg

KEYS = sr.SAME_KEYS


def setup():
    c = open_case("ground_bunny")
    flat, seg, rad, want = tg.case("ground_bunny")
    ds = lib.DeviceScene(flat)
    host = ds.closest_segments(seg, radius=rad, count=True)
    sr.same(host, want, "host form")
    sr.same_counts(host["stats"], want, tg.N, "host form")
    return c, ds, flat, seg, rad, want


def outputs(dev, n):
    spec = {"tri": ((n,), np.int32), "dist2": ((n,), np.float32), "s": ((n,), np.float32), "point": ((n, 3), np.float32), "vw": ((n, 2), np.float32),
            "feature": ((n,), np.uint8)}
    return Outputs(dev, spec, QUERY_FILL)


def device_case():
    c, ds, flat, seg, rad, want = setup()
    dev, side = c.dev, c.side
    n = tg.N
    d_seg, d_rad = c.put(seg, rad)
    frame = c.render(ds)
    out = outputs(dev, n)
    for rep in range(2):
        def queries():
            ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=(rep == 1), **out.ptrs())
        frame.pending_beside(rep, side, queries)
        out.same(want, f"second stream, rep {rep}")
    frame.after()
    # NULL stream = the scene's own stream; outputs may be NULL one by one; nothing wanted launches nothing
    for k in KEYS:
        ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), **out.ptrs(keys=tuple(x for x in KEYS if x != k)))
        torch.cuda.synchronize()
        assert ds.closest_segments(seg[:1], radius=rad[:1])["tri"][0] == want["tri"][0]      # (a host call on the same stream waits for it)
        out.same(want, f"all outputs but {k}", untouched=(k,))
    ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr())
    ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs(keys=("feature",)))
    side.synchronize()
    out.same(want, "one output", untouched=("tri", "dist2", "s", "point", "vw"))
    # segments, radii and masks at addresses that are only 4-byte aligned; fewer segments than the buffers hold
    ones = torch.full((n,), -1, dtype=torch.int32, device=dev)
    odd_s, odd_r, odd_m = float_aligned(dev, d_seg), float_aligned(dev, d_rad), float_aligned(dev, ones)
    for m in (n, 65, 1):
        o = outputs(dev, m)
        ds.closest_segments_device(m, odd_s.data_ptr(), radius=odd_r.data_ptr(), seg_mask=odd_m.data_ptr(), stream=side.cuda_stream, **o.ptrs())
        side.synchronize()
        o.same(sr.first(want, m), f"float-aligned, {m} segments, masks of all ones")
    # masks on the device: the bunny hidden from every second segment
    om = np.uint32([1, 2])
    ds.set_object_masks(om)
    sm = np.where(np.arange(n) % 2 == 0, 3, 1).astype(np.uint32)
    d_sm, = c.put(sm.view(np.int32))
    ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), seg_mask=d_sm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    masked = sr.closest_segments(flat, seg, rad, seg_mask=sm, obj_mask=om)
    assert not np.array_equal(masked["tri"], want["tri"])
    out.same(masked, "a mask per segment")
    ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, **out.ptrs())
    side.synchronize()
    out.same(want, "unmasked beside a table")

    def shared(sh):
        sh.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), seg_mask=d_sm.data_ptr(), stream=side.cuda_stream, **out.ptrs())
        side.synchronize()
        out.same(masked, "shared handle: the one table")
    through_shared_handle(ds, shared)
    print("segments device case: ok")


def refit_case():
    c, ds, flat, seg, rad, want = setup()
    dev, side = c.dev, c.side
    n = tg.N
    moved = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4).copy()
    moved[..., 1] += np.float32(6.0) * np.sin(np.float32(0.05) * moved[..., 0])          # no matrix does this
    moved[..., 2] += np.float32(3.0)
    d_seg, d_rad, d_moved = c.put(seg, rad, moved)
    out = outputs(dev, n)
    ds.refit_prepare()
    ds.refit_device(d_moved.data_ptr(), stride=4, stream=side.cuda_stream)
    ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=side.cuda_stream, count=True, **out.ptrs())
    side.synchronize()
    new = refit_ref.refit_flat(flat, moved)
    w = sr.closest_segments(new, seg, rad)
    assert not np.array_equal(w["dist2"], want["dist2"])
    out.same(w, "after the refit")
    host = ds.closest_segments(seg, radius=rad, count=True)
    sr.same(host, w, "after the refit, host form")
    sr.same_counts(host["stats"], w, n, "after the refit, host form")
    print("segments refit case: ok")


def graph_case():
    c, ds, flat, seg, rad, want = setup()
    n = tg.N
    d_seg, d_rad = c.put(seg, rad)
    out = outputs(c.dev, n)
    captured(lambda stream: ds.closest_segments_device(n, d_seg.data_ptr(), radius=d_rad.data_ptr(), stream=stream, **out.ptrs()), out, want, "replay {rep}",
             [(out, ("tri",))])
    print("segments graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "refit": refit_case, "graph": graph_case}[sys.argv[1]]()
