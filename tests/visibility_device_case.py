"""Run by tests/test_gpu_visibility.py in its own process (torch initialises HIP first): the _device forms of the masked calls on torch
tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_visibility.py pins against tests/visibility_ref.py on
the same cases); rays, t_range and ray_mask at addresses that are only 4-byte aligned; every launch captured into a hipGraph AFTER the
table is set and replayed twice to the eager bits; a table set between two replays is what the next replay reads."""
import numpy as np
import torch

from query_device_common import QUERY_FILL, SHARE, Outputs, captured, float_aligned, open_case, path_spec
from simple_raytracer_amd import lib
import render_paths_ref as rpr
import shade_query_ref as sq
import shadow_rule_ref as sh
import visibility_ref as vr

SCENE, DEPTH, FILL = "cubes4_a40", vr.DEPTH, 7
PROBE = ("seg_hit_id",)
TRACE = ("hit_id", "t", "bary")


def queries(c, ds, flat, rays, table):
    dev, side = c.dev, c.side
    n = rays.shape[0]
    masks, _ = vr.ray_masks(SCENE, n)
    plain = ds.trace_rays(rays)
    t1 = np.where(plain["hit_id"] >= 0, plain["t"], np.float32(50.0)).astype(np.float32)
    tr = np.stack([t1 * np.float32(0.5), np.where(np.arange(n) % 2 == 0, np.float32(np.inf), t1 * np.float32(1.5))], axis=1).astype(np.float32)
    skip = (np.arange(n) % 5 - 1).astype(np.int32)
    host = dict(ds.trace_rays(rays, t_range=tr, ray_mask=masks), occluded=ds.occluded(rays, skip, t_range=tr, ray_mask=masks))
    assert not np.array_equal(host["hit_id"], ds.trace_rays(rays, t_range=tr)["hit_id"]) and 0 < host["occluded"].sum() < n
    d_rays, d_tr, d_skip, d_masks = c.put(rays, tr, skip, masks.view(np.int32))
    out = Outputs(dev, {"hit_id": ((n,), np.int32), "t": ((n,), np.float32), "bary": ((n, 3), np.float32), "occluded": ((n,), np.uint8)}, QUERY_FILL)

    def both(r, tr_, m, stream, count=False):
        ds.trace_rays_device(n, r.data_ptr(), stream=stream, count=count, t_range=tr_.data_ptr(), ray_mask=m.data_ptr(), **out.ptrs(keys=TRACE))
        ds.occluded_device(n, r.data_ptr(), out.t["occluded"].data_ptr(), skip_obj=d_skip.data_ptr(), stream=stream, t_range=tr_.data_ptr(), ray_mask=m.data_ptr())

    for count in (False, True):
        both(d_rays, d_tr, d_masks, side.cuda_stream, count); side.synchronize()
        out.same(host, f"second stream, counting {count}")
    both(float_aligned(dev, d_rays), float_aligned(dev, d_tr), float_aligned(dev, d_masks), side.cuda_stream); side.synchronize()
    out.same(host, "rays, t_range and ray_mask only 4-byte aligned")
    # a NULL ray_mask and a NULL t_range in the device form
    ds.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, ray_mask=0, **out.ptrs(keys=TRACE))
    ds.occluded_device(n, d_rays.data_ptr(), out.t["occluded"].data_ptr(), skip_obj=d_skip.data_ptr(), stream=side.cuda_stream, ray_mask=0); side.synchronize()
    out.same(dict(plain, occluded=ds.occluded(rays, skip)), "NULL ray_mask, table of one bit per object")
    # captured after the table is set; the table is read when the kernel runs
    gph = captured(lambda stream: both(d_rays, d_tr, d_masks, stream), out, host, "replay {rep}", [(out, ("hit_id", "occluded"))])
    ds.set_object_masks(None)
    now = dict(ds.trace_rays(rays, t_range=tr, ray_mask=masks), occluded=ds.occluded(rays, skip, t_range=tr, ray_mask=masks))      # (host calls on the table's stream: it has arrived)
    assert not np.array_equal(now["hit_id"], host["hit_id"])
    gph.replay(); torch.cuda.synchronize()
    out.same(now, "replay after the table changed")
    ds.set_object_masks(table)
    ds.trace_rays(rays[:1])


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, rays, lights, refl = sh.lamp_case(SCENE)
    n = rays.shape[0]
    table = vr.case_table(flat)
    ds = lib.DeviceScene(flat)
    ds.set_object_masks(table)
    queries(c, ds, flat, rays, table)

    p = sq.shade_params(lights)
    d_rays, d_refl = c.put(rays, refl)
    vis = vr.case_vis(SCENE, 0)
    plain = ds.shade_paths(rays, p, DEPTH, refl, vr.BOUNCE_T_MIN)
    for label, rule in (("no rule", None), ("ENDED", sh.ENDED)):
        host = ds.shade_paths(rays, p, DEPTH, refl, vr.BOUNCE_T_MIN, shadow=rule, visibility=vis)
        assert (host["rgb8"] != plain["rgb8"]).any()
        out = Outputs(dev, path_spec((n,), DEPTH), FILL)

        def call(r, stream):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=vr.BOUNCE_T_MIN, stream=stream, shadow=rule, visibility=vis,
                                  **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}, replay {{rep}}", [(out, PROBE)])

    for what, kw in (("whole frame", {}), ("tile share", SHARE)):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, vr.BOUNCE_T_MIN, fill=FILL, shadow=sh.ENDED, visibility=vis)
        out = Outputs(dev, path_spec((ds.rows(fp), ds.cols(fp)), DEPTH), FILL)

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=vr.BOUNCE_T_MIN, stream=stream, shadow=sh.ENDED, visibility=vis, **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}, replay {{rep}}", [(out, PROBE)])
    ds.close()
    print("visibility device case: ok")


if __name__ == "__main__":
    main()
