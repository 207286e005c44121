"""Run by tests/test_gpu_visibility.py in its own process (torch initialises HIP first): the _device forms of the masked calls on torch
tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_visibility.py pins against tests/visibility_ref.py on
the same cases); rays, t_range and ray_mask at addresses that are only 4-byte aligned; every launch captured into a hipGraph AFTER the
table is set and replayed twice to the eager bits; a table set between two replays is what the next replay reads."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import render_paths_ref as rpr                 # noqa: E402
import shade_query_ref as sq                   # noqa: E402
import shadow_rule_ref as sh                   # noqa: E402
import visibility_ref as vr                    # noqa: E402
from query_device_common import bits, float_aligned      # noqa: E402
from shadow_rule_device_case import Outputs, captured    # noqa: E402

SCENE, DEPTH = "cubes4_a40", vr.DEPTH


def word_aligned(dev, d):
    """The same 4-byte words at an address that is only 4-byte aligned."""
    odd = torch.empty(d.numel() + 1, dtype=d.dtype, device=dev)
    odd[1:].copy_(d.reshape(-1))
    assert odd[1:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    return odd[1:]


def queries(dev, ds, flat, rays, table):
    n = rays.shape[0]
    masks, _ = vr.ray_masks(SCENE, n)
    plain = ds.trace_rays(rays)
    t1 = np.where(plain["hit_id"] >= 0, plain["t"], np.float32(50.0)).astype(np.float32)
    tr = np.stack([t1 * np.float32(0.5), np.where(np.arange(n) % 2 == 0, np.float32(np.inf), t1 * np.float32(1.5))], axis=1).astype(np.float32)
    skip = (np.arange(n) % 5 - 1).astype(np.int32)
    host = ds.trace_rays(rays, t_range=tr, ray_mask=masks)
    occ_host = ds.occluded(rays, skip, t_range=tr, ray_mask=masks)
    assert not np.array_equal(host["hit_id"], ds.trace_rays(rays, t_range=tr)["hit_id"]) and 0 < occ_host.sum() < n
    d_rays, d_tr, d_skip = torch.from_numpy(rays).to(dev), torch.from_numpy(tr).to(dev), torch.from_numpy(skip).to(dev)
    d_masks = torch.from_numpy(masks.view(np.int32)).to(dev)
    hit = torch.full((n,), -5, dtype=torch.int32, device=dev); t = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    bary = torch.full((n, 3), -1.0, dtype=torch.float32, device=dev); occ = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def same(want, want_occ, what):
        assert np.array_equal(hit.cpu().numpy(), want["hit_id"]), (what, "hit ids")
        assert np.array_equal(bits(t.cpu().numpy()), bits(want["t"])), (what, "t")
        assert np.array_equal(bits(bary.cpu().numpy()), bits(want["bary"])), (what, "bary")
        assert np.array_equal(occ.cpu().numpy(), want_occ), (what, "occluded")
        hit.fill_(-5); t.fill_(-1.0); bary.fill_(-1.0); occ.fill_(7)
        torch.cuda.synchronize()

    def both(r, tr_, m, stream, count=False):
        ds.trace_rays_device(n, r.data_ptr(), stream=stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), count=count, t_range=tr_.data_ptr(),
                             ray_mask=m.data_ptr())
        ds.occluded_device(n, r.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=stream, t_range=tr_.data_ptr(), ray_mask=m.data_ptr())

    for count in (False, True):
        both(d_rays, d_tr, d_masks, side.cuda_stream, count); side.synchronize()
        same(host, occ_host, f"second stream, counting {count}")
    both(float_aligned(dev, d_rays), word_aligned(dev, d_tr), word_aligned(dev, d_masks), side.cuda_stream); side.synchronize()
    same(host, occ_host, "rays, t_range and ray_mask only 4-byte aligned")
    # a NULL ray_mask and a NULL t_range in the device form
    ds.trace_rays_device(n, d_rays.data_ptr(), stream=side.cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), bary=bary.data_ptr(), ray_mask=0)
    ds.occluded_device(n, d_rays.data_ptr(), occ.data_ptr(), skip_obj=d_skip.data_ptr(), stream=side.cuda_stream, ray_mask=0); side.synchronize()
    same(plain, ds.occluded(rays, skip), "NULL ray_mask, table of one bit per object")
    # captured after the table is set; the table is read when the kernel runs
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        both(d_rays, d_tr, d_masks, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (hit.cpu().numpy() == -5).all() and (occ.cpu().numpy() == 7).all(), "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        same(host, occ_host, f"replay {rep}")
    ds.set_object_masks(None)
    now, now_occ = ds.trace_rays(rays, t_range=tr, ray_mask=masks), ds.occluded(rays, skip, t_range=tr, ray_mask=masks)      # (host calls on the table's stream: it has arrived)
    assert not np.array_equal(now["hit_id"], host["hit_id"])
    gph.replay(); torch.cuda.synchronize()
    same(now, now_occ, "replay after the table changed")
    ds.set_object_masks(table)
    ds.trace_rays(rays[:1])


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    flat, rays, lights, refl = sh.lamp_case(SCENE)
    n = rays.shape[0]
    table = vr.case_table(flat)
    ds = lib.DeviceScene(flat)
    ds.set_object_masks(table)
    queries(dev, ds, flat, rays, table)

    p = sq.shade_params(lights)
    d_rays, d_refl = torch.from_numpy(rays).to(dev), torch.from_numpy(refl).to(dev)
    side = torch.cuda.Stream(device=dev)
    vis = vr.case_vis(SCENE, 0)
    plain = ds.shade_paths(rays, p, DEPTH, refl, vr.BOUNCE_T_MIN)
    for label, rule in (("no rule", None), ("ENDED", sh.ENDED)):
        host = ds.shade_paths(rays, p, DEPTH, refl, vr.BOUNCE_T_MIN, shadow=rule, visibility=vis)
        assert (host["rgb8"] != plain["rgb8"]).any()
        out = Outputs(dev, (n,))

        def call(r, stream):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=vr.BOUNCE_T_MIN, stream=stream, shadow=rule, visibility=vis,
                                  **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}")

    for what, kw in (("whole frame", {}), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=2))):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, vr.BOUNCE_T_MIN, fill=7, shadow=sh.ENDED, visibility=vis)
        out = Outputs(dev, (ds.rows(fp), ds.cols(fp)))

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=vr.BOUNCE_T_MIN, stream=stream, shadow=sh.ENDED, visibility=vis, **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}")
    ds.close()
    print("visibility device case: ok")


if __name__ == "__main__":
    main()
