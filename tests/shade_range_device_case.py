"""Run by tests/test_gpu_shade_range.py in its own process (torch initialises HIP first): srt_shade_rays_range_device on torch tensors.
`device`: a second stream and the scene's own, results equal to the host entry point's (which the tests that call this pin against the
yardstick), a t_range pointer that is only float-aligned, a permuted batch, the identities, two handles of srt_scene_share.
`graph`: the call captured into a hipGraph -- one launch on one stream, the light table already resident -- and replayed."""
import sys
import numpy as np
import torch

from query_device_common import QUERY_FILL, UNBOUNDED, Outputs, bits, captured, float_aligned, open_case, shade_spec, through_shared_handle
from simple_raytracer_amd import abi, lib
import shade_query_ref as sq
import shade_range_ref as sr

N = sr.DEVICE_CASE_N


def setup():
    """The batch of shade_range_ref.device_case_inputs / device_case_intervals and what the host forms give for it."""
    c = open_case(sr.DEVICE_CASE_SCENE)
    ds = lib.DeviceScene(c.g.flat)
    rays, lights = sr.device_case_inputs(c.g.flat)
    p = sq.shade_params(lights)
    plain = ds.shade_rays(rays, p)
    tr = sr.device_case_intervals(plain["hit_id"], plain["t"])
    host = ds.shade_rays(rays, p, t_range=tr)              # (the last host call: its light table is on the device)
    assert not np.array_equal(host["hit_id"], plain["hit_id"]) and (host["hit_id"] >= 0).sum() > N // 4
    assert not np.array_equal(bits(host["rgb_linear"]), bits(plain["rgb_linear"]))
    return c, ds, rays, tr, p, plain, host


def device_case():
    c, ds, rays, tr, p, plain, host = setup()
    dev, g, side = c.dev, c.g, c.side
    d_rays, d_tr = c.put(rays, tr)
    assert d_tr.data_ptr() % 8 == 0
    out = Outputs(dev, shade_spec(N), QUERY_FILL)
    for count in (False, True):
        p.flags = abi.SRT_FLAG_COUNT_WORK if count else 0
        ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        p.flags = 0
        side.synchronize()
        out.same(host, f"second stream, counting {count}")
    # NULL stream = the scene's own stream; outputs may be NULL one by one, and all of them
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr(), **out.ptrs(keys=("hit_id", "rgb8")))
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr(), **out.ptrs(keys=("t", "rgb_linear")))
    ds.shade_rays_device(N, d_rays.data_ptr(), p, t_range=d_tr.data_ptr())
    assert ds.trace_rays(rays[:4])["hit_id"].shape == (4,)     # (a host call on the same stream waits for it)
    torch.cuda.synchronize()
    out.same(host, "own stream")
    odd = float_aligned(dev, d_tr)                             # the same intervals 4 bytes further: the narrow loads
    ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=odd.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "float-aligned t_range")
    odd_rays = float_aligned(dev, d_rays)
    ds.shade_rays_device(N, odd_rays.data_ptr(), p, stream=side.cuda_stream, t_range=odd.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same(host, "float-aligned rays and t_range")
    # a ray's result depends on the ray and its interval alone: the batch in another order
    perm = np.random.default_rng(13).permutation(N)
    d_pr, d_pt = c.put(rays[perm], tr[perm])
    ds.shade_rays_device(N, d_pr.data_ptr(), p, stream=side.cuda_stream, t_range=d_pt.data_ptr(), **out.ptrs())
    side.synchronize()
    out.same({k: host[k][perm] for k in out.t}, "permuted")
    # the identities, device form: a NULL t_range and the three intervals that bound nothing give srt_shade_rays' bytes
    for pair in UNBOUNDED:
        d_id = None if pair is None else c.put(np.tile(np.array(pair, np.float32), (N, 1)))[0]
        ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=None if d_id is None else d_id.data_ptr(), **out.ptrs())
        side.synchronize()
        out.same(plain, f"identity {pair}")

    def shared(sh):                                            # two handles of srt_scene_share, each with its own light table
        sh2 = ds.share()
        other = Outputs(dev, shade_spec(N), QUERY_FILL)
        p2 = sq.shade_params(abi.light_staircase(g.light, 3))
        want2 = ds.shade_rays(rays, p2, t_range=tr)
        assert not np.array_equal(bits(want2["rgb_linear"]), bits(host["rgb_linear"]))
        sh.shade_rays_device(N, d_rays.data_ptr(), p, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs())
        sh2.shade_rays_device(N, d_rays.data_ptr(), p2, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **other.ptrs())
        side.synchronize()
        out.same(host, "shared handle"); other.same(want2, "second shared handle, its own table")
        sh2.close()
    through_shared_handle(ds, shared)
    print("shade range device case: ok")


def graph_case():
    c, ds, rays, tr, p, plain, host = setup()                  # (the host call with p was the last: its table is on the device)
    d_rays, d_tr = c.put(rays, tr)
    out = Outputs(c.dev, shade_spec(N), QUERY_FILL)
    captured(lambda stream: ds.shade_rays_device(N, d_rays.data_ptr(), p, stream=stream, t_range=d_tr.data_ptr(), **out.ptrs()), out, host, "replay {rep}",
             [(out, ("hit_id",))])
    print("shade range graph case: ok")


if __name__ == "__main__":
    {"device": device_case, "graph": graph_case}[sys.argv[1]]()
