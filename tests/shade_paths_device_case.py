"""Run by tests/test_gpu_shade_paths.py in its own process (torch initialises HIP first): srt_shade_paths_device on torch tensors -- a
second stream; results equal to the host entry point's (which tests/test_gpu_shade_paths.py pins against tests/shade_path_ref.py on the
same batch); rays and t_range at an address that is only float-aligned; a handle of srt_scene_share; a render beside the call keeps its
pixels, statistics and pipeline string; the single launch captured into a hipGraph and replayed twice to the eager bits."""
import numpy as np

from query_device_common import Outputs, captured, float_aligned, open_case, path_spec, through_shared_handle
from simple_raytracer_amd import lib
import ray_query_ref as rq
import shade_path_ref as sp
import shade_query_ref as sq

SCENE, N, DEPTH, FILL = "cubes4_a40", 257, 3, 7


def main():
    c = open_case(SCENE)
    dev, g, side = c.dev, c.g, c.side
    ds = lib.DeviceScene(g.flat)
    rays = rq.unrelated_rays(g.flat, N)
    lights = sq.lights_for(SCENE, g.light, 3)
    refl = np.float32(sp.REFLECTANCE)
    p = sq.shade_params(lights)
    plain = ds.shade_rays(rays, p)
    tr = np.where((plain["hit_id"] >= 0)[:, None], np.stack([plain["t"] * np.float32(0.5), plain["t"] * np.float32(1.5)], axis=1), np.float32([0.0, np.inf])).astype(np.float32)
    host = ds.shade_paths(rays, p, DEPTH, refl, sp.BOUNCE_T_MIN, t_range=tr)
    assert (host["seg_hit_id"][1] >= 0).sum() > 4
    d_rays, d_tr, d_refl = c.put(rays, tr, refl)
    out = Outputs(dev, path_spec((N,), DEPTH), FILL)
    frame = c.render(ds)

    def call(h, r, t_, stream):
        h.shade_paths_device(N, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sp.BOUNCE_T_MIN, t_range=t_.data_ptr(), stream=stream, **out.ptrs())

    call(ds, d_rays, d_tr, side.cuda_stream); side.synchronize()
    out.same(host, "second stream")
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)
    for r, t_, what in ((odd_rays, d_tr, "float-aligned rays"), (d_rays, odd_tr, "float-aligned t_range"), (odd_rays, odd_tr, "float-aligned rays and t_range")):
        call(ds, r, t_, side.cuda_stream); side.synchronize()
        out.same(host, what)

    def shared(sh):
        call(sh, d_rays, d_tr, side.cuda_stream); side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)

    frame.pending_beside("shade_paths", side, lambda: call(ds, d_rays, d_tr, side.cuda_stream))
    out.same(host, "beside a pending render")
    frame.after()

    # the light table is on the device: the call is one launch, and may be captured
    captured(lambda stream: call(ds, d_rays, d_tr, stream), out, host, "replay {rep}", [(out, ("seg_hit_id",))])
    print("shade paths device case: ok")


if __name__ == "__main__":
    main()
