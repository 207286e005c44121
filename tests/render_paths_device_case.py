"""Run by tests/test_gpu_render_paths.py in its own process (torch initialises HIP first): srt_render_paths_device on torch tensors -- a
second stream; results equal to the host entry point's (which tests/test_gpu_render_paths.py pins against the yardstick); a tile share whose
padding keeps the tensors' fill; a handle of srt_scene_share; a render beside the call keeps its pixels, statistics and pipeline string; the
single launch captured into a hipGraph and replayed twice to the eager bits."""
import numpy as np

from query_device_common import Outputs, captured, open_case, path_spec, through_shared_handle
from simple_raytracer_amd import lib
import render_paths_ref as rp
import shade_path_ref as sp
import shade_query_ref as sq

SCENE, DEPTH, FILL = "ground_bunny", 3, 7


def main():
    c = open_case(SCENE)
    dev, g, side = c.dev, c.g, c.side
    ds = lib.DeviceScene(g.flat)
    lights = sq.lights_for(SCENE, g.light, 3)
    refl = np.float32(sp.REFLECTANCE[:2])
    d_refl, = c.put(refl)
    frame = c.render(ds)

    for what, kw in (("whole frame", {}), ("spp 4", dict(spp=4)), ("tile share", dict(block_rows=8, block_cols=8, block_first=1, block_stride=3))):
        p = rp.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(p, DEPTH, refl, sp.BOUNCE_T_MIN, fill=FILL)
        assert (host["seg_hit_id"][1][rp.owned(p) >= 0] >= 0).sum() > 20
        out = Outputs(dev, path_spec((ds.rows(p), ds.cols(p)), DEPTH), FILL)

        def call(h, stream):
            h.render_paths_device(p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sp.BOUNCE_T_MIN, stream=stream, **out.ptrs())

        call(ds, side.cuda_stream); side.synchronize()
        out.same(host, what + ", second stream")

        def shared(sh):
            call(sh, side.cuda_stream); side.synchronize()
            out.same(host, what + ", shared handle")
        through_shared_handle(ds, shared)

        frame.pending_beside("render_paths", side, lambda: call(ds, side.cuda_stream))
        out.same(host, what + ", beside a pending render")
        frame.after()

        # the light table is on the device: the call is one launch, and may be captured
        captured(lambda stream: call(ds, stream), out, host, what + ", replay {rep}", [(out, ("seg_hit_id",))])
    print("render paths device case: ok")


if __name__ == "__main__":
    main()
