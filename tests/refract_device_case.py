"""Run by tests/test_gpu_refract.py in its own process (torch initialises HIP first): the _device forms of the refracting path calls on
torch tensors -- a second stream, results equal to the host forms' (which tests/test_gpu_refract.py pins against tests/refract_ref.py on
the same case); a NULL table in the device form is the _masked call; one launch of srt_shade_paths_refract_device and one of
srt_render_paths_refract_device captured into a hipGraph (a single node each) and replayed twice to the eager bits."""
from query_device_common import SHARE, Outputs, captured, float_aligned, open_case, path_spec
from simple_raytracer_amd import lib
import refract_ref as rf
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh

SCENE, DEPTH, FILL = "cubes4_a40", sh.DEPTH, 7
PROBE = ("seg_hit_id",)


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, rays, lights, refl = sp.frame_case(SCENE)
    n = rays.shape[0]
    ior = rf.case_ior(flat)
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl, d_ior = c.put(rays, refl, ior)
    mirror = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN)
    for label, rule in (("no rule", None), ("SELF", sh.SELF)):
        host = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior)
        assert (host["seg_hit_id"][1] != mirror["seg_hit_id"][1]).any() and (host["rgb8"] != mirror["rgb8"]).any()
        out = Outputs(dev, path_spec((n,), DEPTH), FILL)

        def call(r, stream, table=d_ior.data_ptr()):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=rule, ior=table,
                                  **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        call(d_rays, side.cuda_stream, 0); side.synchronize()
        out.same(ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule), f"paths, {label}, a NULL table")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}, replay {{rep}}", [(out, PROBE)])

    for what, kw in (("whole frame", {}), ("tile share", SHARE)):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, rf.BOUNCE_T_MIN, fill=FILL, shadow=sh.SELF, ior=ior)
        out = Outputs(dev, path_spec((ds.rows(fp), ds.cols(fp)), DEPTH), FILL)

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, ior=d_ior.data_ptr(), **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}, replay {{rep}}", [(out, PROBE)])
    ds.close()
    print("refract device case: ok")


if __name__ == "__main__":
    main()
