"""Run by tests/test_gpu_shadow_rule.py in its own process (torch initialises HIP first): srt_shade_paths_shadow_device and
srt_render_paths_shadow_device on torch tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_shadow_rule.py
pins against tests/shadow_rule_ref.py on the same cases); rays at an address that is only float-aligned; each single launch captured
into a hipGraph and replayed twice to the eager bits."""
from query_device_common import SHARE, Outputs, captured, float_aligned, open_case, path_spec
from simple_raytracer_amd import lib
import render_paths_ref as rpr
import shade_query_ref as sq
import shadow_rule_ref as sh

SCENE, DEPTH, FILL = "cubes4_a40", sh.DEPTH, 7
PROBE = ("seg_hit_id",)


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, rays, lights, refl = sh.lamp_case(SCENE)
    n = rays.shape[0]
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl = c.put(rays, refl)
    plain = ds.shade_paths(rays, p, DEPTH, refl, sh.BOUNCE_T_MIN)
    for label, rule in (("SELF", sh.SELF), ("ENDED", sh.ENDED)):
        host = ds.shade_paths(rays, p, DEPTH, refl, sh.BOUNCE_T_MIN, shadow=rule)
        assert (host["rgb8"] != plain["rgb8"]).any()
        out = Outputs(dev, path_spec((n,), DEPTH), FILL)

        def call(r, stream):
            ds.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sh.BOUNCE_T_MIN, stream=stream, shadow=rule, **out.ptrs())

        call(d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        odd = float_aligned(dev, d_rays)
        call(odd, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        captured(lambda stream: call(d_rays, stream), out, host, f"paths, {label}, replay {{rep}}", [(out, PROBE)])

    for what, kw in (("whole frame", {}), ("tile share", SHARE)):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, sh.BOUNCE_T_MIN, fill=FILL, shadow=sh.SELF)
        out = Outputs(dev, path_spec((ds.rows(fp), ds.cols(fp)), DEPTH), FILL)

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=sh.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, **out.ptrs())

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}, replay {{rep}}", [(out, PROBE)])
    ds.close()
    print("shadow rule device case: ok")


if __name__ == "__main__":
    main()
