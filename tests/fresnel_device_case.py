"""Run by tests/test_gpu_fresnel.py in its own process (torch initialises HIP first): the _device forms of the Fresnel path calls on torch
tensors -- a second stream, results equal to the host forms' (which tests/test_gpu_fresnel.py pins against tests/fresnel_ref.py on the
same case), the side rays' rows included; rays at an address that is only float-aligned; a NULL f0 in the device form is the _refract
call and leaves the side rows alone; a handle of srt_scene_share; a render pending on another stream stays untouched; one launch of
srt_shade_paths_fresnel_device and one of srt_render_paths_fresnel_device captured into a hipGraph and replayed twice to the eager bits."""
from query_device_common import SHARE, Outputs, captured, float_aligned, open_case, path_spec, through_shared_handle
from simple_raytracer_amd import lib
import fresnel_ref as fr
import refract_ref as rf
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_query_ref as sq
import shadow_rule_ref as sh

SCENE, DEPTH, FILL = "cubes4_a40", 3, 7
ARG = {"fresnel": "side_fresnel"}              # result key -> argument, where they differ
PROBE = ("seg_hit_id", "side_hit_id")


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, rays, lights, refl = sp.frame_case(SCENE)
    n = rays.shape[0]
    ior, f0 = rf.case_ior(flat), fr.case_f0(flat)
    ds = lib.DeviceScene(flat)
    p = sq.shade_params(lights)
    d_rays, d_refl, d_ior, d_f0 = c.put(rays, refl, ior, f0)
    frame = c.render(ds)
    want_all = sp.ALL_KEYS + fr.SIDE_KEYS
    glass = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, ior=ior)
    for label, rule in (("no rule", None), ("SELF", sh.SELF)):
        host = ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior, fresnel=f0, want=want_all)
        assert (host["side_hit_id"] >= 0).any() and (host["rgb8"] != glass["rgb8"]).any()
        out = Outputs(dev, path_spec((n,), DEPTH, side_rows=True), FILL)

        def call(h, r, stream, table=d_f0.data_ptr()):
            h.shade_paths_device(n, r.data_ptr(), p, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=rule, ior=d_ior.data_ptr(),
                                 fresnel=table, **out.ptrs(ARG))

        call(ds, d_rays, side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, second stream")
        call(ds, float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
        out.same(host, f"paths, {label}, float-aligned rays")
        call(ds, d_rays, side.cuda_stream, 0); side.synchronize()
        out.same(ds.shade_paths(rays, p, DEPTH, refl, rf.BOUNCE_T_MIN, shadow=rule, ior=ior), f"paths, {label}, a NULL f0", untouched=fr.SIDE_KEYS)

        def shared(h):
            call(h, d_rays, side.cuda_stream); side.synchronize()
            out.same(host, f"paths, {label}, shared handle")
        through_shared_handle(ds, shared)
        frame.pending_beside("fresnel paths", side, lambda: call(ds, d_rays, side.cuda_stream))
        out.same(host, f"paths, {label}, beside a pending render")
        frame.after()
        captured(lambda stream: call(ds, d_rays, stream), out, host, f"paths, {label}, replay {{rep}}", [(out, PROBE)])

    for what, kw in (("whole frame", {}), ("tile share", SHARE)):
        fp = rpr.camera_params(SCENE, lights, **kw)
        host = ds.render_paths(fp, DEPTH, refl, rf.BOUNCE_T_MIN, fill=FILL, shadow=sh.SELF, ior=ior, fresnel=f0, want=want_all)
        assert (host["side_hit_id"][rpr.owned(fp)[None].repeat(DEPTH, 0) >= 0] >= 0).any()
        out = Outputs(dev, path_spec((ds.rows(fp), ds.cols(fp)), DEPTH, side_rows=True), FILL)

        def fcall(stream):
            ds.render_paths_device(fp, DEPTH, reflectance=d_refl.data_ptr(), bounce_t_min=rf.BOUNCE_T_MIN, stream=stream, shadow=sh.SELF, ior=d_ior.data_ptr(),
                                   fresnel=d_f0.data_ptr(), **out.ptrs(ARG))

        fcall(side.cuda_stream); side.synchronize()
        out.same(host, f"frame, {what}, second stream")
        captured(fcall, out, host, f"frame, {what}, replay {{rep}}", [(out, PROBE)])
    ds.close()
    print("fresnel device case: ok")


if __name__ == "__main__":
    main()
