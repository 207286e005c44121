"""CPU: the yardstick of shaded paths under a shadow rule (tests/shadow_rule_ref.py) against the yardstick it extends, and the input
conditions of every case tests/test_gpu_shadow_rule.py uses.  With rule None, and with each identity interval at flags = 0, it is
shade_path_ref.shade_paths bit for bit; t_min > t_max shadows nothing; every lamp case has an occluder beyond the lamp, a sample the hit
object shadows itself, and a ray the rule changes through a bounce alone.  The last test needs no device: the four new entry points
refuse a NULL handle."""
import ctypes as C

import numpy as np
import pytest

import shade_path_ref as sp
import shadow_rule_ref as sh
from simple_raytracer_amd import abi


def test_rule_none_and_the_identities_are_the_existing_yardstick(oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    want = sp.shade_paths(oracle, flat, rays, lights, sh.DEPTH, refl, sh.BOUNCE_T_MIN)
    sp.assert_same(sh.case_reference(oracle, name, None), want, "rule None")
    for label, rule in sh.IDENTITIES.items():
        sp.assert_same(sh.case_reference(oracle, name, rule), want, label)
    # the one-call form on a thinned batch: the same rows
    thin = np.ascontiguousarray(rays[::11])
    o = sh.shade_paths(oracle, flat, thin, lights, sh.DEPTH, refl, sh.BOUNCE_T_MIN, rule=sh.SELF)
    ref = sh.case_reference(oracle, name, sh.SELF)
    sp.assert_same(o, {k: (v[::11] if k in ("rgb_linear", "rgb8") else v[:, ::11]) for k, v in ref.items()}, "thinned, SELF")


def test_a_reversed_interval_shadows_nothing(oracle):
    name = "cubes4_a40"
    flat, _, _, refl = sh.lamp_case(name)
    segs = sh.case_trace(oracle, name)
    assert any(sh.shadow_bits(flat, s, None).any() for s in segs)
    assert not any(sh.shadow_bits(flat, s, sh.NO_SHADOWS).any() for s in segs)
    lit = sh.shade_paths_of(oracle, flat, segs, sh.DEPTH, None, refl, bits=[np.zeros_like(sh.shadow_bits(flat, s, None)) for s in segs])
    sp.assert_same(sh.case_reference(oracle, name, sh.NO_SHADOWS), lit, "t_min > t_max")


@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_lamp_cases_meet_their_input_conditions(oracle, name):
    flat, *_ = sh.lamp_case(name)
    segs = sh.case_trace(oracle, name)
    sp.condition(sh.case_reference(oracle, name, None))           # the paths are shade_path_ref.FRAMES' own: every segment is reached
    c = sh.conditions(flat, segs, sh.case_reference(oracle, name, None), sh.case_reference(oracle, name, sh.SELF))
    print(name, c)
    assert c["beyond"] > 0, "no sample is shadowed by an occluder beyond the lamp"
    assert c["own"] > 0, "no sample is shadowed by the hit object itself"
    assert c["bounce"] > 0, "the rule changes no pixel through a bounce alone"
    # the two rules of the GPU tests differ from one another and from the reference's rule in the pixels
    a, b, n = (sh.case_reference(oracle, name, r)["rgb8"] for r in (sh.SELF, sh.ENDED, None))
    assert (a != b).any() and (b != n).any()


def test_the_frame_yardstick_at_spp_1_is_the_path_yardstick(oracle):
    """render_paths on a small frame equals shade_paths on that frame's rays, under a rule."""
    import render_paths_ref as rpr
    flat, _, lights, refl = sh.lamp_case("cubes4_a40")
    p = rpr.camera_params("cubes4_a40", lights, 16, 9)
    rays, live = rpr.frame_rays_owned(p)
    assert live.all()
    a = rpr.flat_rows(sh.render_paths(oracle, flat, p, 2, refl, sh.BOUNCE_T_MIN, rule=sh.SELF))
    sp.assert_same(a, sh.shade_paths(oracle, flat, rays.reshape(-1, 6), lights, 2, refl, sh.BOUNCE_T_MIN, rule=sh.SELF), "16 x 9 frame")


def test_the_entry_points_refuse_a_null_handle():
    from simple_raytracer_amd import build, lib
    build.build_all()
    L = lib.load()
    p = abi.make_params(8, 8, abi.light_staircase(np.float32([0.0, 0.0, 0.0]), 1))
    pd = abi.PathDesc(2, 1e-3, None)
    rule = abi.shadow_rule(sh.SELF)
    assert rule.flags == abi.SRT_SHADOW_SELF and abi.shadow_rule(sh.ENDED).flags == 0 and abi.shadow_rule(None) is None
    assert C.sizeof(abi.ShadowRule) == 12
    rays = np.zeros((1, 6), np.float32)
    f32p = C.POINTER(C.c_float)
    for r in (None, C.byref(rule)):
        assert L.srt_shade_paths_shadow(None, 1, rays.ctypes.data_as(f32p), None, C.byref(p), C.byref(pd), r, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_shade_paths_shadow_device(None, 1, rays.ctypes.data, None, C.byref(p), C.byref(pd), r, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_shadow(None, C.byref(p), C.byref(pd), r, None, None, None, None) == abi.SRT_ERR_ARG
        assert L.srt_render_paths_shadow_device(None, C.byref(p), C.byref(pd), r, None, None, None, None) == abi.SRT_ERR_ARG
