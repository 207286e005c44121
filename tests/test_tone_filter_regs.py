"""CPU-only: the register and scratch conditions of the tone map's filter (quant_tone in srt_device.h, called by store_pixel), read from the
built library's code object (tools/kernel_regs.py).  Conditions, not measurements:
  - k_shade_tile<1> and k_shade_tile_batch<1>, built for eight waves per SIMD, stay within 64 VGPRs and without scratch;
  - no kernel that tone-maps gains scratch or drops an occupancy class against the commit before the filter (PARENT below: VGPRs,
    scratch bytes, spilled VGPRs of every kernel whose code the filter changed; profiles/tone_filter_kernels.txt is the full comparison,
    in which every other kernel is byte-identical).
The exact functions are ONE out-of-line function (quant_tone_exact) that these kernels call from a rare loop, so a kernel's VGPR count is
at least that function's, and a kernel that spills already (k_trace_shade_nq: 17 VGPRs, 68 B) has its frame rounded up to the 16-byte
alignment of a frame with a call: 80 B where the parent's metadata said 72, the same 17 spilled registers.  The condition for such a
kernel is therefore on the spill count, and on the scratch size up to that alignment."""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VGPRS_PER_SIMD_LANE = 512      # gfx950; allocated in granules of 8, at most 8 waves per SIMD
EIGHT_WAVES = ("k_shade_tile<1>", "k_shade_tile_batch<1>")

# kernel: (VGPRs, scratch bytes, spilled VGPRs) at the parent commit
PARENT = {
    "k_resolve": (34, 0, 0), "k_shade<true>": (125, 0, 0), "k_shade<false>": (121, 0, 0), "k_trace_shade_nq<512, true, 6, 16, false>": (80, 72, 17),
    "k_shade_tile<1>": (44, 0, 0), "k_shade_tile<0>": (101, 0, 0), "k_shade_tile_batch<1>": (42, 0, 0), "k_shade_tile_batch<0>": (100, 0, 0),
    "k_query_shade<false, false, false, false>": (121, 0, 0), "k_query_shade<true, false, false, false>": (129, 0, 0),
    "k_query_shade<false, true, false, false>": (121, 0, 0), "k_query_shade<true, true, false, false>": (129, 0, 0),
    "k_query_shade<false, false, true, false>": (94, 0, 0), "k_query_shade<true, false, true, false>": (100, 0, 0),
    "k_query_shade<false, true, true, false>": (94, 0, 0), "k_query_shade<true, true, true, false>": (100, 0, 0),
    "k_query_shade<false, false, false, true>": (121, 0, 0), "k_query_shade<true, false, false, true>": (129, 0, 0),
    "k_query_shade<false, true, false, true>": (121, 0, 0), "k_query_shade<true, true, false, true>": (129, 0, 0),
    "k_query_shade<false, false, true, true>": (94, 0, 0), "k_query_shade<true, false, true, true>": (100, 0, 0),
    "k_query_shade<false, true, true, true>": (94, 0, 0), "k_query_shade<true, true, true, true>": (100, 0, 0),
    "k_query_path<false, false, false>": (209, 0, 0), "k_query_path<true, false, false>": (225, 0, 0),
    "k_query_path<false, true, false>": (211, 0, 0), "k_query_path<true, true, false>": (227, 0, 0), "k_query_path<false, false, true>": (167, 0, 0),
    "k_query_path<true, false, true>": (184, 0, 0), "k_query_path<false, true, true>": (170, 0, 0), "k_query_path<true, true, true>": (187, 0, 0),
    "k_query_path_shadow<false, false, false>": (208, 0, 0), "k_query_path_shadow<true, false, false>": (224, 0, 0),
    "k_query_path_shadow<false, true, false>": (210, 0, 0), "k_query_path_shadow<true, true, false>": (226, 0, 0),
    "k_query_path_shadow<false, false, true>": (167, 0, 0), "k_query_path_shadow<true, false, true>": (183, 0, 0),
    "k_query_path_shadow<false, true, true>": (170, 0, 0), "k_query_path_shadow<true, true, true>": (186, 0, 0),
    "k_query_path_masked<false, false, false>": (209, 0, 0), "k_query_path_masked<true, false, false>": (226, 0, 0),
    "k_query_path_masked<false, true, false>": (211, 0, 0), "k_query_path_masked<true, true, false>": (228, 0, 0),
    "k_query_path_masked<false, false, true>": (168, 0, 0), "k_query_path_masked<true, false, true>": (185, 0, 0),
    "k_query_path_masked<false, true, true>": (171, 0, 0), "k_query_path_masked<true, true, true>": (188, 0, 0),
    "k_query_path_refract<false, false, false>": (209, 0, 0), "k_query_path_refract<true, false, false>": (226, 0, 0),
    "k_query_path_refract<false, true, false>": (210, 0, 0), "k_query_path_refract<true, true, false>": (227, 0, 0),
    "k_query_path_refract<false, false, true>": (168, 0, 0), "k_query_path_refract<true, false, true>": (185, 0, 0),
    "k_query_path_refract<false, true, true>": (168, 0, 0), "k_query_path_refract<true, true, true>": (187, 0, 0),
    "k_query_path_fresnel<false, false, false>": (223, 0, 0), "k_query_path_fresnel<true, false, false>": (240, 0, 0),
    "k_query_path_fresnel<false, true, false>": (224, 0, 0), "k_query_path_fresnel<true, true, false>": (241, 0, 0),
    "k_query_path_fresnel<false, false, true>": (184, 0, 0), "k_query_path_fresnel<true, false, true>": (200, 0, 0),
    "k_query_path_fresnel<false, true, true>": (185, 0, 0), "k_query_path_fresnel<true, true, true>": (201, 0, 0),
    "k_render_path<false, false, false>": (238, 0, 0), "k_render_path<true, false, false>": (254, 0, 0),
    "k_render_path<false, true, false>": (240, 0, 0), "k_render_path<true, true, false>": (258, 0, 0),
    "k_render_path<false, false, true>": (196, 0, 0), "k_render_path<true, false, true>": (212, 0, 0),
    "k_render_path<false, true, true>": (199, 0, 0), "k_render_path<true, true, true>": (215, 0, 0),
    "k_render_path_shadow<false, false, false>": (237, 0, 0), "k_render_path_shadow<true, false, false>": (253, 0, 0),
    "k_render_path_shadow<false, true, false>": (239, 0, 0), "k_render_path_shadow<true, true, false>": (255, 0, 0),
    "k_render_path_shadow<false, false, true>": (195, 0, 0), "k_render_path_shadow<true, false, true>": (211, 0, 0),
    "k_render_path_shadow<false, true, true>": (198, 0, 0), "k_render_path_shadow<true, true, true>": (214, 0, 0),
    "k_render_path_masked<false, false, false>": (238, 0, 0), "k_render_path_masked<true, false, false>": (255, 0, 0),
    "k_render_path_masked<false, true, false>": (240, 0, 0), "k_render_path_masked<true, true, false>": (258, 0, 0),
    "k_render_path_masked<false, false, true>": (197, 0, 0), "k_render_path_masked<true, false, true>": (213, 0, 0),
    "k_render_path_masked<false, true, true>": (200, 0, 0), "k_render_path_masked<true, true, true>": (217, 0, 0),
    "k_render_path_refract<false, false, false>": (239, 0, 0), "k_render_path_refract<true, false, false>": (256, 0, 0),
    "k_render_path_refract<false, true, false>": (240, 0, 0), "k_render_path_refract<true, true, false>": (258, 0, 0),
    "k_render_path_refract<false, false, true>": (198, 0, 0), "k_render_path_refract<true, false, true>": (215, 0, 0),
    "k_render_path_refract<false, true, true>": (199, 0, 0), "k_render_path_refract<true, true, true>": (216, 0, 0),
    "k_render_path_fresnel<false, false, false>": (251, 0, 0), "k_render_path_fresnel<true, false, false>": (266, 0, 0),
    "k_render_path_fresnel<false, true, false>": (252, 0, 0), "k_render_path_fresnel<true, true, false>": (268, 0, 0),
    "k_render_path_fresnel<false, false, true>": (211, 0, 0), "k_render_path_fresnel<true, false, true>": (228, 0, 0),
    "k_render_path_fresnel<false, true, true>": (212, 0, 0), "k_render_path_fresnel<true, true, true>": (229, 0, 0),
}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    build.build_all()
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.read(build.LIB_HIP, str(tmp_path_factory.mktemp("co") / "x"), False)
    return {r["short"]: r for r in rows}


def figure(kernels, name, key):
    assert name in kernels, f"{name} is not in the library"
    return int(kernels[name].get(key, "0"))


def waves_per_simd(vgprs):
    return min(8, VGPRS_PER_SIMD_LANE // (-(-vgprs // 8) * 8))


@pytest.mark.parametrize("name", EIGHT_WAVES)
def test_integer_shininess_shading_kernels_keep_eight_waves_without_scratch(kernels, name):
    assert figure(kernels, name, "vgpr_count") <= 64
    assert figure(kernels, name, "private_segment_fixed_size") == 0
    assert figure(kernels, name, "vgpr_spill_count") == 0


def test_every_kernel_that_tone_maps_is_in_the_library(kernels):
    assert not [k for k in PARENT if k not in kernels]


def test_no_kernel_that_tone_maps_drops_an_occupancy_class(kernels):
    worse = {k: (v, figure(kernels, k, "vgpr_count")) for k, (v, _, _) in PARENT.items() if waves_per_simd(figure(kernels, k, "vgpr_count")) < waves_per_simd(v)}
    assert not worse, worse


def test_no_kernel_that_tone_maps_gains_scratch(kernels):
    worse = {}
    for k, (_, scratch, spills) in PARENT.items():
        now, now_spills = figure(kernels, k, "private_segment_fixed_size"), figure(kernels, k, "vgpr_spill_count")
        if now_spills > spills or now > -(-scratch // 16) * 16:
            worse[k] = ((scratch, spills), (now, now_spills))
    assert not worse, worse
