"""CPU-only: the register, scratch and LDS figures of the kernels that take a frame's tile spans -- k_trace_nq_spans<512, true, 7, 16>,
k_trace_nq_half_spans<512, true, 7, 16>, k_shade_tile_spans<0> and <1> -- read from the built library's code object
(tools/kernel_regs.py).  A whole frame of the fused pipeline runs THESE, not the kernels of the same bodies that the other register
tests pin, so the conditions of the occupancy argument are stated for them too: no scratch, 72 VGPRs for seven waves per SIMD,
and the LDS of the kernels they stand in for; the span lookup may cost SGPRs and nothing else."""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gfx950: a CU has 160 KiB of LDS in granules of 1280 B; a SIMD lane has 512 VGPRs in granules of 8.
#   seven waves per SIMD: floor(512 / 7) = 73 rounds down to 72 registers; eight: 64.
#   half-tile form: fourteen workgroups of two waves per CU, floor(163,840 / 14) = 11,702 B rounds down to nine granules.
#   four-wave form: seven workgroups of four waves per CU, floor(163,840 / 7) = 23,405 B rounds down to eighteen granules.
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
TRACE = {"k_trace_nq_half_spans<512, true, 7, 16>": ("k_trace_nq_half<512, true, 7, 16>", 14),
         "k_trace_nq_spans<512, true, 7, 16>": ("k_trace_nq<false, 512, true, 7, 16, false, false, false, false>", 7)}
SHADE_INT, SHADE_GENERAL = "k_shade_tile_spans<1>", "k_shade_tile_spans<0>"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    build.build_all()
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = kr.read(build.LIB_HIP, str(tmp_path_factory.mktemp("co") / "x"), False)
    return {r["short"]: r for r in rows}


def figure(kernels, name, key):
    assert name in kernels, f"{name} is not in the library: {sorted(k for k in kernels if k.startswith(name.split('<')[0]))}"
    return int(kernels[name].get(key, "0"))


@pytest.mark.parametrize("name", sorted(TRACE) + [SHADE_INT, SHADE_GENERAL])
def test_no_scratch(kernels, name):
    assert figure(kernels, name, "private_segment_fixed_size") == 0
    assert figure(kernels, name, "vgpr_spill_count") == 0


@pytest.mark.parametrize("name", sorted(TRACE))
def test_trace_builds_fit_seven_waves_per_simd(kernels, name):
    assert figure(kernels, name, "vgpr_count") <= 72


@pytest.mark.parametrize("name", sorted(TRACE))
def test_trace_builds_keep_the_lds_and_the_residency_of_the_kernels_they_stand_in_for(kernels, name):
    plain, workgroups = TRACE[name]
    lds = figure(kernels, name, "group_segment_fixed_size")
    assert lds == figure(kernels, plain, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert workgroups * rounded <= LDS_PER_CU, f"{lds} B of LDS per workgroup ({rounded} allocated): {LDS_PER_CU // rounded} workgroups per CU"


def test_integer_shininess_shading_build_fits_eight_waves_per_simd(kernels):
    assert figure(kernels, SHADE_INT, "vgpr_count") <= 64
    assert figure(kernels, SHADE_INT, "group_segment_fixed_size") == figure(kernels, "k_shade_tile<1>", "group_segment_fixed_size")


def test_general_shading_build_keeps_four_waves_per_simd(kernels):
    """k_shade_tile<0> (the general pow's f64 temporaries: about 100 VGPRs) runs at four waves per SIMD: floor(512 / 4) = 128."""
    assert figure(kernels, SHADE_GENERAL, "vgpr_count") <= 128
