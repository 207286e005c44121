"""CPU-only: the register, scratch and LDS figures of the one-wave trace kernel over the tile spans (k_trace_nq_wave8_spans<384, true, 16, XCD_PAIRS>:
the half-tile body compiled without packed f32 operations, for a workgroup of ONE wave that tests the roots of its own 32 rays;
srt_kernels.h), read from the built library's code object (tools/kernel_regs.py).  Conditions, not measurements: no scratch, and the two
limits that thirty-two workgroups -- 32 waves -- per CU need at once: 64 VGPRs a wave and four LDS granules a workgroup.  (Workgroups of
one wave are not under the limit of sixteen per CU that the two-wave form meets; tests/test_gpu_trace_wave8.py asks the runtime.)"""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gfx950: a CU has 160 KiB of LDS, allocated in granules of 320 dwords = 1280 B; a SIMD lane has 512 VGPRs, allocated in granules of 8.
#   VGPRs: 32 workgroups x 1 wave = 32 waves per CU = 8 per SIMD, and 512 / 8 = 64 registers a wave.
#   LDS:   163,840 / 32 = 5,120 B = four granules a workgroup.
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
WORKGROUPS_PER_CU = 32
VGPRS_FOR_EIGHT_WAVES = 64

KERNELS = ["k_trace_nq_wave8_spans<384, true, 16, true>", "k_trace_nq_wave8_spans<384, true, 16, false>"]      # the dispatch order shipped, and variant 32's


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


@pytest.mark.parametrize("name", KERNELS)
def test_one_wave_build_fits_eight_waves_per_simd(kernels, name):
    assert figure(kernels, name, "vgpr_count") <= VGPRS_FOR_EIGHT_WAVES


@pytest.mark.parametrize("name", KERNELS)
def test_one_wave_build_spills_nothing(kernels, name):
    assert figure(kernels, name, "vgpr_spill_count") == 0


@pytest.mark.parametrize("name", KERNELS)
def test_one_wave_build_has_no_scratch(kernels, name):
    assert figure(kernels, name, "private_segment_fixed_size") == 0


@pytest.mark.parametrize("name", KERNELS)
def test_thirty_two_workgroups_fit_a_cus_lds(kernels, name):
    lds = figure(kernels, name, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert WORKGROUPS_PER_CU * rounded <= LDS_PER_CU, f"{lds} B of LDS per workgroup ({rounded} allocated): {LDS_PER_CU // rounded} workgroups per CU"
