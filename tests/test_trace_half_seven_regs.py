"""CPU-only: the register, scratch and LDS figures of the half-tile trace kernel's seven-wave build (k_trace_nq_half<512, true, 7, 16>:
the closest-hit phase's dir[] and best[] laid over the shadow phase's LDS, HalfTileLds in srt_kernels.h), read from the built library's
code object (tools/kernel_regs.py).  Conditions, not measurements: no scratch, and the two limits that fourteen workgroups -- 28
waves -- per CU need at once: 72 VGPRs a wave and nine LDS granules a workgroup."""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# gfx950: a CU has 160 KiB of LDS, allocated in granules of 320 dwords = 1280 B; a SIMD lane has 512 VGPRs, allocated in granules of 8.
#   VGPRs: 14 workgroups x 2 waves = 28 waves per CU = 7 per SIMD, and floor(512 / 7) = 73 rounds down to 72 registers a wave.
#   LDS:   floor(163,840 / 14) = 11,702 B rounds down to nine granules = 11,520 B a workgroup.
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
WORKGROUPS_PER_CU = 14
VGPRS_FOR_SEVEN_WAVES = 72

SEVEN = "k_trace_nq_half<512, true, 7, 16>"


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


def test_seven_wave_build_has_no_scratch(kernels):
    assert figure(kernels, SEVEN, "private_segment_fixed_size") == 0
    assert figure(kernels, SEVEN, "vgpr_spill_count") == 0


def test_seven_wave_build_fits_seven_waves_per_simd(kernels):
    assert figure(kernels, SEVEN, "vgpr_count") <= VGPRS_FOR_SEVEN_WAVES


def test_fourteen_workgroups_fit_a_cus_lds(kernels):
    lds = figure(kernels, SEVEN, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert WORKGROUPS_PER_CU * rounded <= LDS_PER_CU, f"{lds} B of LDS per workgroup ({rounded} allocated): {LDS_PER_CU // rounded} workgroups per CU"
