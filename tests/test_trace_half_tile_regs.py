"""CPU-only: the register, scratch and LDS figures of the fused trace kernel's half-tile form (k_trace_nq_half: two waves of 8x4 pixels
per 8x8 tile), read from the built library's code object (tools/kernel_regs.py).  Conditions, not measurements: no scratch -- a
spilled register's reload is an L2 round trip on the dependent chain of a wave whose lifetime is the kernel's throughput (DESIGN.md
s5) -- and the residency of the build that was measured: twelve workgroups, 24 waves, per CU."""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The residency that was measured ("half tiles"): 12 workgroups of 128 threads per CU.
#   LDS: a gfx950 CU has 160 KiB, allocated in granules of 320 dwords = 1280 B.  12,680 B per workgroup round up to 10 granules =
#        12,800 B, and floor(163,840 / 12,800) = 12 workgroups.  (11 granules, 14,080 B, would admit 11.)
#   VGPRs: a SIMD lane has 512, allocated in granules of 8.  12 workgroups x 2 waves = 24 waves per CU = 6 per SIMD, and
#        floor(512 / 6) = 85 rounds down to 80 registers a wave.
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
VGPRS_PER_SIMD_LANE = 512
VGPR_GRANULE = 8
SIMDS_PER_CU = 4
WAVES_PER_WORKGROUP = 2
WORKGROUPS_PER_CU_MEASURED = 12

HALF = "k_trace_nq_half<512, true, 6, 16>"


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


def test_half_tile_kernel_has_no_scratch(kernels):
    assert figure(kernels, HALF, "private_segment_fixed_size") == 0
    assert figure(kernels, HALF, "vgpr_spill_count") == 0


def test_half_tile_kernel_keeps_the_measured_residency(kernels):
    lds = figure(kernels, HALF, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    by_lds = LDS_PER_CU // rounded
    assert by_lds >= WORKGROUPS_PER_CU_MEASURED, f"{lds} B of LDS per workgroup ({rounded} allocated): {by_lds} workgroups per CU"
    vgprs = -(-figure(kernels, HALF, "vgpr_count") // VGPR_GRANULE) * VGPR_GRANULE
    by_vgprs = (VGPRS_PER_SIMD_LANE // vgprs) * SIMDS_PER_CU // WAVES_PER_WORKGROUP
    assert by_vgprs >= WORKGROUPS_PER_CU_MEASURED, f"{vgprs} VGPRs a wave: {VGPRS_PER_SIMD_LANE // vgprs} waves per SIMD, {by_vgprs} workgroups per CU"
