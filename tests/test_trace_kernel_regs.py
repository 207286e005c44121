"""CPU-only: the register, scratch and LDS figures of the shipped node-queue kernels, read from the built library's code object
(tools/kernel_regs.py).  Conditions, not measurements: the fused trace kernel and its batch form run at seven waves per SIMD (at most
72 VGPRs) WITHOUT scratch -- a spilled register's reload is an L2 round trip on the dependent chain of a wave whose lifetime is the
kernel's throughput -- and seven workgroups of them fit a CU's LDS."""
import importlib.util
import os

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# LDS of a gfx950 CU: 160 KiB; workgroups per CU <= floor(160 KiB / LDS per workgroup).  The allocation is rounded up to the granule the
# compiler's target description gives for a 160 KiB LDS (320 dwords = 1280 bytes); rounding only tightens the condition.  Seven
# workgroups of 256 threads (4 waves each = 28 waves, seven per SIMD) are resident only if seven rounded allocations fit.
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
MAX_VGPRS_7_WAVES = 72          # 512 VGPRs per SIMD lane / 7 waves, in granules of 8

TRACE = "k_trace_nq<false, 512, true, 7, 16, false, false, false, false>"
TRACE_BATCH = "k_trace_nq_batch<512, true, 7, 16, true>"
CLOSEST = "k_closest_hit_nq<false, 512, 2, 2, true, false, false, 7>"
CLOSEST_BATCH = "k_closest_hit_nq_batch<512, true, true>"


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


@pytest.mark.parametrize("name", [TRACE, TRACE_BATCH])
def test_fused_trace_kernels_run_seven_waves_without_scratch(kernels, name):
    assert figure(kernels, name, "private_segment_fixed_size") == 0
    assert figure(kernels, name, "vgpr_spill_count") == 0
    assert figure(kernels, name, "vgpr_count") <= MAX_VGPRS_7_WAVES
    lds = figure(kernels, name, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert 7 * rounded <= LDS_PER_CU, f"{lds} B of LDS per workgroup: seven workgroups need {7 * rounded} of {LDS_PER_CU}"


@pytest.mark.parametrize("name", [CLOSEST, CLOSEST_BATCH])
def test_closest_hit_kernels_keep_their_figures(kernels, name):
    assert figure(kernels, name, "private_segment_fixed_size") == 0
    assert figure(kernels, name, "vgpr_count") <= MAX_VGPRS_7_WAVES
