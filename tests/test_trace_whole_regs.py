"""CPU-only: the whole-frame trace and shading kernels (k_trace_nq_whole8_spans<384, true, 16, true>, k_shade_tile_whole_spans<INT_SHIN>,
srt_kernels.h) as the built library's code object states them (tools/kernel_regs.py) and as its listing shows them (llvm-objdump).

Conditions.  The trace kernel meets those of tests/test_trace_wave8_regs.py -- at most 64 VGPRs, no VGPR spill, no scratch, at most four
LDS granules: thirty-two workgroups of one wave per CU.  The shading kernel has no more VGPRs and no more scratch than k_shade_tile_spans
of the same library (whose figures tests pin, and which tools/kernel_regs.py --compare shows unchanged: profiles/trace_whole_kernels.txt).

Properties of the listing, pinned as reached (profiles/trace_whole_kernels.txt has them beside the general kernel's):
  scalar-load waits (s_waitcnt with lgkmcnt) before the wave's first LDS write, counted down the listing: at most 3, the goal.  Reached: 2,
    and only the first lies on the path of a launch that is not being captured (the second belongs to the epoch word of a captured one).
  register-to-register v_mov_b32 per triangle test in the triangle loops of both phases: at most 2, the goal.  Reached: at most 1 per
    pair of tests in the closest-hit phase's loops, 0 in the shadow phase's.  (The general kernel: 17 to 21 a test.)
  SGPRs parked in VGPR lanes (v_writelane_b32): the goal was none.  MISSED: 11, against the general kernel's 21; v_readlane_b32 17 against
    65.  Pinned at 11."""
import importlib.util
import os
import re
import subprocess

import pytest

from simple_raytracer_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024
LDS_GRANULE = 1280
WORKGROUPS_PER_CU = 32
VGPRS_FOR_EIGHT_WAVES = 64

TRACE = "k_trace_nq_whole8_spans<384, true, 16, true>"
GENERAL = "k_trace_nq_wave8_spans<384, true, 16, true>"
SHADE = [("k_shade_tile_whole_spans<1>", "k_shade_tile_spans<1>"), ("k_shade_tile_whole_spans<0>", "k_shade_tile_spans<0>")]

WAITS_BEFORE_FIRST_LDS_WRITE = 3
COPIES_PER_TRIANGLE_TEST = 2
PARKED_SGPRS = 11


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    """(kernel name -> registers, kernel name -> listing as (address, opcode, operands, branch target or None))"""
    build.build_all()
    spec = importlib.util.spec_from_file_location("kernel_regs", os.path.join(ROOT, "tools", "kernel_regs.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    d = str(tmp_path_factory.mktemp("co") / "x")
    rows = {r["short"]: r for r in kr.read(build.LIB_HIP, d, False)}
    txt = subprocess.run([os.path.join(kr.LLVM, "llvm-objdump"), "-d", "-C", os.path.join(d, "k.co")], capture_output=True, text=True, check=True).stdout
    listings, cur, base = {}, None, 0
    for line in txt.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            name = m.group(2).replace("void ", "").split("(")[0]
            cur = listings.setdefault(name, []) if name in (TRACE, GENERAL) else None
            base = int(m.group(1), 16)
            continue
        m = re.match(r"\s+(\S+)\s*(.*?)\s*// ([0-9A-F]{12}):", line)
        if cur is None or not m:
            continue
        t = re.search(r"\+0x([0-9a-f]+)>$", line)
        cur.append((int(m.group(3), 16), m.group(1), m.group(2), base + int(t.group(1), 16) if t and m.group(1).startswith(("s_cbranch", "s_branch")) else None))
    return rows, listings


def figure(rows, name, key):
    assert name in rows, f"{name} is not in the library"
    return int(rows[name].get(key, "0"))


def test_the_trace_kernel_fits_thirty_two_one_wave_workgroups_a_cu(code):
    rows, _ = code
    assert figure(rows, TRACE, "vgpr_count") <= VGPRS_FOR_EIGHT_WAVES
    assert figure(rows, TRACE, "vgpr_spill_count") == 0
    assert figure(rows, TRACE, "private_segment_fixed_size") == 0
    lds = figure(rows, TRACE, "group_segment_fixed_size")
    rounded = -(-lds // LDS_GRANULE) * LDS_GRANULE
    assert WORKGROUPS_PER_CU * rounded <= LDS_PER_CU, f"{lds} B of LDS per workgroup ({rounded} allocated)"


@pytest.mark.parametrize("whole,general", SHADE)
def test_the_shading_kernel_needs_no_more_than_the_general_one(code, whole, general):
    rows, _ = code
    assert figure(rows, whole, "vgpr_count") <= figure(rows, general, "vgpr_count")
    assert figure(rows, whole, "private_segment_fixed_size") <= figure(rows, general, "private_segment_fixed_size")
    assert figure(rows, whole, "vgpr_spill_count") <= figure(rows, general, "vgpr_spill_count")


def waits_before_first_lds_write(listing):
    n = 0
    for _, op, args, _ in listing:
        if op.startswith("ds_write"):
            return n
        n += op == "s_waitcnt" and "lgkmcnt" in args
    raise AssertionError("no LDS write in the listing")


def triangle_loops(listing):
    """[(register copies, triangle tests)] of the loops that hold one or two triangle tests.  A loop: a backward branch and its target (the
    pair loops show as a loop of two tests around a loop of one).  A triangle test: the one exact division of ray_triangle,
    v_div_fixup_f32; the loops of the walk around them hold the slab test's exact fallback as well, six divisions in a row, and are
    left out by their count.  A register copy: v_mov_b32 from a VGPR."""
    at = {a: i for i, (a, _, _, _) in enumerate(listing)}
    back = [(at[t], i) for i, (a, _, _, t) in enumerate(listing) if t is not None and t <= a and t in at]
    out = []
    for s, e in back:
        body = listing[s:e + 1]
        tests = sum(op.startswith("v_div_fixup_f32") for _, op, _, _ in body)
        if tests in (1, 2):
            copies = sum(op.startswith("v_mov_b32") and re.match(r"v\d+, v\d+$", args) is not None for _, op, args, _ in body)
            out.append((copies, tests))
    return out


def test_one_batch_of_argument_loads_in_front_of_the_first_lds_write(code):
    _, listings = code
    n, general = waits_before_first_lds_write(listings[TRACE]), waits_before_first_lds_write(listings[GENERAL])
    print(f"scalar-load waits before the first LDS write, down the listing: {n} (general kernel: {general})")
    assert n <= WAITS_BEFORE_FIRST_LDS_WRITE


def test_the_triangle_loops_do_not_copy_their_records(code):
    _, listings = code
    loops, general = triangle_loops(listings[TRACE]), triangle_loops(listings[GENERAL])
    print(f"(register copies, tests) per triangle loop: {loops} (general kernel: {general})")
    assert len(loops) >= 2, "the loops of both phases are found"
    assert max(c / t for c, t in general) >= 15, "the measure sees the general kernel's rotation"
    for copies, tests in loops:
        assert copies <= COPIES_PER_TRIANGLE_TEST * tests, (copies, tests)


def test_sgprs_parked_in_vgpr_lanes(code):
    _, listings = code
    parked = {k: sum(op.startswith("v_writelane_b32") for _, op, _, _ in listings[k]) for k in (TRACE, GENERAL)}
    read = {k: sum(op.startswith("v_readlane_b32") for _, op, _, _ in listings[k]) for k in (TRACE, GENERAL)}
    print(f"v_writelane_b32 / v_readlane_b32: {parked[TRACE]} / {read[TRACE]} (general kernel: {parked[GENERAL]} / {read[GENERAL]})")
    assert parked[TRACE] <= PARKED_SGPRS and parked[TRACE] < parked[GENERAL]
