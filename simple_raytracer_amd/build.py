"""Builds the product's native code in-tree with hipcc for gfx950 (no JIT cache: the .so files travel
with the repo snapshot to the GPU box).  `python -m simple_raytracer_amd.build` or build_all()."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_HIP = os.path.join(HERE, "libsrt_hip.so")
HIP_SRC = os.path.join(CSRC, "srt_hip.hip")
# What libsrt_hip.so, and every measurement variant of it, is compiled from: the one translation unit and the headers it includes.
HIP_DEPS = [HIP_SRC] + [os.path.join(CSRC, f) for f in ("srt_device.h", "srt_kernels.h", "srt_packet.h", "srt_query.h", "srt_tile_spans.h")] + [os.path.join(HERE, "..", "include", f) for f in ("srt.h", "srt_points.h", "srt_nearest.h", "srt_signed.h", "srt_points_multi.h", "srt_segments.h")]

# -ffp-contract=off is part of the numerical contract: FMA contraction changes hit results
# (SURVEY.md H1).  Correctly rounded f32 divide / sqrt are hipcc defaults and must stay on.
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
               "-Wall", "-Wno-unused-function"]


def hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def build_hip(force=False, verbose=False):
    if not force and not _stale(LIB_HIP, HIP_DEPS):
        return LIB_HIP
    cmd = [hipcc()] + HIPCC_FLAGS + ["-o", LIB_HIP, HIP_SRC]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for libsrt_hip.so")
    if verbose and r.stderr:
        print(r.stderr)
    return LIB_HIP


LIB_HOST = os.path.join(HERE, "libsrt_host.so")
HOST_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-pthread"]
# What libsrt_host.so is compiled from, stated once: srt_host.cpp and srt_jpeg.cpp are the half that needs no GPU (they link without
# libsrt_hip: tools/host_sanitize.py), srt_host_render.cpp calls the C ABI, srt_host_c.cpp is the plain-C face of both.
HOST_DIR = os.path.join(CSRC, "host")
HOST_CPU_SRCS = [os.path.join(HOST_DIR, f) for f in ("srt_host.cpp", "srt_jpeg.cpp")]
HOST_SRCS = HOST_CPU_SRCS + [os.path.join(HOST_DIR, f) for f in ("srt_host_render.cpp", "srt_host_c.cpp")]
HOST_DEPS = HOST_SRCS + [os.path.join(HOST_DIR, f) for f in ("srt_host.h", "srt_host_internal.h", "srt_host_c.h")] + [os.path.join(HERE, "..", "include", f) for f in ("srt.h", "srt_points.h", "srt_nearest.h", "srt_signed.h", "srt_points_multi.h", "srt_segments.h")]


def build_host(force=False, verbose=False):
    """Host-side C++ mirror of the reference's scene interface (g++); links the HIP library for the
    drop-in sendRaysAndIntersectPointsColors."""
    if not force and not _stale(LIB_HOST, HOST_DEPS + [LIB_HIP]):
        return LIB_HOST
    cmd = ["g++"] + HOST_FLAGS + ["-o", LIB_HOST] + HOST_SRCS + ["-L" + HERE, "-lsrt_hip", "-Wl,-rpath,$ORIGIN", "-lz"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("g++ failed for libsrt_host.so")
    if verbose and r.stderr:
        print(r.stderr)
    return LIB_HOST


EXAMPLE_ORBIT = os.path.join(HERE, "..", "examples", "orbit")


def build_examples(force=False, verbose=False):
    """examples/orbit: a scene script in the shape of the reference's main(), on the host mirror."""
    src = os.path.join(HERE, "..", "examples", "orbit.cpp")
    if not force and not _stale(EXAMPLE_ORBIT, [src, LIB_HOST]):
        return EXAMPLE_ORBIT
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-o", EXAMPLE_ORBIT, src,
           "-L" + HERE, "-lsrt_host", "-lsrt_hip", "-Wl,-rpath,$ORIGIN/../simple_raytracer_amd"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("g++ failed for examples/orbit")
    return EXAMPLE_ORBIT


EXAMPLE_C = os.path.join(HERE, "..", "examples", "c_abi_minimal")


def build_c_example(force=False, verbose=False):
    """examples/c_abi_minimal: include/srt.h from plain C (gcc), no host mirror."""
    src = os.path.join(HERE, "..", "examples", "c_abi_minimal.c")
    if not force and not _stale(EXAMPLE_C, [src, LIB_HIP, os.path.join(HERE, "..", "include", "srt.h")]):
        return EXAMPLE_C
    cmd = ["gcc", "-O2", "-std=c11", "-Wall", "-Wextra", "-o", EXAMPLE_C, src, "-L" + HERE, "-lsrt_hip", "-Wl,-rpath,$ORIGIN/../simple_raytracer_amd"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("gcc failed for examples/c_abi_minimal")
    return EXAMPLE_C


def stale_artefacts():
    """Names of the product's native artefacts that are missing or older than their sources (nothing is built)."""
    out = []
    if _stale(LIB_HIP, HIP_DEPS):
        out.append("libsrt_hip.so")
    if _stale(LIB_HOST, HOST_DEPS):
        out.append("libsrt_host.so")
    return out


def build_all(force=False, verbose=False):
    return [build_hip(force, verbose), build_host(force, verbose), build_examples(force, verbose), build_c_example(force, verbose)]


def build_diag(verbose=False):
    """Diagnostic build with in-kernel cycle stamps (-DSRT_DIAG): libsrt_hip_diag.so, never loaded by the product."""
    out = os.path.join(HERE, "libsrt_hip_diag.so")
    cmd = [hipcc()] + HIPCC_FLAGS + ["-DSRT_DIAG", "-o", out, HIP_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for the diagnostic build")
    return out


LIB_SURFACE_LANE = os.path.join(HERE, "libsrt_hip_surface_lane.so")


def build_surface_lane_stores(force=False):
    """The surface kernels' other store form (-DSRT_SURFACE_LANE_STORES, srt_query.h): libsrt_hip_surface_lane.so, never loaded by the
    product; tools/ray_query_probe.py --surface times it beside the shipped library."""
    if not force and not _stale(LIB_SURFACE_LANE, HIP_DEPS):
        return LIB_SURFACE_LANE
    cmd = [hipcc()] + HIPCC_FLAGS + ["-DSRT_SURFACE_LANE_STORES", "-o", LIB_SURFACE_LANE, HIP_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for the lane-stores build")
    return LIB_SURFACE_LANE


LIB_SEGMENTS_NO_BOX_TEST_2 = os.path.join(HERE, "libsrt_hip_segments_no_box_test_2.so")


def build_segments_no_box_test_2(force=False):
    """The segment query without its second box test (-DSRT_SEGMENTS_NO_BOX_TEST_2, srt_query.h): libsrt_hip_segments_no_box_test_2.so, never
    loaded by the product; tools/ray_query_probe.py --segments times it beside the shipped library."""
    if not force and not _stale(LIB_SEGMENTS_NO_BOX_TEST_2, HIP_DEPS):
        return LIB_SEGMENTS_NO_BOX_TEST_2
    cmd = [hipcc()] + HIPCC_FLAGS + ["-DSRT_SEGMENTS_NO_BOX_TEST_2", "-o", LIB_SEGMENTS_NO_BOX_TEST_2, HIP_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for the build without box test 2")
    return LIB_SEGMENTS_NO_BOX_TEST_2


LIB_AO_DEAL = {True: os.path.join(HERE, "libsrt_hip_ao_spread.so"), False: os.path.join(HERE, "libsrt_hip_ao_block.so")}


def build_ao_deal(spread, force=False):
    """The ambient-occlusion calls with ONE deal of rays to waves whatever the direction count (-DSRT_AO_SPREAD_FROM, srt_hip.hip): the
    spread deal from 0 directions on (libsrt_hip_ao_spread.so) or never (libsrt_hip_ao_block.so).  Never loaded by the product;
    tools/ray_query_probe.py --ao times both beside the shipped rule."""
    out = LIB_AO_DEAL[bool(spread)]
    if not force and not _stale(out, HIP_DEPS):
        return out
    cmd = [hipcc()] + HIPCC_FLAGS + ["-DSRT_AO_SPREAD_FROM=" + ("0u" if spread else "0xFFFFFFFFu"), "-o", out, HIP_SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stdout + r.stderr)
        raise RuntimeError("hipcc failed for the ambient-occlusion deal build")
    return out


if __name__ == "__main__":
    if "--ao-deals" in sys.argv:
        print(build_ao_deal(True), build_ao_deal(False))
    elif "--segments-no-box-test-2" in sys.argv:
        print(build_segments_no_box_test_2())
    elif "--diag" in sys.argv:
        print(build_diag(verbose=True))
    elif "--surface-lane-stores" in sys.argv:
        print(build_surface_lane_stores())
    else:
        build_all(force="--force" in sys.argv, verbose=True)
