"""CPU: the yardstick of the K-nearest-triangles queries (tests/points_multi_ref.py) and the binding of include/srt_points_multi.h.

  * the columns: column 0 is tests/point_ref.closest_points, and at r = +inf the columns are a brute-force sort over all triangles;
  * the nearest form's walk simulated with k slots, offers arriving late, the bound read from slot k - 1 alone: the yardstick's columns on
    every fixture of tests/test_gpu_nearest.py, with the counts between the mandatory set's and the closest form's;
  * the inputs of tests/test_gpu_points_multi.py reach every case: points with nothing within the radius, with fewer than k and with
    more than k, on every scene, and a batch of ties;
  * the header against abi.POINT_MULTI_PROTOTYPES / POINT_MULTI_STRUCTS with the compiler's layout, and which symbol each method reaches."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import nearest_ref as nr
import point_ref as pr
import points_multi_ref as pm
import test_gpu_nearest as tn
import test_gpu_points as tp
from header_mirror import check_prototypes, parse_header
from simple_raytracer_amd import abi, build, lib
from test_query_dispatch import N, scene

F = np.float32
INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = parse_header(open(os.path.join(INCLUDE, "srt_points_multi.h")).read())
ARGC = {name: len(args) for name, _, args in HEADER["prototypes"]}
NAMES = ["srt_closest_points_multi_device", "srt_closest_points_multi", "srt_nearest_points_multi_device", "srt_nearest_points_multi"]
FIELDS = ["n_within", "n_found", "tri", "dist2", "point", "vw", "region"]
COVERED = ("sliced", "roots33", "comb256", "shuffled", "ground_bunny")


@pytest.mark.parametrize("name", ["cube", "sliced", "roots33", "comb256"])
def test_columns(name):
    flat, pts, rad, single = tp.case(name)
    cand = pm.candidates(flat, pts, rad)
    for k in (1, 4, 16):
        want = pm.columns(cand, k)
        pr.same({key: want[key][:, 0] for key in pr.SAME_KEYS}, single, f"{name}, column 0 of {k}")
        assert (want["node_tests"], want["tri_tests"], want["hits"]) == (single["node_tests"], single["tri_tests"], single["hits"])
        assert np.array_equal(want["n_found"], np.minimum(want["n_within"], k)) and np.array_equal(want["n_found"], (want["tri"] >= 0).sum(1))
        assert np.array_equal(np.isinf(want["dist2"]), want["tri"] < 0)
    # r = +inf: every triangle is a candidate; the columns are the sort of all of them by (dist2, id)
    p = pts[:65]
    k = 16
    want = pm.closest_points_multi(flat, p, k)
    rec = pr.records_of(flat)
    T = rec.shape[0]
    for i in range(len(p)):
        d2 = pr.closest_on_triangles(np.repeat(p[i:i + 1], T, 0), rec)["dist2"]
        ok = np.flatnonzero(~np.isnan(d2))
        best = ok[np.lexsort((ok, d2[ok]))][:k]
        assert want["n_within"][i] == ok.size and want["n_found"][i] == best.size
        assert np.array_equal(want["tri"][i, :best.size], best) and np.array_equal(want["dist2"][i, :best.size].view(np.uint32), d2[best].view(np.uint32))
        assert (want["tri"][i, best.size:] == -1).all()


def check_walks(flat, pts, rad, k, what):
    want = pm.closest_points_multi(flat, pts, k, rad)
    need_nodes, need_tris = pm.mandatory(flat, pts, want, k, rad)
    for rep, max_delay in enumerate((0, 512)):
        got = pm.shrinking_walk(flat, pts, k, rad, max_delay=max_delay, seed=rep)
        pm.same(got, want, f"{what}, k {k}, delay {max_delay}")
        assert (got["node_tests_each"] >= need_nodes).all() and (got["tri_tests_each"] >= need_tris).all(), (what, k, max_delay)
        assert (got["node_tests_each"] <= want["node_tests_each"]).all() and (got["tri_tests_each"] <= want["tri_tests_each"]).all(), (what, k, max_delay)
    return got, want


def test_the_simulated_walk_gives_the_columns():
    """Every fixture of tests/test_gpu_nearest.py: the walk with k slots and late offers gives the yardstick's columns, whatever the delay.
    The small scenes take 32 of their points at two k, without a radius and with the radii of the GPU tests; the bunny 4 points."""
    for what, flat, pts in tn.fixtures():
        small = flat.n_tris < 1000
        if small:
            assert nr.ancestors_hold(flat, pts) == 0, what
        sub = pts[:32] if small else pts[:4]
        rad = tp.radii_for(float(np.linalg.norm(np.ptp(np.ascontiguousarray(flat.tri_points, F)[..., :3].reshape(-1, 3), axis=0))), tp.N, 17, 64)[:len(sub)]
        for k in (4, 16) if small else (4,):
            got, want = check_walks(flat, sub, None, k, what)
            if flat.n_tris > 64:
                assert got["tri_tests"] < want["tri_tests"], (what, k)
            if small:
                check_walks(flat, sub, rad, k, what + ", radii")


@pytest.mark.parametrize("name", COVERED)
def test_the_inputs_reach_every_case(name):
    """tests/test_gpu_points.case(name) as tests/test_gpu_points_multi.py uses it: for k = 4 and k = 16 there are points with nothing within
    their radius (the empty columns), with fewer than k (the partly filled row) and with more than k (what falls off the last slot)."""
    flat, pts, rad, _ = tp.case(name)
    within = pm.candidates(flat, pts, rad)["n_within"]
    for k in (4, 16):
        none, some, over = int((within == 0).sum()), int(((within > 0) & (within < k)).sum()), int((within > k).sum())
        print(name, "k", k, "points with 0 /", f"1..{k - 1} / >{k} within:", none, some, over)
        assert none > 0 and some > 0 and over > 0, (name, k, none, some, over)
    if name == "sliced":
        assert (int((within == 0).sum()), int(((within > 0) & (within < 16)).sum()), int((within >= 16).sum())) == (108, 55, 94)


def test_ties():
    flat = gu.GoldenScene("cube").flat
    pts = pm.tie_batch(flat)
    assert pts.shape == (11, 3)
    want = pm.closest_points_multi(flat, pts, 8)
    runs = pm.equal_runs(want)
    print("longest run of equal dist2 per point:", runs.tolist())
    assert (runs >= 3).any() and (runs[:8] >= 3).all(), runs
    assert (want["dist2"][:8, :3] == 0).all() and (want["n_within"] == flat.n_tris).all()
    for i in range(len(pts)):
        ids = want["tri"][i][want["dist2"][i] == want["dist2"][i, 0]]
        assert (np.diff(ids) > 0).all()
    got = pm.shrinking_walk(flat, pts, 8, max_delay=64, seed=2)
    pm.same(got, want, "ties, simulated")


def test_the_mirror_matches_the_extension_header(tmp_path):
    assert [name for name, _, _ in HEADER["prototypes"]] == list(abi.POINT_MULTI_PROTOTYPES) == NAMES
    assert list(HEADER["structs"]) == list(abi.POINT_MULTI_STRUCTS) == ["srt_point_multi_out"]
    assert HEADER["constants"] == {"SRT_POINT_MULTI_MAX": abi.POINT_MULTI_MAX} and abi.POINT_MULTI_MAX == 16 == lib.POINT_MULTI_MAX
    assert check_prototypes(abi.POINT_MULTI_PROTOTYPES, {**abi.STRUCTS, **abi.POINT_STRUCTS, **abi.POINT_MULTI_STRUCTS}, HEADER) == []
    assert lib.POINT_MULTI_SYMBOLS == tuple(abi.POINT_MULTI_PROTOTYPES)
    assert not set(lib.POINT_MULTI_SYMBOLS) & (set(lib.ABI_SYMBOLS) | set(lib.POINT_SYMBOLS) | set(lib.NEAREST_SYMBOLS) | set(lib.SIGNED_SYMBOLS))
    protos = {name: (ret, args) for name, ret, args in HEADER["prototypes"]}
    for a, b in (("srt_nearest_points_multi_device", "srt_closest_points_multi_device"), ("srt_nearest_points_multi", "srt_closest_points_multi")):
        assert protos[a] == protos[b]
    fields = HEADER["structs"]["srt_point_multi_out"]
    assert fields == [f for f, _ in abi.PointMultiOut._fields_] == list(abi.POINT_MULTI_FIELDS) == FIELDS
    # the struct as the C compiler lays it out, through include/srt.h alone (which brings the extension header along)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "srt.h"', "int main(void) {", '    printf("%zu\\n", sizeof(srt_point_multi_out));']
    lines += [f'    printf("%zu %zu\\n", offsetof(srt_point_multi_out, {f}), sizeof(((srt_point_multi_out*)0)->{f}));' for f in fields]
    lines += ["    return sizeof(&srt_closest_points_multi) == sizeof(&srt_nearest_points_multi_device) && SRT_POINT_MULTI_MAX == 16 ? 0 : 1;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-I" + INCLUDE, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = [[int(x) for x in l.split()] for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert out[0] == [C.sizeof(abi.PointMultiOut)] and out[1:] == [[getattr(abi.PointMultiOut, f).offset, getattr(abi.PointMultiOut, f).size] for f in fields]
    # the header alone compiles too
    (tmp_path / "alone.c").write_text('#include "srt_points_multi.h"\nint main(void) { return sizeof(srt_point_multi_out) ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-I" + INCLUDE, "-o", str(tmp_path / "alone"), str(tmp_path / "alone.c")], check=True)
    build.build_all()
    L = lib.load()
    assert all(hasattr(L, name) for name in lib.POINT_MULTI_SYMBOLS)
    assert abi.SRT_ABI_VERSION == 3
    text = open(os.path.join(INCLUDE, "srt.h")).read()
    assert '#include "srt_points_multi.h"' in text and text.index('#include "srt_signed.h"') < text.index('#include "srt_points_multi.h"')


def test_symbols_and_defaults():
    sig = inspect.signature(lib.DeviceScene.closest_points_multi).parameters
    assert list(sig)[:3] == ["self", "points", "k"]
    assert [(key, sig[key].default) for key in ("radius", "point_mask", "count")] == [("radius", None), ("point_mask", None), ("count", False)]
    assert sig["want"].default == tuple(FIELDS)
    near = inspect.signature(lib.DeviceScene.nearest_points_multi).parameters
    assert near["want"].default == tuple(FIELDS[1:]) and list(near) == list(sig)
    dev = inspect.signature(lib.DeviceScene.closest_points_multi_device).parameters
    assert list(dev)[:4] == ["self", "n", "d_points", "k"] and all(dev[key].default == 0 for key in ["radius", "point_mask", "stream"] + FIELDS)
    ndev = inspect.signature(lib.DeviceScene.nearest_points_multi_device).parameters
    assert list(ndev) == [key for key in dev if key != "n_within"]


@pytest.mark.parametrize("method,symbol", [("closest_points_multi", "srt_closest_points_multi"), ("nearest_points_multi", "srt_nearest_points_multi")])
@pytest.mark.parametrize("radius", [None, 2.5, np.ones(N, np.float32)])
@pytest.mark.parametrize("point_mask", [None, True, np.arange(N, dtype=np.uint32)])
def test_dispatch_host(method, symbol, radius, point_mask):
    ds = scene()
    o = getattr(ds, method)(np.zeros((N, 3), np.float32), 5, radius=radius, point_mask=point_mask, count=True)
    assert ds.L.calls == [(symbol, ARGC[symbol])]
    assert o["n_found"].shape == (N,) and o["n_found"].dtype == np.uint32 and o["tri"].shape == (N, 5) and o["dist2"].shape == (N, 5)
    assert o["point"].shape == (N, 5, 3) and o["vw"].shape == (N, 5, 2) and o["region"].shape == (N, 5) and o["region"].dtype == np.uint8
    assert ("n_within" in o) == (method == "closest_points_multi") and "stats" in o
    ds = scene()
    assert set(getattr(ds, method)(np.zeros((N, 3), np.float32), 2, want=("dist2",))) == {"dist2", "stats"}
    assert ds.L.calls == [(symbol, ARGC[symbol])]


@pytest.mark.parametrize("radius,point_mask", [(0, 0), (0x1000, 0), (0, 0x2000), (0x1000, 0x2000)])
def test_dispatch_device(radius, point_mask):
    ds = scene()
    ds.closest_points_multi_device(N, 0x100, 7, radius=radius, point_mask=point_mask, stream=0, count=True, n_within=0x400, tri=0x200, dist2=0x300)
    assert ds.L.calls == [("srt_closest_points_multi_device", ARGC["srt_closest_points_multi_device"])]
    ds = scene()
    ds.nearest_points_multi_device(N, 0x100, 7, radius=radius, point_mask=point_mask, stream=0, count=True, n_found=0x400, tri=0x200)
    assert ds.L.calls == [("srt_nearest_points_multi_device", ARGC["srt_nearest_points_multi_device"])]
