"""No GPU: the yardstick of the closest-point query (tests/point_ref.py) IS a closest point, and the Python face of the new calls.

The yardstick's float32 arithmetic is checked against an independent float64 formulation on the same float32 records -- the foot of the
perpendicular on the triangle's plane where it lies inside, else the nearest of the three clamped segment projections -- in distance
(|sqrt(dist2_32) - sqrt(dist2_64)| in units of u * max|coordinate|, u = 2^-24; a relative bound on dist2 would be wrong: a point almost
touching a triangle loses its distance to cancellation) and in the region code wherever float64 says the point is not within rounding of
a Voronoi boundary.  With r = +inf the winner is brute force over all triangles.  Then the mirror of include/srt_points.h
(abi.POINT_PROTOTYPES, abi.POINT_STRUCTS) against that header, by the parser and the rules tests/test_abi_mirror.py applies to include/srt.h;
the symbols, the methods' defaults, and which C symbol each method reaches, by the recorder of tests/test_query_dispatch.py."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import point_ref as pr
import tree_shapes as ts
from header_mirror import check_prototypes, parse_header
from simple_raytracer_amd import abi, build, lib
from test_query_dispatch import N, scene

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADER = parse_header(open(os.path.join(INCLUDE, "srt_points.h")).read())
ARGC = {name: len(args) for name, _, args in HEADER["prototypes"]}


def reached(ds, symbol):
    assert ds.L.calls == [(symbol, ARGC[symbol])], (ds.L.calls, symbol, ARGC[symbol])

F = np.float32
U = 2.0 ** -24
SEEDS = (1, 2, 3, 4)
PAIRS = 40000
# The largest |sqrt(dist2_32) - sqrt(dist2_64)| / (u * max|coordinate|) over SEEDS as measured (per seed: 12.40, 7.49, 17.51, 5.40; the
# worst cases are points ON the plane of a triangle, where the true distance is 0 and the float32 one is rounding noise), and the bound:
# twice that.  The inputs are deterministic; the margin only absorbs another numpy build.
MEASURED_ERR = 17.51
ERR_BOUND = 2.0 * MEASURED_ERR
ASPECT_MIN = 0.1                   # area / (longest edge)^2 of the compared triangles (an equilateral one has 0.43)
MARGIN = 1e-5                      # a float64 quantity of a region test counts as decided when it is beyond MARGIN of its scale (170 u)


def pairs(seed):
    """PAIRS (point, triangle record) pairs: triangles about the origin and about (100, -40, 250), of sizes 1e-2 .. 30; points anywhere
    around them, points ON the triangle's own plane (the true distance is 0 or an edge's), a hair off it, and far off it, over and
    beyond each edge and vertex."""
    rng = np.random.default_rng(seed)
    m = PAIRS
    centre = np.where(rng.random((m, 1)) < 0.5, F(0.0), np.float32([100.0, -40.0, 250.0])).astype(F)
    size = (10.0 ** rng.uniform(-2, 1.5, (m, 1, 1))).astype(F)
    tri = np.ones((m, 3, 4), F)
    tri[..., :3] = centre[:, None, :] + rng.uniform(-1, 1, (m, 3, 3)).astype(F) * size
    # the distance error of a sliver grows as 1 / its aspect (v and w of the face region are quotients of cancelled sums), so the triangles
    # of this comparison have area / (longest edge)^2 >= ASPECT_MIN: a thinner one gets a third vertex at a right angle.  (Zero-area and
    # collinear triangles are pinned bit for bit by tests/point_edges.py; what they compute is not a distance.)
    a, b, c = (tri[:, j, :3].astype(np.float64) for j in range(3))
    longest = np.maximum(np.linalg.norm(b - a, axis=1), np.maximum(np.linalg.norm(c - a, axis=1), np.linalg.norm(c - b, axis=1)))
    thin = np.linalg.norm(np.cross(b - a, c - a), axis=1) < ASPECT_MIN * 1.5 * longest * longest
    side = np.cross(b - a, rng.normal(size=(m, 3)))
    side = side / np.linalg.norm(side, axis=1, keepdims=True) * np.linalg.norm(b - a, axis=1, keepdims=True)
    tri[thin, 2, :3] = (a + side)[thin].astype(F)
    rec = pr.records_of(type("T", (), {"tri_points": tri})())
    A, e1, e2 = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64), rec[:, 6:9].astype(np.float64)
    vw = rng.uniform(-0.6, 1.6, (m, 2))                                # inside, beyond every edge, beyond every vertex
    nrm = np.cross(e1, e2)
    nrm = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-30)
    kind = rng.integers(0, 4, m)
    off = np.select([kind == 0, kind == 1, kind == 2], [0.0, 10.0 ** rng.uniform(-7, -3, m), 10.0 ** rng.uniform(-2, 0, m)], 10.0 ** rng.uniform(0, 2, m))
    off = off * size[:, 0, 0] * rng.choice([-1.0, 1.0], m)
    p = (A + e1 * vw[:, :1] + e2 * vw[:, 1:] + nrm * off[:, None]).astype(F)
    return p, rec


def closest64(p, rec):
    """The independent formulation, float64 on the float32 records: (dist2, region) per pair, and the margin of the region decision --
    the smallest |quantity| / scale over the quantities the region tests compare with zero."""
    p = p.astype(np.float64); A = rec[:, 0:3].astype(np.float64); e1 = rec[:, 3:6].astype(np.float64); e2 = rec[:, 6:9].astype(np.float64)
    B, C = A + e1, A + e2
    dot = lambda a, b: (a * b).sum(1)
    n = np.cross(e1, e2); nn = dot(n, n)
    ap = p - A
    with np.errstate(all="ignore"):
        s = dot(ap, n) / nn
        fa = ap - s[:, None] * n                                      # the foot of the perpendicular, from A
        v = dot(np.cross(fa, e2), n) / nn; w = dot(np.cross(e1, fa), n) / nn
        inside = (nn > 0) & (v >= 0) & (w >= 0) & (v + w <= 1)
        face = s * s * nn
    seg_d2, seg_t = [], []
    for P, Q in ((A, B), (B, C), (A, C)):
        d = Q - P; dd = dot(d, d)
        with np.errstate(all="ignore"):
            t = np.where(dd > 0, np.clip(dot(p - P, d) / dd, 0.0, 1.0), 0.0)
        r = p - (P + d * t[:, None])
        seg_d2.append(dot(r, r)); seg_t.append(t)
    seg_d2, seg_t = np.stack(seg_d2, 1), np.stack(seg_t, 1)
    k = np.argmin(seg_d2, 1)
    rows = np.arange(p.shape[0])
    t = seg_t[rows, k]
    code = np.array([[4, 1, 5], [5, 2, 6], [4, 3, 6]])                 # segment x (start, inside, end)
    region = np.where(inside, 0, code[k, np.where(t == 0, 0, np.where(t == 1, 2, 1))])
    dist2 = np.where(inside, face, seg_d2[rows, k])
    # the margin, from Ericson's quantities in float64
    d1, d2 = dot(e1, ap), dot(e2, ap)
    bp = ap - e1; d3, d4 = dot(e1, bp), dot(e2, bp)
    cp = ap - e2; d5, d6 = dot(e1, cp), dot(e2, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    L = np.maximum(np.abs(e1).sum(1), np.abs(e2).sum(1))
    S = L * (np.abs(p).sum(1) + np.abs(A).sum(1) + np.abs(e1).sum(1) + np.abs(e2).sum(1))
    lin = np.min(np.abs(np.stack([d1, d2, d3, d6, d4 - d3, d5 - d6], 1)), 1) / S
    quad = np.min(np.abs(np.stack([va, vb, vc], 1)), 1) / (S * S)
    return dist2, region, np.minimum(lin, quad)


@pytest.fixture(scope="module")
def compared():
    out = []
    for seed in SEEDS:
        p, rec = pairs(seed)
        c = pr.closest_on_triangles(p, rec)
        d2_64, region64, margin = closest64(p, rec)
        out.append((seed, p, rec, c, d2_64, region64, margin))
    return out


def test_distance_against_float64(compared):
    worst = 0.0
    for seed, p, rec, c, d2_64, region64, margin in compared:
        fin = np.isfinite(c["dist2"])
        assert fin.all(), (seed, fin.mean())                           # no case is left out of the comparison
        a, b, c_ = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64), rec[:, 6:9].astype(np.float64)
        longest = np.maximum(np.linalg.norm(b, axis=1), np.maximum(np.linalg.norm(c_, axis=1), np.linalg.norm(c_ - b, axis=1)))
        assert (np.linalg.norm(np.cross(b, c_), axis=1) >= ASPECT_MIN * longest * longest).all()
        assert (c["dist2"][fin] >= 0).all() and not np.signbit(c["dist2"][fin]).any()
        A, e1, e2 = rec[:, 0:3].astype(np.float64), rec[:, 3:6].astype(np.float64), rec[:, 6:9].astype(np.float64)
        M = np.max(np.abs(np.concatenate([p.astype(np.float64), A, A + e1, A + e2], 1)), 1)
        err = np.abs(np.sqrt(c["dist2"].astype(np.float64)) - np.sqrt(d2_64)) / (U * M)
        k = int(np.argmax(np.where(fin, err, -1.0)))
        print(f"seed {seed}: {int(fin.sum())} finite pairs of {fin.size}, largest distance error {err[k]:.3f} u * max|coordinate| at pair {k} "
              f"(dist {np.sqrt(d2_64[k]):.3e}, max|coordinate| {M[k]:.3e})")
        worst = max(worst, float(err[fin].max()))
        assert (err[fin] <= ERR_BOUND).all(), (seed, float(err[fin].max()))
        # the point returned is at that distance, and on the triangle
        q = c["point"].astype(np.float64)
        back = np.abs(np.sqrt(((p.astype(np.float64) - q) ** 2).sum(1)) - np.sqrt(d2_64)) / (U * M)
        assert (back[fin] <= ERR_BOUND + 4.0).all(), (seed, float(back[fin].max()))      # + the rounding of P1 + q itself
        assert (c["v"][fin] >= 0).all() and (c["w"][fin] >= 0).all() and (c["v"][fin] + c["w"][fin] <= 1.0 + 4 * U).all()
    print(f"largest over the seeds: {worst:.3f} (MEASURED_ERR {MEASURED_ERR}, bound {ERR_BOUND})")
    assert worst > 0.25 * MEASURED_ERR, "the recorded measurement is stale"


def test_region_against_float64(compared):
    for seed, p, rec, c, d2_64, region64, margin in compared:
        decided = margin > MARGIN
        share = float(decided.mean())
        print(f"seed {seed}: region compared on {share:.3f} of the pairs, regions seen {np.bincount(c['region'], minlength=7).tolist()}")
        assert share > 0.4 and (np.bincount(c["region"][decided], minlength=7) > 100).all(), "every region is compared"
        bad = np.flatnonzero(decided & (c["region"] != region64))
        assert bad.size == 0, (seed, bad[:5], c["region"][bad[:5]], region64[bad[:5]], margin[bad[:5]])


def test_literal_cases():
    """The triangle (0,0,0) (1,0,0) (0,1,0): every region by hand."""
    rec = np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]])
    cases = [((0.25, 0.25, 2.0), 0, (0.25, 0.25), 4.0), ((0.5, -1.0, 0.0), 1, (0.5, 0.0), 1.0), ((1.0, 1.0, 0.0), 2, (0.5, 0.5), 0.5),
             ((-2.0, 0.5, 0.0), 3, (0.0, 0.5), 4.0), ((-1.0, -1.0, 0.0), 4, (0.0, 0.0), 2.0), ((3.0, -1.0, 0.0), 5, (1.0, 0.0), 5.0),
             ((-1.0, 3.0, 0.0), 6, (0.0, 1.0), 5.0),
             # on the boundaries: the first region of the table wins
             ((0.0, 0.0, 0.0), 4, (0.0, 0.0), 0.0), ((1.0, 0.0, 0.0), 5, (1.0, 0.0), 0.0), ((0.0, 1.0, 0.0), 6, (0.0, 1.0), 0.0),
             ((0.5, 0.0, 0.0), 1, (0.5, 0.0), 0.0), ((0.0, 0.5, 0.0), 3, (0.0, 0.5), 0.0), ((0.5, 0.5, 0.0), 2, (0.5, 0.5), 0.0)]
    for p, region, vw, d2 in cases:
        c = pr.closest_on_triangles(np.float32([p]), rec)
        assert (int(c["region"][0]), float(c["v"][0]), float(c["w"][0]), float(c["dist2"][0])) == (region, vw[0], vw[1], d2), (p, c)


@pytest.mark.parametrize("name", ["cube", "sliced", "loose", "shuffled"])
def test_winner_is_brute_force_without_a_radius(name):
    flat = gu.GoldenScene("cube").flat if name == "cube" else ts.family(name)
    rng = np.random.default_rng(7)
    mn, mx = flat.tri_points[..., :3].reshape(-1, 3).min(0), flat.tri_points[..., :3].reshape(-1, 3).max(0)
    pts = (mn + (mx - mn) * rng.uniform(-0.5, 1.5, (65, 3))).astype(F)
    o = pr.closest_points(flat, pts)
    tri, d2 = pr.brute_force(flat, pts)
    assert np.array_equal(o["tri"], tri) and np.array_equal(o["dist2"].view(np.uint32), d2.view(np.uint32))
    assert o["node_tests"] == 65 * flat.n_nodes and o["tri_tests"] == 65 * flat.n_tris and o["hits"] == 65
    # a radius only takes candidates away: the winner within it is the same triangle or none, the counts shrink, nothing else moves
    r = np.sqrt(np.median(d2)).astype(F)
    q = pr.closest_points(flat, pts, radius=r)
    with np.errstate(invalid="ignore"):
        inside = d2 <= r * r
    assert np.array_equal(q["tri"], np.where(inside, tri, -1)) and q["node_tests"] < o["node_tests"] and q["tri_tests"] < o["tri_tests"]
    assert np.array_equal(q["dist2"][inside].view(np.uint32), d2[inside].view(np.uint32)) and np.isinf(q["dist2"][~inside]).all()
    # the radii that walk nothing, and the order of the points
    none = pr.closest_points(flat, pts, radius=np.where(np.arange(65) % 2 == 0, F(-1.0), F(np.nan)))
    assert (none["tri"] == -1).all() and none["node_tests"] == 0 and none["tri_tests"] == 0
    perm = rng.permutation(65)
    z = pr.closest_points(flat, pts[perm], radius=r)
    assert np.array_equal(z["tri"], q["tri"][perm]) and (z["node_tests"], z["tri_tests"]) == (q["node_tests"], q["tri_tests"])
    # masks: all ones is the unmasked query; an object no point sees is not walked
    assert pr.closest_points(flat, pts, radius=r, point_mask=np.full(65, 0xFFFFFFFF, np.uint32), obj_mask=np.full(flat.n_objects, 0xFFFFFFFF, np.uint32))["node_tests"] == q["node_tests"]
    hidden = pr.closest_points(flat, pts, point_mask=np.full(65, 1, np.uint32), obj_mask=np.where(np.arange(flat.n_objects) == 0, 2, 1).astype(np.uint32))
    assert not np.isin(hidden["tri"], np.flatnonzero(flat.tri_obj == 0)).any()


def test_the_mirror_matches_the_extension_header(tmp_path):
    """include/srt_points.h against abi.POINT_PROTOTYPES / POINT_STRUCTS: every argument, the header's order, the struct as the C compiler
    lays it out; include/srt.h brings the header along, and the library exports what it declares."""
    assert [name for name, _, _ in HEADER["prototypes"]] == list(abi.POINT_PROTOTYPES) == ["srt_closest_points_device", "srt_closest_points"]
    assert list(HEADER["structs"]) == list(abi.POINT_STRUCTS) == ["srt_point_out"] and not HEADER["constants"]
    assert check_prototypes(abi.POINT_PROTOTYPES, {**abi.STRUCTS, **abi.POINT_STRUCTS}, HEADER) == []
    assert lib.POINT_SYMBOLS == tuple(abi.POINT_PROTOTYPES) and not set(lib.POINT_SYMBOLS) & set(lib.ABI_SYMBOLS)
    fields = HEADER["structs"]["srt_point_out"]
    assert fields == [f for f, _ in abi.PointOut._fields_] == list(abi.POINT_FIELDS) == ["tri", "dist2", "point", "vw", "region"]
    # the struct as the C compiler lays it out, through include/srt.h alone (which brings the extension header along)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "srt.h"', "int main(void) {", '    printf("%zu\\n", sizeof(srt_point_out));']
    lines += [f'    printf("%zu %zu\\n", offsetof(srt_point_out, {f}), sizeof(((srt_point_out*)0)->{f}));' for f in fields]
    lines += ["    return sizeof(&srt_closest_points) == sizeof(&srt_closest_points_device) ? 0 : 1;", "}"]      # (declared; nothing to link)
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-I" + INCLUDE, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = [[int(x) for x in l.split()] for l in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert out[0] == [C.sizeof(abi.PointOut)] and out[1:] == [[getattr(abi.PointOut, f).offset, getattr(abi.PointOut, f).size] for f in fields]
    build.build_all()
    L = lib.load()
    assert all(hasattr(L, name) for name in lib.POINT_SYMBOLS)
    assert C.sizeof(abi.PointOut) == 5 * C.sizeof(C.c_void_p) and [getattr(abi.PointOut, f).offset for f in fields] == [k * C.sizeof(C.c_void_p) for k in range(5)]
    assert abi.SRT_ABI_VERSION == 3


def test_symbols_and_defaults():
    for name in ("srt_closest_points_device", "srt_closest_points"):
        assert name in lib.POINT_SYMBOLS and name in ARGC
    sig = inspect.signature(lib.DeviceScene.closest_points).parameters
    assert [(k, sig[k].default) for k in ("radius", "point_mask", "count")] == [("radius", None), ("point_mask", None), ("count", False)]
    sig = inspect.signature(lib.DeviceScene.closest_points_device).parameters
    assert list(sig)[:3] == ["self", "n", "d_points"]
    assert all(sig[k].default == 0 for k in ("radius", "point_mask", "stream", "tri", "dist2", "point", "vw", "region")) and sig["count"].default is False


@pytest.mark.parametrize("radius", [None, 2.5, np.ones(N, np.float32)])
@pytest.mark.parametrize("point_mask", [None, True, np.arange(N, dtype=np.uint32)])
def test_dispatch_host(radius, point_mask):
    ds = scene()
    o = ds.closest_points(np.zeros((N, 3), np.float32), radius=radius, point_mask=point_mask, count=True)
    reached(ds, "srt_closest_points")
    assert o["tri"].shape == (N,) and o["dist2"].shape == (N,) and o["point"].shape == (N, 3) and o["vw"].shape == (N, 2) and o["region"].dtype == np.uint8
    assert "stats" in o
    ds = scene()
    assert set(ds.closest_points(np.zeros((N, 3), np.float32), want=("dist2",))) == {"dist2", "stats"}
    reached(ds, "srt_closest_points")


@pytest.mark.parametrize("radius,point_mask", [(0, 0), (0x1000, 0), (0, 0x2000), (0x1000, 0x2000)])
def test_dispatch_device(radius, point_mask):
    ds = scene()
    ds.closest_points_device(N, 0x100, radius=radius, point_mask=point_mask, stream=0, count=True, tri=0x200, dist2=0x300)
    reached(ds, "srt_closest_points_device")
