"""No GPU: the yardstick of the signed-distance query (tests/sign_ref.py, include/srt_signed.h) gives a TRUE sign, sees its mutants, and the
binding matches the header.

  * truth: the generalised winding number in float64, the sum of Van Oosterom-Strackee solid angles (arctan2) over every triangle, on the
    closed meshes tests/golden/meshes/cube.npz, sphere.npz and horse.npz and on two overlapping cubes.  Points nearer the surface than
    1e-3 of the extent are left out (at most 5 % of them); on all the others `inside` under the DEFAULT table equals |w| > 0.5;
  * on the two overlapping cubes winding is right and parity is not (it gives XOR);
  * a flipped det sign, a vote of >=, and t = 0 not counted each change an output of the lattice batch (sign_ref.lattice_batch);
  * include/srt_signed.h against abi.SIGNED_PROTOTYPES / SIGNED_STRUCTS, the structs as the C compiler lays them out, the symbol tables
    disjoint, both lib methods' argument counts.
The bunny of ground_bunny is NOT closed (223 edges without a partner): it serves bit parity in tests/test_gpu_signed.py, not this file."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu
import point_ref as pr
import sign_ref as sg
from header_mirror import check_prototypes, parse_header
from oracle import pyoracle
from simple_raytracer_amd import abi, lib
from test_query_dispatch import N, scene

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
HEADER = parse_header(open(os.path.join(INCLUDE, "srt_signed.h")).read())
F = np.float32


def mesh(key):
    m = gu.load_mesh(key)
    return np.ascontiguousarray(m["points"] if isinstance(m, dict) else m, F)


def placed(tris, turn_deg=0.0, scale=1.0, shift=(0.0, 0.0, 0.0)):
    """The triangles turned about y, scaled and shifted (a proper motion: the orientation stays)."""
    a = np.deg2rad(turn_deg)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    out = np.ones(tris.shape, F)
    out[..., :3] = (tris[..., :3].astype(np.float64) @ R.T * scale + np.asarray(shift)).astype(F)
    return out


def built(objects):
    """The flat scene of `objects` (each n x 3 x 4) through the host mirror's builder."""
    from simple_raytracer_amd import build, host
    import scenes
    build.build_host()
    recipe = scenes.Recipe(); meshes = {}
    for k, t in enumerate(objects):
        meshes[f"m{k}"] = t
        recipe.load(f"obj{k}", f"m{k}"); recipe.bvh(f"obj{k}")
    recipe.light = (0.0, 0.0, 0.0)
    return host.build_flat_scene(recipe, meshes)


def winding_number(tri_points, p):
    """The generalised winding number of every point of p (n x 3) about the triangles, float64: sum of 2 atan2(det, ...) / 4 pi."""
    P = np.asarray(tri_points, np.float64).reshape(-1, 3, 4)[..., :3]
    w = np.zeros(p.shape[0])
    for i, q in enumerate(np.asarray(p, np.float64)):
        a, b, c = P[:, 0] - q, P[:, 1] - q, P[:, 2] - q
        la, lb, lc = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1), np.linalg.norm(c, axis=1)
        num = np.einsum("ij,ij->i", a, np.cross(b, c))
        den = la * lb * lc + np.einsum("ij,ij->i", a, b) * lc + np.einsum("ij,ij->i", a, c) * lb + np.einsum("ij,ij->i", b, c) * la
        w[i] = 2.0 * np.arctan2(num, den).sum() / (4.0 * np.pi)
    return w


def closed_and_outward(flat):
    """Every directed edge is matched once by its reverse (per object, by position), and the signed volume per object is positive."""
    for k in range(flat.n_objects):
        t = np.ascontiguousarray(flat.tri_points, F).reshape(-1, 3, 4)[flat.tri_obj == k]
        assert sg.signed_volume(t) > 0, k
        _, ids = np.unique(t[..., :3].reshape(-1, 3), axis=0, return_inverse=True)
        ids = ids.reshape(-1, 3)
        edges = np.concatenate([ids[:, [0, 1]], ids[:, [1, 2]], ids[:, [2, 0]]])
        fwd = {(int(a), int(b)) for a, b in edges}
        assert len(fwd) == len(edges) and all((b, a) in fwd for a, b in fwd), k


def box_points(flat, n, seed):
    """n random points in 1.5 x the scene's box, and the scene's extent."""
    P = np.ascontiguousarray(flat.tri_points, F)[..., :3].reshape(-1, 3)
    mn, mx = P.min(0).astype(np.float64), P.max(0).astype(np.float64)
    c, h = (mn + mx) / 2, (mx - mn) / 2
    return (c + h * 1.5 * np.random.default_rng(seed).uniform(-1, 1, (n, 3))).astype(F), float(np.linalg.norm(mx - mn))


def true_sign(flat, n, seed, what):
    closed_and_outward(flat)
    pts, ext = box_points(flat, n, seed)
    keep = np.sqrt(pr.closest_points(flat, pts)["dist2"].astype(np.float64)) >= 1e-3 * ext
    assert keep.mean() >= 0.95, (what, keep.mean())
    pts = pts[keep]
    w = winding_number(flat.tri_points, pts)
    assert (np.abs(w - np.round(w)) < 1e-6).all(), what                 # (closed: an integer away from the surface)
    got = sg.signs(pyoracle, flat, pts, counts=False)
    truth = np.abs(w) > 0.5
    print(f"{what}: {len(pts)} points kept of {n}, inside {int(truth.sum())}, rays that disagree with the vote "
          f"{int(((got['winding'] > 0) != truth[:, None]).sum())} of {got['winding'].size}")
    assert truth.any() and not truth.all(), what
    assert np.array_equal(got["inside"] != 0, truth), (what, np.flatnonzero((got["inside"] != 0) != truth)[:8])
    return pts, w, got


@pytest.mark.parametrize("name,n,turn", [("cube", 2500, 25.0), ("cube", 2500, 0.0), ("sphere", 2500, 0.0)])
def test_the_default_table_gives_the_true_sign(name, n, turn):
    flat = built([placed(mesh(name), turn, 20.0 if name == "cube" else 1.0, (3.0, -2.0, 40.0))])
    true_sign(flat, n, 7, f"{name}, turned {turn}")


def test_the_true_sign_on_the_horse():
    """65 points: the yardstick's node pass is rays x nodes."""
    true_sign(built([mesh("horse")]), 65, 9, "horse")


def test_winding_is_right_on_overlapping_cubes_and_parity_is_not():
    cube = mesh("cube")
    flat = built([placed(cube, 25.0, 20.0), placed(cube, -10.0, 20.0, (12.0, 9.0, -7.0))])
    pts, w, got = true_sign(flat, 2500, 11, "two cubes")
    both = np.round(w) == 2
    assert both.sum() > 20 and (got["winding"][both] == 2).all()
    odd = sg.signs(pyoracle, flat, pts, parity=True, counts=False)
    assert (odd["inside"][both] == 0).all() and np.array_equal(odd["inside"][~both], got["inside"][~both])


def test_mutants_are_seen():
    flat = sg.lattice_scene()
    assert flat.n_nodes == 1 and flat.node_count[0] == 12
    closed_and_outward(flat)
    pts, dirs = sg.lattice_batch()
    want = sg.signs(pyoracle, flat, pts, dirs)
    # what the batch is for: the origin sees only exits, and more than one where its ray leaves through a face's diagonal (two triangles),
    # an edge (four) or a vertex (six); points on the surface start at t = 0
    origin = int(np.flatnonzero((pts == 0).all(1))[0])
    assert (want["winding"][origin] >= 1).all() and np.array_equal(want["crossings"][origin], want["winding"][origin]) and want["inside"][origin] == 1
    c = pyoracle.ray_triangle(np.repeat(sg.sign_rays(pts, dirs), 12, axis=0), np.tile(np.ascontiguousarray(flat.tri_points, F).reshape(-1, 12), (len(pts) * len(dirs), 1)))
    assert (c == 0).sum() > 100 and (want["crossings"] > 2).any() and (want["crossings"][origin] > 1).any()
    strict = np.abs(pts).max(1) < 1
    assert (want["inside"][strict] == 1).all() and (want["inside"][np.abs(pts).max(1) > 1] == 0).all()
    for mutant in (dict(flip=True), dict(at_least=True), dict(zero_counts=False)):
        got = sg.signs(pyoracle, flat, pts, dirs, counts=False, **mutant)
        changed = [k for k in ("inside", "winding", "crossings") if not np.array_equal(got[k], want[k])]
        print(mutant, "changes", changed)
        assert changed, mutant
    assert not np.array_equal(sg.signs(pyoracle, flat, pts, dirs, parity=True, counts=False)["inside"], want["inside"])
    # the counts of the sign rays: one node a ray, its 12 triangles where the box is hit
    assert (want["node_tests_each"] == 1).all() and np.isin(want["tri_tests_each"], (0, 12)).all()


def test_sdist():
    d2 = np.array([0.0, 2.0, np.inf, 1e-30, 3.0], F)
    got = sg.sdist_of(np.uint8([1, 1, 1, 0, 0]), d2)
    assert np.array_equal(got.view(np.uint32), np.array([-0.0, -np.sqrt(F(2.0)), -np.inf, np.sqrt(F(1e-30)), np.sqrt(F(3.0))], F).view(np.uint32))


def test_the_mirror_matches_the_header(tmp_path):
    names = ["srt_signed_points_device", "srt_signed_points"]
    assert [name for name, _, _ in HEADER["prototypes"]] == list(abi.SIGNED_PROTOTYPES) == names
    assert list(HEADER["structs"]) == list(abi.SIGNED_STRUCTS) == ["srt_sign", "srt_sign_out"]
    assert HEADER["constants"] == {"SRT_SIGN_MAX_DIRS": abi.SIGN_MAX_DIRS, "SRT_SIGN_PARITY": abi.SIGN_PARITY}
    assert check_prototypes(abi.SIGNED_PROTOTYPES, {**abi.STRUCTS, **abi.POINT_STRUCTS, **abi.SIGNED_STRUCTS}, HEADER) == []
    assert lib.SIGNED_SYMBOLS == tuple(abi.SIGNED_PROTOTYPES)
    assert not set(lib.SIGNED_SYMBOLS) & (set(lib.ABI_SYMBOLS) | set(lib.POINT_SYMBOLS) | set(lib.NEAREST_SYMBOLS))
    assert HEADER["structs"]["srt_sign"] == [f for f, _ in abi.Sign._fields_] == ["dirs", "n_dirs", "flags"]
    assert HEADER["structs"]["srt_sign_out"] == [f for f, _ in abi.SignOut._fields_] == list(abi.SIGN_FIELDS) == ["sdist", "inside", "winding", "crossings"]
    # the structs and the default table as the C compiler has them, through include/srt.h alone (which brings the header along)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "srt.h"', "int main(void) {", "    const float d[9] = SRT_SIGN_DEFAULT_DIRS;"]
    for name, cls in abi.SIGNED_STRUCTS.items():
        lines.append(f'    printf("%zu\\n", sizeof({name}));')
        lines += [f'    printf("%zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
    lines += ['    for (int k = 0; k < 9; k++) printf("%a\\n", (double)d[k]);']
    lines += ["    return sizeof(&srt_signed_points) == sizeof(&srt_signed_points_device) && SRT_ABI_VERSION == 3 ? 0 : 1;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-I" + INCLUDE, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.splitlines()
    at = 0
    for cls in abi.SIGNED_STRUCTS.values():
        rows = [[int(x) for x in l.split()] for l in out[at:at + 1 + len(cls._fields_)]]
        assert rows[0] == [C.sizeof(cls)] and rows[1:] == [[getattr(cls, f).offset, getattr(cls, f).size] for f, _ in cls._fields_], cls
        at += 1 + len(cls._fields_)
    table = np.array([float.fromhex(l) for l in out[at:at + 9]], F).reshape(3, 3)
    assert np.array_equal(table.view(np.uint32), abi.SIGN_DEFAULT_DIRS.view(np.uint32)) and abi.SIGN_DEFAULT_DIRS.dtype == F
    assert np.array_equal(abi.SIGN_DEFAULT_DIRS, np.array([[0.57, 0.31, 0.76], [-0.43, 0.81, -0.39], [0.29, -0.66, -0.69]], F))
    assert abi.SRT_ABI_VERSION == 3
    srt_h = open(os.path.join(INCLUDE, "srt.h")).read()
    assert srt_h.index('#include "srt_nearest.h"') < srt_h.index('#include "srt_signed.h"')


def test_symbols_and_defaults():
    sig = inspect.signature(lib.DeviceScene.signed_points).parameters
    assert [(k, sig[k].default) for k in ("radius", "point_mask", "dirs", "parity", "count")] == [("radius", None), ("point_mask", None), ("dirs", None), ("parity", False), ("count", False)]
    assert set(sig["want"].default) == set(abi.SIGN_FIELDS) | set(abi.POINT_FIELDS)
    sig = inspect.signature(lib.DeviceScene.signed_points_device).parameters
    assert list(sig)[:3] == ["self", "n", "d_points"]
    assert all(sig[k].default == 0 for k in ("radius", "point_mask", "dirs", "n_dirs", "stream") + tuple(abi.SIGN_FIELDS) + tuple(abi.POINT_FIELDS))
    assert sig["count"].default is False and sig["parity"].default is False


@pytest.mark.parametrize("dirs", [None, np.eye(3, dtype=np.float32)[:2]])
def test_dispatch(dirs):
    argc = {name: len(args) for name, _, args in HEADER["prototypes"]}
    nd = 3 if dirs is None else 2
    ds = scene()
    o = ds.signed_points(np.zeros((N, 3), F), radius=2.5, point_mask=True, dirs=dirs, parity=True, count=True)
    assert ds.L.calls == [("srt_signed_points", argc["srt_signed_points"])]
    assert o["sdist"].shape == (N,) and o["inside"].dtype == np.uint8 and o["winding"].shape == (N, nd) and o["winding"].dtype == np.int32
    assert o["crossings"].shape == (N, nd) and o["crossings"].dtype == np.uint32 and o["point"].shape == (N, 3) and "stats" in o
    ds = scene()
    assert set(ds.signed_points(np.zeros((N, 3), F), dirs=dirs, want=("inside",))) == {"inside", "stats"}
    ds = scene()
    ds.signed_points_device(N, 0x100, radius=0x1000, dirs=0x400 if dirs is not None else 0, n_dirs=0 if dirs is None else 2, stream=0, count=True, inside=0x200, dist2=0x300)
    assert ds.L.calls == [("srt_signed_points_device", argc["srt_signed_points_device"])]
