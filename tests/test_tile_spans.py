"""The tile-span table (simple_raytracer_amd/csrc/srt_tile_spans.h) against the reference's slab test, on the CPU.

The table says which 8x8 tiles of a frame may hold a ray that passes some object's root box; the trace launch starts no workgroup for
the others and the shading launch fills them with background.  It is right iff, for every tile it excludes, all 64 rays fail every root
box under the reference's own comparisons.  The judge is a numpy float32 restatement of intersectRayAabbNoOrigin (oracle/srt_oracle.c
ray_aabb), operation by operation, pinned here against the oracle on the golden known-answer rows.  The header is driven through
tools/tile_spans_cli.cpp, built with g++ (no HIP), and the same program runs once more under -fsanitize=address,undefined.
"""
import os
import subprocess

import numpy as np
import pytest

import golden_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI_SRC = os.path.join(ROOT, "tools", "tile_spans_cli.cpp")
CSRC = os.path.join(ROOT, "simple_raytracer_amd", "csrc")
FRAMES = [(96, 54), (100, 52), (192, 108), (1920, 1080)]


# ---- the judge -----------------------------------------------------------------------------------------------------------------
def ray_aabb_f32(o, d, mn, mx):
    """oracle/srt_oracle.c:70-82 in float32; o, d: (..., 3) rays, mn, mx: (..., 3) boxes (broadcast).  Returns bool."""
    f = np.float32
    o, d, mn, mx = (np.asarray(a, f) for a in (o, d, mn, mx))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        def axis(a):
            lo, hi = (mn[..., a] - o[..., a]) / d[..., a], (mx[..., a] - o[..., a]) / d[..., a]
            sw = lo > hi
            return np.where(sw, hi, lo), np.where(sw, lo, hi)
        minx, maxx = axis(0)
        miny, maxy = axis(1)
        out = ~((maxx < miny) | (maxy < minx))
        minx = np.where(miny > minx, miny, minx)
        maxx = np.where(maxy < maxx, maxy, maxx)
        minz, maxz = axis(2)
        out &= ~((minx > maxz) | (minz > maxx))
    return out


def test_restatement_equals_the_oracle_on_the_golden_rows():
    from oracle import pyoracle as po
    kat = gu.load_kat()
    ray, box = kat["ab_ray"], kat["ab_box"]
    assert np.array_equal(ray_aabb_f32(ray[:, :3], ray[:, 3:6], box[:, :3], box[:, 3:6]), po.ray_aabb(ray, box).astype(bool))
    assert np.array_equal(ray_aabb_f32(kat["ab_ray"][:, :3], kat["ab_ray"][:, 3:6], kat["ab_box"][:, :3], kat["ab_box"][:, 3:6]), kat["ab_hit"].astype(bool))


def live_tiles(mn, mx, W, H, focal):
    """(gy, gx) bool: some ray of the tile passes some root box under the reference's comparisons.  Rays as the kernels and the
    reference form them: (i0 + x, j0 + y, focal), i0 = int(-W / 2)."""
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    d = np.empty((H, W, 3), np.float32)
    d[..., 0] = (i0 + np.arange(W, dtype=np.int64)).astype(np.float32)[None, :]
    d[..., 1] = (j0 + np.arange(H, dtype=np.int64)).astype(np.float32)[:, None]
    d[..., 2] = np.float32(focal)
    o = np.zeros(3, np.float32)
    hit = np.zeros((H, W), bool)
    for k in range(mn.shape[0]):
        hit |= ray_aabb_f32(o, d, mn[k], mx[k])
    gy, gx = (H + 7) // 8, (W + 7) // 8
    pad = np.zeros((gy * 8, gx * 8), bool)
    pad[:H, :W] = hit
    return pad.reshape(gy, 8, gx, 8).any(axis=(1, 3))


# ---- the program under test ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_spans") / "tile_spans_cli")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, CLI_SRC], check=True)
    return exe


def fmt(x):
    return float(np.float32(x)).hex() if np.isfinite(x) else ("nan" if np.isnan(x) else ("inf" if x > 0 else "-inf"))


def case_text(mn, mx, W, H, focal):
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    lines = [f"{mn.shape[0]} {W} {H} {i0} {j0} {fmt(focal)}"]
    lines += [" ".join(fmt(v) for v in (*mn[k], *mx[k])) for k in range(mn.shape[0])]
    return "\n".join(lines) + "\n"


def run_cases(exe, cases):
    """cases: [(mn, mx, W, H, focal)] -> [None (off) or a (gy, gx) bool array of kept tiles], one process for all."""
    r = subprocess.run([exe], input="".join(case_text(*c) for c in cases), capture_output=True, text=True, check=True)
    lines = r.stdout.splitlines()
    out, at = [], 0
    for (mn, mx, W, H, focal) in cases:
        on, row0, n_rows = (int(v) for v in lines[at].split()); at += 1
        if not on:
            out.append(None); continue
        gy, gx = (H + 7) // 8, (W + 7) // 8
        spans = [tuple(int(v) for v in s.split(":")) for s in lines[at].split()]; at += 1
        assert len(spans) == gy
        kept = np.zeros((gy, gx), bool)
        for r_, (x0, n) in enumerate(spans):
            assert x0 + n <= gx
            if not (row0 <= r_ < row0 + n_rows):
                assert n == 0, "a span outside row0 .. row0 + n_rows"
            kept[r_, x0:x0 + n] = True
        assert n_rows >= 1 and row0 + n_rows <= gy
        out.append(kept)
    assert at == len(lines)
    return out


def root_boxes(flat):
    r = flat.obj_root.astype(np.int64)
    return flat.node_min.reshape(-1, 3)[r].copy(), flat.node_max.reshape(-1, 3)[r].copy()


def assert_conservative(kept, mn, mx, W, H, focal, what):
    live = live_tiles(mn, mx, W, H, focal)
    missed = live & ~kept
    assert not missed.any(), f"{what}: {int(missed.sum())} excluded tiles hold a ray that passes a root box, first (row, tile) {tuple(np.argwhere(missed)[0])}"


# ---- golden scenes -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_tables(cli):
    boxes = {name: root_boxes(gu.GoldenScene(name).flat) for name in gu.SCENES}
    cases = [(boxes[name][0], boxes[name][1], W, H, 400.0) for name in gu.SCENES for (W, H) in FRAMES]
    keys = [(name, W, H) for name in gu.SCENES for (W, H) in FRAMES]
    return boxes, dict(zip(keys, run_cases(cli, cases)))


@pytest.mark.parametrize("name", gu.SCENES)
def test_golden_scenes_exclude_no_live_tile(golden_tables, name):
    boxes, tables = golden_tables
    mn, mx = boxes[name]
    for (W, H) in FRAMES:
        kept = tables[(name, W, H)]
        assert kept is not None, f"{name} {W}x{H}: fell back"
        assert_conservative(kept, mn, mx, W, H, 400.0, f"{name} {W}x{H}")


def test_headline_frames_keep_what_the_rule_promises(golden_tables):
    _, tables = golden_tables
    assert int(tables[("ground_bunny", 1920, 1080)].sum()) <= 16612
    assert int(tables[("cube_ground", 1920, 1080)].sum()) <= 15254


# ---- seeded random families ------------------------------------------------------------------------------------------------------
def rect_rule_front(mn, mx, W, H, focal):
    """The rule restated for boxes wholly in front (z_min > 0), in float64: per box the projected rectangle, grown by one tile and clamped;
    per row the hull of the rectangles.  Returns the kept mask."""
    gy, gx = (H + 7) // 8, (W + 7) // 8
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    lo_x = np.full(gy, gx, np.int64); hi_x = np.full(gy, -1, np.int64)
    for k in range(mn.shape[0]):
        lo = mn[k].astype(np.float64); hi = mx[k].astype(np.float64)
        lo = lo - (np.abs(lo) * 2.0 ** -22 + 2.0 ** -100); hi = hi + (np.abs(hi) * 2.0 ** -22 + 2.0 ** -100)
        assert lo[2] > 0
        def rng(a0, a1, off, n):
            q0 = a0 / hi[2] if a0 >= 0 else a0 / lo[2]
            q1 = a1 / hi[2] if a1 <= 0 else a1 / lo[2]
            t0 = max(np.floor((focal * q0 - off) / 8.0) - 1, 0); t1 = min(np.floor((focal * q1 - off) / 8.0) + 1, n - 1)
            return int(t0), int(t1)
        tx0, tx1 = rng(lo[0], hi[0], i0, gx); ty0, ty1 = rng(lo[1], hi[1], j0, gy)
        if tx0 > tx1 or ty0 > ty1:
            continue
        lo_x[ty0:ty1 + 1] = np.minimum(lo_x[ty0:ty1 + 1], tx0); hi_x[ty0:ty1 + 1] = np.maximum(hi_x[ty0:ty1 + 1], tx1)
    kept = np.zeros((gy, gx), bool)
    for r in range(gy):
        if hi_x[r] >= lo_x[r]:
            kept[r, lo_x[r]:hi_x[r] + 1] = True
    return kept


def family(name, rng, W, H, focal):
    """One scene of 1..3 boxes of the family."""
    n = int(rng.integers(1, 4))
    mn = np.empty((n, 3), np.float32); mx = np.empty((n, 3), np.float32)
    for k in range(n):
        z = float(rng.uniform(2.0, 600.0))
        half_w, half_h = 0.75 * W / focal * z, 0.75 * H / focal * z          # a centre up to 1.5 half-frames out at depth z
        c = np.array([rng.uniform(-half_w, half_w), rng.uniform(-half_h, half_h), z])
        e = np.array([rng.uniform(0.01, 0.3) * half_w, rng.uniform(0.01, 0.3) * half_h, rng.uniform(0.01, 0.9) * (z - 1.0)]) + 1e-3
        lo, hi = c - e, c + e
        if name == "front":
            lo[2] = max(lo[2], 1.0)
        elif name == "straddle":
            lo[2] = -rng.uniform(0.01, 50.0)
        elif name == "origin":
            lo = -np.abs(rng.uniform(0.0, 30.0, 3)); hi = np.abs(rng.uniform(0.0, 30.0, 3))
        elif name == "flat":
            a = int(rng.integers(0, 3)); hi[a] = lo[a]
        elif name == "zero_face":
            a = int(rng.integers(0, 2)); kind = int(rng.integers(0, 3))
            if kind == 0: lo[a], hi[a] = 0.0, abs(hi[a]) + 0.5
            elif kind == 1: lo[a], hi[a] = -abs(lo[a]) - 0.5, -0.0
            else: lo[a] = hi[a] = 0.0
            if rng.integers(0, 2): lo[2] = -rng.uniform(0.01, 50.0)
        elif name == "behind":
            lo[2], hi[2] = -hi[2], -max(lo[2], 1.0)
        elif name.startswith("off_"):
            a, s = {"off_left": (0, -1), "off_right": (0, 1), "off_up": (1, -1), "off_down": (1, 1)}[name]
            half = (W if a == 0 else H) / focal * z
            centre = s * rng.uniform(0.55, 3.0) * half; ext = rng.uniform(0.001, 0.04) * half
            lo[a], hi[a] = centre - ext, centre + ext
            lo[2] = max(lo[2], 1.0)
        mn[k], mx[k] = lo.astype(np.float32), hi.astype(np.float32)
    return mn, mx


FAMILIES = ["front", "straddle", "origin", "flat", "zero_face", "behind", "off_left", "off_right", "off_up", "off_down"]


@pytest.mark.parametrize("fam", FAMILIES)
def test_random_family(cli, fam):
    rng = np.random.default_rng(0x7115 + FAMILIES.index(fam))
    cases = []
    for (W, H) in ((96, 54), (100, 52)):
        for focal in (400.0, 60.0, 30.5):
            cases += [(*family(fam, rng, W, H, focal), W, H, focal) for _ in range(12)]
    tables = run_cases(cli, cases)
    n_excluded = 0
    for (mn, mx, W, H, focal), kept in zip(cases, tables):
        assert kept is not None, f"{fam}: a finite, ordered scene fell back"
        assert_conservative(kept, mn, mx, W, H, focal, fam)
        n_excluded += int((~kept).sum())
        if fam == "front":
            assert int(kept.sum()) <= int(rect_rule_front(mn, mx, W, H, focal).sum()), "keeps more than the rectangles' own area"
        if fam == "origin":
            assert kept.all()
    if fam != "origin":
        assert n_excluded > 0, "the family never excluded a tile: it tests nothing"


def test_fallback_inputs_yield_off(cli):
    ok_mn, ok_mx = np.array([[-1, -1, 5]], np.float32), np.array([[1, 1, 6]], np.float32)
    def with_(mn_or_mx, a, v):
        mn, mx = ok_mn.copy(), ok_mx.copy()
        (mn if mn_or_mx == 0 else mx)[0, a] = v
        return mn, mx
    cases = [(ok_mn, ok_mx, 96, 54, f) for f in (0.0, -400.0, np.inf, -np.inf, np.nan)]
    for a in range(3):
        cases += [(*with_(0, a, v), 96, 54, 400.0) for v in (np.nan, -np.inf, np.inf, -1e31)]
        cases += [(*with_(1, a, v), 96, 54, 400.0) for v in (np.nan, np.inf, 1e31)]
        cases += [(*with_(0, a, 3.0e38), 96, 54, 400.0)]                       # inverted: min beyond max (an empty leaf's box)
    fmax = np.float32(3.4028235e38)
    cases.append((np.array([[fmax] * 3], np.float32), np.array([[-fmax] * 3], np.float32), 96, 54, 400.0))
    cases.append((np.vstack([ok_mn, [[np.nan] * 3]]).astype(np.float32), np.vstack([ok_mx, [[1, 1, 1]]]).astype(np.float32), 96, 54, 400.0))
    cases.append((ok_mn, ok_mx, 96, 8 * 512 + 1, 400.0))                       # more tile rows than the table has room for
    cases.append((np.tile(ok_mn, (4097, 1)), np.tile(ok_mx, (4097, 1)), 96, 54, 400.0))      # more objects than a table is made for per call
    assert all(t is None for t in run_cases(cli, cases))
    # and the plain scene itself is on, at the table's last row too
    assert all(t is not None for t in run_cases(cli, [(ok_mn, ok_mx, 96, 54, 400.0), (ok_mn, ok_mx, 96, 8 * 512, 400.0),
                                                     (np.tile(ok_mn, (4096, 1)), np.tile(ok_mx, (4096, 1)), 96, 54, 400.0)]))


def test_nothing_in_view_keeps_one_tile(cli):
    mn, mx = np.array([[5000, 5000, 5]], np.float32), np.array([[5001, 5001, 6]], np.float32)
    (kept,) = run_cases(cli, [(mn, mx, 96, 54, 400.0)])
    assert kept is not None and int(kept.sum()) == 1 and kept[0, 0]
    (kept,) = run_cases(cli, [(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 96, 54, 400.0)])
    assert kept is not None and int(kept.sum()) == 1


def test_cli_under_address_and_undefined_sanitizers(tmp_path):
    """The header and the helper's main as a stand-alone program under -fsanitize=address,undefined: every family once, the fallbacks, the
    tallest frame.  (Nothing here is loaded into python.)"""
    exe = str(tmp_path / "tile_spans_cli_san")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, CLI_SRC], check=True)
    rng = np.random.default_rng(99)
    text = "".join(case_text(*family(fam, rng, W, H, 400.0), W, H, 400.0) for fam in FAMILIES for (W, H) in ((96, 54), (100, 52), (1920, 1080)))
    text += case_text(np.array([[np.nan, 0, 0]], np.float32), np.array([[1, 1, 1]], np.float32), 96, 54, 400.0)
    text += case_text(np.array([[-1, -1, 5]], np.float32), np.array([[1, 1, 6]], np.float32), 65535 * 8, 4096, 400.0)
    text += case_text(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 8, 8, 400.0)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
