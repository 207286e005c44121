"""The tile-span table follows a box's outline (simple_raytracer_amd/csrc/srt_tile_spans.h: z slices, a pixel of margin), on the CPU.

tests/test_tile_spans.py asks that the table excludes no live tile; this file asks how many dead ones it keeps.  Live tiles are counted
here, ray by ray, by that file's float32 restatement of the reference's slab test.  The bound of 1.05 x live on the two headline frames
is the rule's own promise (a prototype stood at 1.018 and 1.016); the one-rectangle rule kept 1.21 and 1.14.
"""
import numpy as np
import pytest

import golden_util as gu
import test_tile_spans as ts

cli = ts.cli      # the module-scoped fixture: tools/tile_spans_cli.cpp built with g++


@pytest.mark.parametrize("name", ["ground_bunny", "cube_ground"])
def test_headline_frames_keep_at_most_a_twentieth_more_than_live(cli, name):
    W, H, focal = 1920, 1080, 400.0
    mn, mx = ts.root_boxes(gu.GoldenScene(name).flat)
    (kept,) = ts.run_cases(cli, [(mn, mx, W, H, focal)])
    assert kept is not None
    live = ts.live_tiles(mn, mx, W, H, focal)
    n_kept, n_live = int(kept.sum()), int(live.sum())
    print(f"{name}: kept {n_kept}, live {n_live}, ratio {n_kept / n_live:.4f}")
    assert not (live & ~kept).any()
    assert n_kept <= 1.05 * n_live, f"{name}: {n_kept} kept tiles for {n_live} live ones"


def rect_rule(mn, mx, W, H, focal):
    """The one-rectangle rule the slices replace, restated in float64 for any finite box that does not hold the origin: per box part
    (z > 0, and the mirror image of z < 0) one projected rectangle, grown by one tile and clamped; per row the hull.  The kept mask."""
    gy, gx = (H + 7) // 8, (W + 7) // 8
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    lo_x = np.full(gy, gx, np.int64); hi_x = np.full(gy, -1, np.int64)
    for k in range(mn.shape[0]):
        lo = mn[k].astype(np.float64); hi = mx[k].astype(np.float64)
        lo = lo - (np.abs(lo) * 2.0 ** -22 + 2.0 ** -100); hi = hi + (np.abs(hi) * 2.0 ** -22 + 2.0 ** -100)
        assert not ((lo <= 0) & (hi >= 0)).all()
        for part in (0, 1):
            (x0, x1), (y0, y1) = ((-hi[0], -lo[0]), (-hi[1], -lo[1])) if part else ((lo[0], hi[0]), (lo[1], hi[1]))
            zb = -lo[2] if part else hi[2]; za = max(-hi[2] if part else lo[2], 0.0)
            if not zb > 0.0:
                continue
            def rng(a0, a1, off, n):
                q0 = a0 / zb if a0 >= 0 else (a0 / za if za > 0 else -np.inf)
                q1 = a1 / zb if a1 <= 0 else (a1 / za if za > 0 else np.inf)
                return max(np.floor((focal * q0 - off) / 8.0) - 1, 0), min(np.floor((focal * q1 - off) / 8.0) + 1, n - 1)
            tx0, tx1 = rng(x0, x1, i0, gx); ty0, ty1 = rng(y0, y1, j0, gy)
            if tx0 > tx1 or ty0 > ty1:
                continue
            tx0, tx1, ty0, ty1 = int(tx0), int(tx1), int(ty0), int(ty1)
            lo_x[ty0:ty1 + 1] = np.minimum(lo_x[ty0:ty1 + 1], tx0); hi_x[ty0:ty1 + 1] = np.maximum(hi_x[ty0:ty1 + 1], tx1)
    kept = np.zeros((gy, gx), bool)
    for r in range(gy):
        if hi_x[r] >= lo_x[r]:
            kept[r, lo_x[r]:hi_x[r] + 1] = True
    return kept


KINDS = ["front", "to_zero", "through_zero", "behind"]


def slab(kind, rng, W, H, focal):
    """One or two long flat boxes, a floor or a ceiling that runs towards the horizon: thin in y and off the axis, narrower than the frame
    where it is near, long in z.  front: z from near to far; to_zero: a z bound of exactly 0; through_zero: z from behind the origin to far
    in front; behind: wholly at z < 0 (its mirror image is what the rays meet)."""
    n = int(rng.integers(1, 3))
    mn = np.empty((n, 3), np.float32); mx = np.empty((n, 3), np.float32)
    for k in range(n):
        near, far = float(rng.uniform(1.0, 8.0)), float(rng.uniform(200.0, 3000.0))
        half_w = float(rng.uniform(0.1, 0.45)) * W / focal * near * 4.0       # at 4 x near it spans 0.2 .. 0.9 of the frame's width
        cx = float(rng.uniform(-0.3, 0.3)) * half_w
        y = float(rng.choice([-1.0, 1.0])) * float(rng.uniform(0.15, 0.6)) * H / focal * near * 4.0
        th = float(rng.uniform(0.0, 0.02)) * abs(y)
        lo = np.array([cx - half_w, y - th, near]); hi = np.array([cx + half_w, y + th, far])
        if kind == "to_zero":
            lo[2] = 0.0
        elif kind == "through_zero":
            lo[2] = -float(rng.uniform(0.5, 100.0))
        elif kind == "behind":
            lo[2], hi[2] = -far, -near
            if rng.integers(0, 2): hi[2] = -0.0
        mn[k], mx[k] = lo.astype(np.float32), hi.astype(np.float32)
    return mn, mx


@pytest.mark.parametrize("kind", KINDS)
def test_slabs_towards_the_horizon(cli, kind):
    rng = np.random.default_rng(0x0071E + KINDS.index(kind))
    cases = []
    for (W, H) in ((96, 54), (200, 120)):
        for focal in (400.0, 60.0):
            cases += [(*slab(kind, rng, W, H, focal), W, H, focal) for _ in range(10)]
    tables = ts.run_cases(cli, cases)
    n_kept = n_rect = 0
    for (mn, mx, W, H, focal), kept in zip(cases, tables):
        assert kept is not None, f"{kind}: a finite, ordered scene fell back"
        ts.assert_conservative(kept, mn, mx, W, H, focal, kind)
        rect = rect_rule(mn, mx, W, H, focal)
        assert not (kept & ~rect).any(), f"{kind}: keeps a tile the one-rectangle rule excludes"
        n_kept += int(kept.sum()); n_rect += int(rect.sum())
    print(f"{kind}: kept {n_kept}, one rectangle {n_rect}")
    assert n_kept < n_rect, f"{kind}: {n_kept} kept tiles, the one-rectangle rule keeps {n_rect}"


def test_slice_count_follows_the_object_count(cli):
    """32 slices up to 128 objects, one at the table's limit of 4096: the same slab, repeated, keeps the one rectangle's tiles (with the
    pixel margin) there and fewer below."""
    rng = np.random.default_rng(5)
    W, H, focal = 200, 120, 60.0
    mn, mx = slab("front", rng, W, H, focal)
    mn, mx = mn[:1], mx[:1]
    counts = [int(t.sum()) for t in ts.run_cases(cli, [(np.tile(mn, (n, 1)), np.tile(mx, (n, 1)), W, H, focal) for n in (1, 128, 1024, 4096)])]
    assert counts[0] == counts[1] <= counts[2] <= counts[3]
    assert counts[0] < counts[3] <= int(rect_rule(mn, mx, W, H, focal).sum())
