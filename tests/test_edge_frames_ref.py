"""The inputs of tests/test_gpu_trace_edges.py (tests/edge_frames.py) are what they are named, on the CPU: by the oracle's frames, by the
span table tools/tile_spans_cli.cpp makes (tests/test_tile_spans.py's cli) and by the reference's slab test (its judge)."""
import numpy as np
import pytest

import edge_frames as ef
import golden_util as gu
import test_tile_spans as ts
import wave8_scenes as w8

cli = ts.cli


def with_shadow_div(p, div):
    q = type(p).from_buffer_copy(p)
    q._lights = p._lights
    q.shadow_div = div
    return q


def test_the_shapes_are_the_ones_named():
    assert len(ef.SHAPES) == len(set(ef.SHAPES)) == 22
    assert {H % 8 for (W, H) in ef.SHAPES} == set(range(8)), "the last tile row is cut at every remainder"
    assert {1, 3, 6, 7} <= {W % 8 for (W, H) in ef.SHAPES}, "the right-hand remainders no other test has"
    assert {(W + 7) // 8 for (W, H) in ef.SHAPES} >= {1, 2, 3, 8, 9, 16, 17}, "one tile, one group of eight, nine, two groups, three"
    assert ef.OFFSET_SHAPES == [(W, H) for (W, H) in ef.SHAPES if (W + 7) // 8 >= 16]


@pytest.mark.parametrize("name", ef.GOLDEN)
def test_every_view_has_a_hit_and_a_miss_where_promised(oracle, name):
    g = gu.GoldenScene(name)
    for (W, H) in ef.SHAPES:
        c = oracle.render(g.flat, ef.edge_view(name, W, H)(1))
        hit = c["hit_id"] >= 0
        if (name, (W, H)) in ef.NO_HIT_POSSIBLE:
            # one row: j0 = 0, every ray lies in the plane y = 0, and no root box of the scene reaches it -- at any focal length
            assert H == 1 and int(-np.float32(H) / 2) == 0
            mn, mx = ts.root_boxes(g.flat)
            assert ((mn[:, 1] > 0) | (mx[:, 1] < 0)).all() and not hit.any()
            continue
        assert hit.any(), f"{name} {W}x{H}: no hit"
        if W * H > 64:
            assert (~hit).any(), f"{name} {W}x{H}: no miss"
    assert ef.NO_HIT_POSSIBLE == {("cubes4_a40", s) for s in ef.SHAPES if s[1] == 1}


def test_a_dead_lower_half_exactly_where_the_last_tile_row_is_cut_at_or_above_its_middle():
    for (W, H) in ef.SHAPES + ef.GRID_SHAPES:
        live = w8.half_tiles(np.ones((H, W), bool))
        assert live[:-1].all() and live[-1, 0].all(), "every half but the last row's lower one holds a pixel"
        assert (not live[-1, 1].any()) == (H % 8 in (1, 2, 3, 4)), (W, H)
        assert live[-1, 1].all() or not live[-1, 1].any()


def test_the_offset_spans_start_off_a_group_and_cross_into_the_next(oracle, cli):
    flat, _ = ef.offset_scene()
    mn, mx = ts.root_boxes(flat)
    tables = ts.run_cases(cli, [(mn, mx, W, H, ef.OFFSET_FOCAL) for (W, H) in ef.OFFSET_SHAPES])
    for (W, H), kept in zip(ef.OFFSET_SHAPES, tables):
        assert kept is not None, "the offset scene has a table"
        ts.assert_conservative(kept, mn, mx, W, H, ef.OFFSET_FOCAL, f"offset {W}x{H}")
        x0, n = ef.OFFSET_SPANS[(W, H)]
        assert x0 % 8 != 0 and x0 + n > 8 * (x0 // 8 + 1), "off a group's first tile, and over the group's end"
        c = oracle.render(flat, ef.offset_view(W, H)(1))
        hit = w8.half_tiles(c["hit_id"] >= 0).any(axis=1)      # (tile rows, tile columns)
        for row in range(kept.shape[0]):
            cols = np.flatnonzero(kept[row])
            assert (int(cols[0]), len(cols)) == (x0, n) and (np.diff(cols) == 1).all(), f"{W}x{H} tile row {row}: span {cols[0]}:{len(cols)}"
        assert hit[0, x0] and hit[0, x0 + n - 1], f"{W}x{H}: the first and the last tile of the span hold hits"
        assert set(np.unique(flat.tri_obj[c["hit_id"][c["hit_id"] >= 0]])) == {0, 1}
        lit = oracle.render(flat, with_shadow_div(ef.offset_view(W, H)(1), 1.0))
        assert (ef.bits(lit["rgb_linear"]) != ef.bits(c["rgb_linear"])).any(), "the chip shadows the wall"


@pytest.mark.parametrize("n", ef.OBJECT_COUNTS)
def test_the_object_grids(oracle, n):
    flat, _ = ef.object_grid(n)
    assert flat.n_objects == n
    n_tris = np.bincount(flat.tri_obj, minlength=n)
    assert list(n_tris) == [2 + 2 * (k % 2) for k in range(n)], "alternately 2 and 4 triangles"
    for (W, H) in ef.GRID_SHAPES:
        view = ef.grid_view(n, W, H)
        c = oracle.render(flat, view(1), pow="device")      # (as shadowed_by_last renders its frame)
        hit = c["hit_id"] >= 0
        seen = np.unique(flat.tri_obj[c["hit_id"][hit]])
        assert list(seen) == list(range(n)), f"n {n} {W}x{H}: objects seen {seen}"      # (the last, and for n >= 32 object 31, among them)
        assert n - 1 in seen and (n < 32 or 31 in seen)
        assert (~hit).any(), "a rim of background"
        passes = ef.root_passes_by_object(ts, flat, W, H, ef.grid_focal(n, W, H))
        assert not (hit & ~passes.any(0)).any()
        if n > 1:
            assert (passes.sum(0) >= 2).any(), "neighbours overlap on screen: some ray passes two root boxes"
        groups = np.stack([passes[g:g + 6].any(0) for g in range(0, n, 6)])      # the root groups of a one-wave workgroup: six objects each
        if n > 6:
            assert (groups.sum(0) >= 2).any(), f"n {n} {W}x{H}: no ray passes root boxes of two groups of six"
            assert (groups[-1] & groups[:-1].any(0)).any(), "... the last group among them"
        if n > 1:      # (one object shadows nothing: a hit's own object is skipped)
            lit = oracle.render(flat, with_shadow_div(view(1), 1.0), pow="device")
            depends = (ef.bits(lit["rgb_linear"]) != ef.bits(c["rgb_linear"])).any(-1)
            by_last = ef.shadowed_by_last(oracle, n, W, H, c)
            assert (depends & by_last).any(), f"n {n} {W}x{H}: the last object shadows no pixel"
            assert not (by_last & ~depends).any()
            if n >= 12 and (W, H) == (64, 40):
                assert (depends & ~by_last).any(), "nearer rectangles shadow farther ones, not the last alone"


def test_the_moved_scenes_change_every_hit(oracle):
    """tests/trace_edges_graph_case.py: the moved scene differs in t wherever both frames have a hit."""
    for flat, view in ((gu.GoldenScene("cubes4_a40").flat, ef.edge_view("cubes4_a40", 24, 35)), (ef.object_grid(33)[0], ef.grid_view(33, 24, 35))):
        a, b = oracle.render(flat, view(1)), oracle.render(ef.moved(flat), view(1))
        both = (a["hit_id"] >= 0) & (b["hit_id"] >= 0)
        assert both.any() and (ef.bits(a["t"])[both] != ef.bits(b["t"])[both]).all()
