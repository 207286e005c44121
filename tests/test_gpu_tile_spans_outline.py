"""GPU (-m gpu): the tile spans that follow the boxes' outline (srt_tile_spans.h: z slices, a pixel of margin) on the device.

ground_bunny and cube_ground -- a slab that narrows towards the horizon under an object -- at 96x54 and 200x120, neither a multiple of the
tile.  At the reference's focal length of 400 the small frames lie inside the slab's projection; at 40 there is sky above it and
background beside it, so every case runs at both.  hit_id, t, rgb_linear and rgb8 are, bit for bit, the full grid's (variant 64) and the
oracle's: eager with and without SRT_FLAG_FRAMES_IN_FLIGHT here, captured and replayed -- and replayed after srt_scene_update has moved
the objects onto tiles the captured table excludes, where the captured launches must stop culling -- in
tests/tile_spans_outline_graph_case.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import test_gpu_tile_spans as base
import test_tile_spans as ts
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = ["ground_bunny", "cube_ground"]
SIZES = [(96, 54), (200, 120)]
FOCALS = [400.0, 40.0]

srt = base.srt
cli = ts.cli


@pytest.mark.parametrize("name", SCENES)
def test_eager_frames_equal_the_full_grid_and_the_oracle(srt, oracle, cli, name):
    g = gu.GoldenScene(name)
    mn, mx = ts.root_boxes(g.flat)
    ds = srt.DeviceScene(g.flat)
    excluded = 0
    for (W, H) in SIZES:
        for focal in FOCALS:
            c = oracle.render(g.flat, g.params(W, H, 1, focal=focal), pow="device")
            (kept,) = ts.run_cases(cli, [(mn, mx, W, H, focal)])
            assert kept is not None
            excluded += int((~kept).sum())
            for hint in (0, abi.SRT_FLAG_FRAMES_IN_FLIGHT):      # four waves per tile / the half-tile form
                p = g.params(W, H, 1, focal=focal, flags=hint)
                what = f"{name} {W}x{H} focal {focal} flags={hint}"
                o = base.shipped_and_full(srt, ds, p, what)
                gf.compare_exact(srt, o, c, gf.owned(p), g.flat, p, what)
                # the frame agrees with the table the host made for it: no hit in an excluded tile
                hit = np.zeros((kept.shape[0] * 8, kept.shape[1] * 8), bool); hit[:H, :W] = o["hit_id"] >= 0
                assert not (hit.reshape(kept.shape[0], 8, kept.shape[1], 8).any(axis=(1, 3)) & ~kept).any(), what
    assert excluded > 0, "no frame of this scene had an excluded tile: the table was never used"
    ds.close()


def test_captured_frames_replay_and_follow_the_scene_onto_excluded_tiles(cli, tmp_path):
    """Own process (torch initialises HIP first, as tests/test_gpu_graph_capture.py).  The tables of the frames it captures are made
    here, on the CPU, by tools/tile_spans_cli.cpp: the case asks that the moved scene has hits in tiles they exclude."""
    tables = {}
    for name in SCENES:
        mn, mx = ts.root_boxes(gu.GoldenScene(name).flat)
        for (W, H) in SIZES:
            for focal in FOCALS:
                (kept,) = ts.run_cases(cli, [(mn, mx, W, H, focal)])
                assert kept is not None
                tables[f"{name}_{W}_{H}_{int(focal)}"] = kept
    path = str(tmp_path / "tables.npz")
    np.savez(path, **tables)
    r = subprocess.run([sys.executable, os.path.join(HERE, "tile_spans_outline_graph_case.py"), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "tile spans outline graph case: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
