"""Run by tests/test_gpu_trace_edges.py in its own process (torch initialises HIP first), once per scene: the trace kernels of frames in
flight captured into a hipGraph at the edge shapes of tests/edge_frames.py.  A captured launch keeps the frame's WHOLE grid -- for the
one-wave workgroups padded to groups of eight tiles and doubled, so that a frame of one pixel launches sixteen workgroups of which one
works --, reads a table whose rows count from tile row 0, and culls only while the records' epoch word is the table's.

Scenes: cubes4_a40 (a wave's own root pass), and the 32- and 33-object grids (the last count with a root pass, the first on the queue
path).  Shapes: 1 x 1, 7 x 3, 9 x 3, 24 x 35, 65 x 12 and 129 x 9.  Builds: the shipped choice under SRT_FLAG_FRAMES_IN_FLIGHT and variant
68 at 1 and 4 light samples (the whole-frame kernels, the general frame's one-wave workgroups), the shipped choice at 5 (two waves a tile).

    eager -> captured -> replay -> srt_scene_update to the moved scene, replay -> srt_scene_update back, replay

every frame bit for bit variant 59's eager frame of the scene the records hold at that moment (tests/trace_half_eight_graph_case.py,
one_case).  The moved scene (edge_frames.moved: away from the camera as well as aside) renders another frame at every shape but 1 x 1,
or the replays after the updates test nothing."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, build, lib      # noqa: E402
import edge_frames as ef                       # noqa: E402
import golden_util as gu                       # noqa: E402
import gpu_frames as gf                        # noqa: E402
import trace_half_eight_graph_case as eight    # noqa: E402

SHAPES = [(1, 1), (7, 3), (9, 3), (24, 35), (65, 12), (129, 9)]
V_FOUR_WAVES, V_GENERAL = 59, 68
BUILDS = [(1, ef.IN_FLIGHT), (1, ef.IN_FLIGHT | V_GENERAL << 8), (4, ef.IN_FLIGHT), (4, ef.IN_FLIGHT | V_GENERAL << 8), (5, ef.IN_FLIGHT)]
FUSED = "k_trace_nq+k_shade_tile"


def scene_and_views(name):
    """(flat scene, view(W, H) -> params(L, flags))"""
    if name == "cubes4_a40":
        return gu.GoldenScene(name).flat, lambda W, H: ef.edge_view(name, W, H)
    n = {"grid32": 32, "grid33": 33}[name]
    return ef.object_grid(n)[0], lambda W, H: ef.grid_view(n, W, H)


def main(name):
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    build.build_host()
    flat, views = scene_and_views(name)
    moved = ef.moved(flat)
    n = 0
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):      # (a stream of the case's own: see tests/tile_spans_outline_graph_case.py)
        ds, four = lib.DeviceScene(flat), lib.DeviceScene(flat)
        for (W, H) in SHAPES:
            view = views(W, H)
            for L in sorted({L for L, _ in BUILDS}):
                want = {}
                for key, scene in (("created", flat), ("moved", moved)):
                    four.update(scene)
                    want[key] = four.render(view(L, ef.IN_FLIGHT | V_FOUR_WAVES << 8))
                    assert four.pipeline == FUSED
                differ = any(not np.array_equal(gf.bits(want["created"][k]), gf.bits(want["moved"][k])) for k in ("t", "rgb_linear"))
                assert differ or (W, H) == (1, 1), f"{name} {W}x{H} L{L}: the moved scene renders the same frame"
                for flags in (f for l, f in BUILDS if l == L):
                    eight.one_case(dev, ds, view(L, abi.SRT_FLAG_NO_TIMING | flags), want, flat, moved, f"{name} {W}x{H} L{L} flags {flags:#x}")
                    n += 1
        ds.close(); four.close()
    assert n == len(SHAPES) * len(BUILDS)
    print(f"trace edges graph case {name}: ok")


if __name__ == "__main__":
    main(sys.argv[1])
