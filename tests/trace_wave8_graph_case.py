"""Run by tests/test_gpu_trace_wave8.py in its own process (torch initialises HIP first): the one-wave trace workgroups over the tile spans
(k_trace_nq_wave8_spans, srt_kernels.h), captured into a hipGraph and replayed.  A captured launch keeps the frame's whole grid -- here twice
as wide as the tiles, padded to groups of eight -- and culls only while the records' epoch word is the table's.  For the shipped choice with
SRT_FLAG_FRAMES_IN_FLIGHT, for variant 31 (the same kernel without the hint) and for variant 32 (the other dispatch order, a tile's halves
next to each other and no padding), at 1 and 4 light samples:

    eager -> captured -> replay -> srt_scene_update to the moved scene, replay -> srt_scene_update back, replay

After the update the epoch differs, and the workgroups outside the captured spans do their tiles' whole work, both halves.  Every frame is
compared, bit for bit in hit_id, t, rgb_linear and rgb8, with variant 59's eager frame -- four waves per tile on the full grid -- of the
scene the records hold at that moment, rendered from records of its own.  Scenes: cubes4_a40 (the wave's own root pass), grid40 (more than
32 objects: the queue path), the ledge (half tiles that pass no root), fans (queue overflow); 37 x 29, 64 x 40 and 40 x 36, where the last
tile row's lower halves have no live pixel."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, build, lib      # noqa: E402
import half_eight_scenes as he                 # noqa: E402
import test_gpu_trace_half_seven as seven      # noqa: E402
import trace_half_eight_graph_case as eight    # noqa: E402
import wave8_scenes as w8                      # noqa: E402

BUILDS = (w8.IN_FLIGHT, w8.V_WAVE_8 << 8, w8.IN_FLIGHT | w8.V_ADJACENT << 8)


def cases():
    """(name, flat scene, params(W, H, L, flags), shapes)"""
    flat, params, _ = seven.scene(lib, "cubes4_a40")
    yield "cubes4_a40", flat, params, w8.SHAPES
    flat, _ = he.grid40_scene()
    yield "grid40", flat, he.grid40_params, [w8.SHAPES[0], w8.SHAPES[2]]
    flat, _ = w8.ledge_scene()
    yield "ledge", flat, w8.ledge_params, [(w8.LEDGE_W, w8.LEDGE_H)]
    flat, _ = he.flat_scene()
    yield "fans", flat, lambda W, H, L, flags=0: he.params(L, flags), [(he.W, he.H)]


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    build.build_host()
    n = 0
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):      # (a stream of the case's own: see tests/tile_spans_outline_graph_case.py)
        for name, flat, params, shapes in cases():
            moved = eight.moved_scene(flat)
            ds, four = lib.DeviceScene(flat), lib.DeviceScene(flat)
            for (W, H) in shapes:
                for L in w8.LIGHTS:
                    want = {}
                    for key, scene in (("created", flat), ("moved", moved)):
                        four.update(scene)
                        want[key] = four.render(params(W, H, L, flags=w8.IN_FLIGHT | w8.V_FOUR_WAVES << 8))
                        assert four.pipeline == seven.FUSED
                    differ = any(not np.array_equal(eight.gf.bits(want["created"][k]), eight.gf.bits(want["moved"][k])) for k in ("t", "rgb_linear"))
                    assert differ, f"{name} {W}x{H} L{L}: the moved scene renders the same frame"
                    for flags in BUILDS:
                        eight.one_case(dev, ds, params(W, H, L, flags=abi.SRT_FLAG_NO_TIMING | flags), want, flat, moved, f"{name} {W}x{H} L{L} flags {flags:#x}")
                        n += 1
            ds.close(); four.close()
    assert n == (3 + 2 + 1 + 1) * len(w8.LIGHTS) * len(BUILDS)
    print("trace wave8 graph case: ok")


if __name__ == "__main__":
    main()
