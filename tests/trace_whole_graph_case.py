"""Run by tests/test_gpu_trace_whole.py in its own process (torch initialises HIP first): the whole-frame trace and shading kernels
(k_trace_nq_whole8_spans, k_shade_tile_whole_spans, srt_kernels.h) captured into a hipGraph and replayed.  A captured launch keeps the
frame's whole grid and culls only while the records' epoch word is the table's -- the word the whole-frame prologue reads through a pointer
it has taken through a register.  For the shipped choice with SRT_FLAG_FRAMES_IN_FLIGHT and for variant 68 (the general frame's kernels
in their place), at 1 and 4 light samples:

    eager -> captured -> replay -> srt_scene_update to the moved scene, replay -> srt_scene_update back, replay

every frame bit for bit variant 59's eager frame of the scene the records hold at that moment (tests/trace_half_eight_graph_case.py).

Then the frames the whole-frame kernels do not fit, which must keep the kernels they had: a split frame (scanline blocks, and column
tiles), camera mode, spp = 4 and a scene whose boxes have changed on the device only.  Variant 0 and variant 68 name the same pipeline
there and give the same bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, build, host, lib      # noqa: E402
import half_eight_scenes as he                 # noqa: E402
import test_gpu_trace_half_seven as seven      # noqa: E402
import trace_half_eight_graph_case as eight    # noqa: E402
import wave8_scenes as w8                      # noqa: E402
import whole_scenes as ws                      # noqa: E402

BUILDS = (w8.IN_FLIGHT, w8.IN_FLIGHT | ws.V_GENERAL << 8)


def cases():
    """(name, flat scene, params(W, H, L, flags), shapes)"""
    flat, params, _ = seven.scene(lib, "cubes4_a40")
    yield "cubes4_a40", flat, params, w8.SHAPES
    flat, _ = he.grid40_scene()
    yield "grid40", flat, he.grid40_params, [w8.SHAPES[2]]
    flat, _ = w8.ledge_scene()
    yield "ledge", flat, w8.ledge_params, [(w8.LEDGE_W, w8.LEDGE_H)]
    flat, _ = he.flat_scene()
    yield "fans", flat, lambda W, H, L, flags=0: he.params(L, flags), [(he.W, he.H)]
    yield "leaves", ws.leaves_scene(), ws.params, [w8.SHAPES[0], w8.SHAPES[2]]


def kept_kernels():
    """Frames that are not whole frames in the reference's ray form: 0 and 68 are the same launches."""
    flat, _, _ = seven.scene(lib, "cubes4_a40")
    lights = lambda L: abi.light_staircase(seven.gu.GoldenScene("cubes4_a40").light, L)
    W, H = 40, 36
    focal = seven.focal("cubes4_a40", W, H)
    shift = np.asarray(host.Transformation.changeObjPosition(3.0, -2.0, 1.0), np.float32).reshape(16)
    frames = {"scanline blocks": dict(block_rows=8, block_first=1, block_stride=2),
              "column tiles": dict(block_rows=8, block_cols=8, block_first=1, block_stride=2),
              "camera mode": dict(ray_matrix=shift),
              "spp 4": dict(spp=4)}
    ds = lib.DeviceScene(flat)
    n = 0
    def pair(what, **kw):
        nonlocal n
        for L in w8.LIGHTS:
            out = []
            for flags in BUILDS:
                out.append((ds.render(abi.make_params(W, H, lights(L), focal=focal, flags=flags, **kw)), ds.pipeline))
            assert out[0][1] == out[1][1], (what, out[0][1], out[1][1])
            seven.same_bits(out[0][0], out[1][0], f"{what} L{L}: variant 0 against 68")
            n += 1
    for what, kw in frames.items():
        pair(what, **kw)
    ds.set_pose_source()
    ds.pose(np.tile(np.asarray(host.Transformation.changeObjPosition(4.0, 2.0, 0.0), np.float32).reshape(1, 16), (flat.n_objects, 1)))
    pair("boxes changed on the device only")
    ds.close()
    assert n == 5 * len(w8.LIGHTS)


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
    assert n == (3 + 1 + 1 + 1 + 2) * len(w8.LIGHTS) * len(BUILDS)
    kept_kernels()
    print("trace whole graph case: ok")


if __name__ == "__main__":
    main()
