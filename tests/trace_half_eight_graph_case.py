"""Run by tests/test_gpu_trace_half_eight.py in its own process (torch initialises HIP first): the half-tile trace kernel's eight-wave
builds over the tile spans (k_trace_nq_half8_spans, srt_kernels.h), captured into a hipGraph and replayed.  For the shipped choice with
SRT_FLAG_FRAMES_IN_FLIGHT (the eight-wave build, 384 queue entries), variant 65 (the seven-wave build) and variant 66 (eight waves, 256
entries), on every scene of the test at 1 and 4 light samples:

    eager -> captured -> replay -> srt_scene_update to the moved scene, replay -> srt_scene_update back, replay

Every frame is compared, bit for bit in hit_id, t, rgb_linear and rgb8, with variant 59's eager frame -- four waves per tile on the full
grid -- of the scene the records hold at that moment, rendered from records of its own."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, build, host, lib      # noqa: E402
import gpu_frames as gf                        # noqa: E402
import pose_ref                                # noqa: E402
import half_eight_scenes as he                 # noqa: E402
import test_gpu_trace_half_seven as seven      # noqa: E402

IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
V_FOUR_WAVES, V_SEVEN_WAVES, V_EIGHT_WAVES_256 = 59, 65, 66
BUILDS = (0, V_SEVEN_WAVES, V_EIGHT_WAVES_256)
LIGHTS = (1, 4)
OUTPUTS = ("hit_id", "t", "rgb_linear", "rgb8")


def cases():
    """(name, flat scene, params(W, H, L, flags), shapes)"""
    for name in ("cubes4_a40", "soup12"):
        flat, params, _ = seven.scene(lib, name)
        yield name, flat, params, seven.SHAPES
    flat, _ = he.grid40_scene()      # (forty objects that the shipped choice traces: the 40-object soup goes to the packet kernels)
    yield "grid40", flat, he.grid40_params, seven.SHAPES
    flat, _ = he.flat_scene()
    yield "fans", flat, lambda W, H, L, flags=0: he.params(L, flags), [(he.W, he.H)]


def moved_scene(flat):
    """Every object a few pixels' worth to the side and up, at the scene's own scale."""
    mn, mx = flat.node_min[flat.obj_root.astype(np.int64)], flat.node_max[flat.obj_root.astype(np.int64)]
    full = mn[:, 0] <= mx[:, 0]
    span = float((mx[full] - mn[full])[:, :2].max())
    mats = np.tile(np.asarray(host.Transformation.changeObjPosition(0.02 * span, -0.015 * span, 0.0), np.float32).reshape(1, 16), (flat.n_objects, 1))
    return pose_ref.pose_flat(flat, mats)


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    build.build_host()
    n = 0
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):      # (a stream of the case's own: see tests/tile_spans_outline_graph_case.py)
        for name, flat, params, shapes in cases():
            moved = moved_scene(flat)
            ds, four = lib.DeviceScene(flat), lib.DeviceScene(flat)
            for (W, H) in shapes:
                for L in LIGHTS:
                    want = {}
                    for key, scene in (("created", flat), ("moved", moved)):
                        four.update(scene)
                        want[key] = four.render(params(W, H, L, flags=IN_FLIGHT | V_FOUR_WAVES << 8))
                        assert four.pipeline == seven.FUSED
                    differ = any(not np.array_equal(gf.bits(want["created"][k]), gf.bits(want["moved"][k])) for k in ("t", "rgb_linear"))
                    assert differ, f"{name} {W}x{H} L{L}: the moved scene renders the same frame"
                    for v in BUILDS:
                        one_case(dev, ds, params(W, H, L, flags=abi.SRT_FLAG_NO_TIMING | IN_FLIGHT | v << 8), want, flat, moved, f"{name} {W}x{H} L{L} variant {v}")
                        n += 1
            ds.close(); four.close()
    assert n == (3 * len(seven.SHAPES) + 1) * len(LIGHTS) * len(BUILDS)
    print("trace half eight graph case: ok")


def one_case(dev, ds, p, want, created, moved, name):
    W, H = p.width, p.height
    hit = torch.full((H, W), -5, dtype=torch.int32, device=dev); t = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    lin = torch.full((H, W, 3), 9.0, dtype=torch.float32, device=dev); rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev)
    def frame():
        ds.render_device(p, stream=torch.cuda.current_stream().cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(), rgb8=rgb8.data_ptr())
        assert ds.pipeline == seven.FUSED, (name, ds.pipeline)
    def check(key, what):
        what = f"{name}: {what}"
        torch.cuda.synchronize()
        o = {"hit_id": hit.cpu().numpy(), "t": t.cpu().numpy(), "rgb_linear": lin.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}
        f = want[key]
        assert np.array_equal(o["hit_id"], f["hit_id"]), (what, "hit ids")
        for k in ("t", "rgb_linear"):
            assert np.array_equal(gf.bits(o[k]), gf.bits(f[k])), (what, k)
        assert np.array_equal(o["rgb8"], f["rgb8"]), (what, "rgb8")
        hit.fill_(-5); t.fill_(7.0); lin.fill_(9.0); rgb8.fill_(77)
    cur = torch.cuda.current_stream().cuda_stream
    assert cur != 0
    frame(); frame(); check("created", "eager")
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        frame(); frame()                                        # (an even number of renders per graph: the two counter sets stay in step)
    gph.replay(); check("created", "replay, nothing moved")
    ds.update(moved, stream=cur); gph.replay(); check("moved", "replay after srt_scene_update to the moved scene")
    ds.update(created, stream=cur); gph.replay(); check("created", "replay after srt_scene_update back")


if __name__ == "__main__":
    main()
