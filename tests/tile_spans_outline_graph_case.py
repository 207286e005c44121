"""Run by tests/test_gpu_tile_spans_outline.py in its own process (torch initialises HIP first): frames with tile spans captured into a
hipGraph and replayed.  The table travels in the captured kernel nodes' arguments, and the captured launches cull by it only while the
records' box epoch is still the table's.  Every replay is compared, bit for bit, with the oracle's frame of the scene the records hold
at that moment and with the eager frame on the full grid (variant 64):

    replay, nothing moved -> srt_scene_update to the moved scene, replay -> srt_scene_update back, replay

argv[1]: an .npz of the captured frames' tables (kept tiles, made on the CPU by the test): at focal 40 the moved scene must have hits in
tiles the captured table excludes, or the case tests nothing."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, build, host, lib      # noqa: E402
from oracle import pyoracle as oracle          # noqa: E402
import golden_util as gu                       # noqa: E402
import gpu_frames as gf                        # noqa: E402
import pose_ref                                # noqa: E402

SCENES = ["ground_bunny", "cube_ground"]
SIZES = [(96, 54), (200, 120)]
FOCALS = [400.0, 40.0]
FULL_GRID = 64 << 8
MOVE_Y = -90.0       # every object, along y: the slab's far edge crosses the horizon rows the captured table leaves out


def main():
    tables = np.load(sys.argv[1])
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    oracle.oracle_lib(); build.build_host()
    # A stream of the case's own for the updates, the eager frames and the replays: srt_scene_update on the null stream means the scene's
    # own (non-blocking) stream, and a replay on the null stream would not wait for its copies.
    with torch.cuda.stream(torch.cuda.Stream(device=dev)):
        n_cases = sum(scene_cases(dev, name, tables) for name in SCENES)
    assert n_cases == 16
    print("tile spans outline graph case: ok")


def scene_cases(dev, name, tables):
    g = gu.GoldenScene(name)
    mats = np.tile(np.asarray(host.Transformation.changeObjPosition(0.0, MOVE_Y, 0.0), np.float32).reshape(1, 16), (g.flat.n_objects, 1))
    moved = pose_ref.pose_flat(g.flat, mats)
    ds = lib.DeviceScene(g.flat)
    full = lib.DeviceScene(g.flat)      # the eager frames on the full grid, from records of their own
    n_cases = 0
    for (W, H) in SIZES:
        for focal in FOCALS:
            kept = tables[f"{name}_{W}_{H}_{int(focal)}"]
            want = {}
            for key, flat in (("created", g.flat), ("moved", moved)):
                full.update(flat)
                want[key] = (oracle.render(flat, abi.make_params(W, H, abi.light_staircase(g.light, 1), focal=focal, flags=abi.SRT_FLAG_NO_TIMING), pow="device"),
                             full.render(abi.make_params(W, H, abi.light_staircase(g.light, 1), focal=focal, flags=FULL_GRID)))
            hit_tiles = np.zeros((kept.shape[0] * 8, kept.shape[1] * 8), bool); hit_tiles[:H, :W] = want["moved"][0]["hit_id"] >= 0
            outside = int((hit_tiles.reshape(kept.shape[0], 8, kept.shape[1], 8).any(axis=(1, 3)) & ~kept).sum())
            if focal == 40.0:
                assert outside > 0, f"{name} {W}x{H}: the moved scene has no hit in a tile the captured table excludes"
            for hint in (0, abi.SRT_FLAG_FRAMES_IN_FLIGHT):      # four waves per tile / the half-tile form
                p = abi.make_params(W, H, abi.light_staircase(g.light, 1), focal=focal, flags=abi.SRT_FLAG_NO_TIMING | hint)
                one_case(dev, ds, p, want, g.flat, moved, f"{name} {W}x{H} focal {focal} flags={hint}", outside)
                n_cases += 1
    ds.close(); full.close()
    return n_cases


def one_case(dev, ds, p, want, created, moved, name, outside):
    W, H = p.width, p.height
    hit = torch.full((H, W), -5, dtype=torch.int32, device=dev); t = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    lin = torch.full((H, W, 3), 9.0, dtype=torch.float32, device=dev); rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev)
    def frame():
        ds.render_device(p, stream=torch.cuda.current_stream().cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(), rgb8=rgb8.data_ptr())
    def check(key, flat, what):
        what = f"{name}: {what}"
        torch.cuda.synchronize()
        o = {"hit_id": hit.cpu().numpy(), "t": t.cpu().numpy(), "rgb_linear": lin.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}
        c, f = want[key]
        o["stats"] = c["stats"]
        gf.compare_exact(lib, o, c, gf.owned(p), flat, p, what)
        assert np.array_equal(o["hit_id"], f["hit_id"]), (what, "hit ids, full grid")
        for k in ("t", "rgb_linear"):
            assert np.array_equal(gf.bits(o[k]), gf.bits(f[k])), (what, k, "full grid")
        assert np.array_equal(o["rgb8"], f["rgb8"]), (what, "rgb8, full grid")
        hit.fill_(-5); t.fill_(7.0); lin.fill_(9.0); rgb8.fill_(77)
    cur = torch.cuda.current_stream().cuda_stream
    assert cur != 0
    frame(); frame(); check("created", created, "eager")
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        frame(); frame()                                        # (an even number of renders per graph: the two counter sets stay in step)
    gph.replay(); check("created", created, "replay, nothing moved")
    ds.update(moved, stream=cur); gph.replay()
    check("moved", moved, f"replay after srt_scene_update to the moved scene ({outside} hit tiles outside the captured table)")
    ds.update(created, stream=cur); gph.replay(); check("created", created, "replay after srt_scene_update back")


if __name__ == "__main__":
    main()
