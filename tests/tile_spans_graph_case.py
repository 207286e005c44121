"""Run by tests/test_gpu_tile_spans.py in its own process (torch initialises HIP first): two whole frames with tile spans on two forked
streams, captured into one hipGraph and replayed -- the table is part of the captured kernel nodes' arguments -- against the eager
frames, bit for bit, and against the full grid (variant 64)."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("cube")
    W, H, B = 100, 52, 2
    first = lib.DeviceScene(g.flat)
    handles = [first, first.share()]
    def params(f, extra=0):
        light = g.light.copy(); light[0] += 40.0 * f
        return abi.make_params(W, H, abi.light_staircase(light, 2), focal=40.0, flags=abi.SRT_FLAG_NO_TIMING | abi.SRT_FLAG_FRAMES_IN_FLIGHT | extra)
    eager = []
    for f in range(B):
        o = lib.DeviceScene(g.flat).render(params(f, 64 << 8))
        assert (o["hit_id"] >= 0).any() and (o["hit_id"] < 0).any()
        eager.append(o)
    hit = [torch.full((H, W), -5, dtype=torch.int32, device=dev) for _ in range(B)]
    t = [torch.full((H, W), 7.0, dtype=torch.float32, device=dev) for _ in range(B)]
    lin = [torch.full((H, W, 3), 9.0, dtype=torch.float32, device=dev) for _ in range(B)]
    rgb8 = [torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev) for _ in range(B)]
    ps = [params(f) for f in range(B)]
    side = [torch.cuda.Stream(device=dev) for _ in range(2)]
    def frames():
        c = torch.cuda.current_stream()
        for st in side:
            st.wait_stream(c)
        for f in range(B):
            handles[f].render_device(ps[f], stream=side[f].cuda_stream, hit_id=hit[f].data_ptr(), t=t[f].data_ptr(), rgb_linear=lin[f].data_ptr(), rgb8=rgb8[f].data_ptr())
        for st in side:
            c.wait_stream(st)
    def check(what):
        torch.cuda.synchronize()
        for f in range(B):
            assert np.array_equal(hit[f].cpu().numpy(), eager[f]["hit_id"]), (what, f, "hit ids")
            assert np.array_equal(t[f].cpu().numpy().view(np.uint32), eager[f]["t"].view(np.uint32)), (what, f, "t")
            assert np.array_equal(lin[f].cpu().numpy().view(np.uint32), eager[f]["rgb_linear"].view(np.uint32)), (what, f, "linear")
            assert np.array_equal(rgb8[f].cpu().numpy(), eager[f]["rgb8"]), (what, f, "rgb8")
            hit[f].fill_(-5); t[f].fill_(7.0); lin[f].fill_(9.0); rgb8[f].fill_(77)
    frames(); check("eager, spans on")
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        frames()
    for rep in range(2):
        gph.replay(); check(f"replay {rep}")
    follow_the_scene(dev, g, W, H)
    captured_refit_then_eager_frame(dev, g, W, H)
    print("tile spans graph case: ok")


def captured_refit_then_eager_frame(dev, g, W, H):
    """The reverse order: a CAPTURED srt_scene_refit_device moves the object out of the spans at every replay, with no host code running.
    Capture it, upload the created scene again (the host's copy of the boxes is valid again), replay, render EAGERLY: the frame is the
    moved scene's -- records whose boxes a graph can change get no tile spans."""
    from oracle import pyoracle as oracle
    from simple_raytracer_amd import build, host
    import gpu_frames as gf
    import pose_ref
    import refit_ref
    oracle.oracle_lib(); build.build_host()
    T = host.Transformation
    p = abi.make_params(W, H, abi.light_staircase(g.light, 2), focal=40.0, flags=abi.SRT_FLAG_NO_TIMING)
    r = int(g.flat.obj_root[0])
    z = 0.5 * float(g.flat.node_min.reshape(-1, 3)[r][2] + g.flat.node_max.reshape(-1, 3)[r][2])
    mats = np.eye(4, dtype=np.float32).reshape(1, 16).copy(); mats[0] = T.changeObjPosition(30.0 * z / 40.0, 0.0, 0.0)
    pts = np.ascontiguousarray(pose_ref.transform_objects(g.flat, mats), np.float32).reshape(-1, 3, 4)
    moved = refit_ref.refit_flat(g.flat, pts)
    d_pts = torch.from_numpy(pts.reshape(-1, 4).copy()).to(dev)
    ds = lib.DeviceScene(g.flat); ds.refit_prepare()
    hit = torch.full((H, W), -5, dtype=torch.int32, device=dev); t = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    lin = torch.full((H, W, 3), 9.0, dtype=torch.float32, device=dev); rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev)
    def eager(flat, what):
        ds.render_device(p, stream=torch.cuda.current_stream().cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(), rgb8=rgb8.data_ptr())
        torch.cuda.synchronize()
        o = {"hit_id": hit.cpu().numpy(), "t": t.cpu().numpy(), "rgb_linear": lin.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}
        c = oracle.render(flat, p, pow="device")
        o["stats"] = c["stats"]
        gf.compare_exact(lib, o, c, gf.owned(p), flat, p, what)
        hit.fill_(-5); t.fill_(7.0); lin.fill_(9.0); rgb8.fill_(77)
        return o
    first = eager(g.flat, "eager, created scene")
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        ds.refit_device(points=d_pts.data_ptr(), stride=4, stream=torch.cuda.current_stream().cuda_stream)
    cur = torch.cuda.current_stream().cuda_stream
    ds.update(g.flat, stream=cur); ds.refit_prepare()            # (an update discards the preparation; the captured launches keep their arguments)
    eager(g.flat, "eager after the update")
    gph.replay()
    after = eager(moved, "eager after the replay of a captured refit")
    cols0 = np.nonzero((first["hit_id"] >= 0).any(axis=0))[0]; cols1 = np.nonzero((after["hit_id"] >= 0).any(axis=0))[0]
    assert cols1.max() > cols0.max() + 16, "the object did not leave the created scene's spans"
    ds.close()


def follow_the_scene(dev, g, W, H):
    """A captured render replayed after the object has moved -- by srt_scene_pose, by srt_scene_update -- renders the moved scene: the table
    in the graph's kernel nodes is the captured boxes', and the kernels stop culling once the records' box epoch is no longer the table's."""
    from oracle import pyoracle as oracle
    from simple_raytracer_amd import build, host
    import gpu_frames as gf
    import pose_ref
    oracle.oracle_lib(); build.build_host()
    T = host.Transformation
    p = abi.make_params(W, H, abi.light_staircase(g.light, 2), focal=40.0, flags=abi.SRT_FLAG_NO_TIMING)
    r = int(g.flat.obj_root[0])
    z = 0.5 * float(g.flat.node_min.reshape(-1, 3)[r][2] + g.flat.node_max.reshape(-1, 3)[r][2])
    mats = np.eye(4, dtype=np.float32).reshape(1, 16).copy(); mats[0] = T.changeObjPosition(30.0 * z / 40.0, 0.0, 0.0)
    moved = pose_ref.pose_flat(g.flat, mats)
    ds = lib.DeviceScene(g.flat); ds.set_pose_source()
    hit = torch.full((H, W), -5, dtype=torch.int32, device=dev); t = torch.full((H, W), 7.0, dtype=torch.float32, device=dev)
    lin = torch.full((H, W, 3), 9.0, dtype=torch.float32, device=dev); rgb8 = torch.full((H, W, 3), 77, dtype=torch.uint8, device=dev)
    def frame():
        ds.render_device(p, stream=torch.cuda.current_stream().cuda_stream, hit_id=hit.data_ptr(), t=t.data_ptr(), rgb_linear=lin.data_ptr(), rgb8=rgb8.data_ptr())
    def check(flat, what):
        torch.cuda.synchronize()
        o = {"hit_id": hit.cpu().numpy(), "t": t.cpu().numpy(), "rgb_linear": lin.cpu().numpy(), "rgb8": rgb8.cpu().numpy()}
        c = oracle.render(flat, p, pow="device")
        o["stats"] = c["stats"]
        gf.compare_exact(lib, o, c, gf.owned(p), flat, p, what)
        hit.fill_(-5); t.fill_(7.0); lin.fill_(9.0); rgb8.fill_(77)
        return o
    frame(); frame()
    first = check(g.flat, "eager")
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        frame(); frame()                                        # (an even number of renders per graph: the two counter sets stay in step)
    gph.replay(); check(g.flat, "replay, nothing moved")
    cur = torch.cuda.current_stream().cuda_stream
    ds.pose(mats, stream=cur); gph.replay()
    after = check(moved, "replay after srt_scene_pose")
    cols0 = np.nonzero((first["hit_id"] >= 0).any(axis=0))[0]; cols1 = np.nonzero((after["hit_id"] >= 0).any(axis=0))[0]
    assert cols1.max() > cols0.max() + 16, "the object did not leave the captured spans"
    ds.update(g.flat, stream=cur); gph.replay(); check(g.flat, "replay after srt_scene_update back to the created scene")
    ds.update(moved, stream=cur); gph.replay(); check(moved, "replay after srt_scene_update to the moved scene")
    ds.close()


if __name__ == "__main__":
    main()
