"""Run by tests/test_gpu_refit.py in its own process (torch initialises HIP first): a deforming frame captured into a hipGraph.  One
stream, a linear chain: a torch op writes the vertex tensor from a phase held in a device tensor, srt_scene_refit_device refits the
scene from it, two srt_render_device calls (SRT_FLAG_NO_TIMING; an even number keeps the alternating counter sets in step) draw it.
Captured once, replayed with two phases: every replay leaves the eager run's records and frames, bit for bit."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402
import refit_ref                               # noqa: E402

W, H = 128, 96


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene("ground_bunny")
    verts, tv = refit_ref.weld(g.flat)
    nV = verts.shape[0]
    ds = lib.DeviceScene(g.flat)
    ds.refit_prepare(tv, nV)
    v0 = torch.from_numpy(verts).to(dev)
    vbuf = v0.clone()
    phase = torch.zeros(1, dtype=torch.float32, device=dev)
    # the whole frame, then the odd 8-row blocks of it: ONE light table (a handle that is given another one waits for its earlier
    # renders before it overwrites the pinned copy, which a capturing stream cannot do)
    lights = abi.light_staircase(g.light, 2)
    params = [abi.make_params(W, H, lights, flags=abi.SRT_FLAG_NO_TIMING),
              abi.make_params(W, H, lights, block_rows=8, block_first=1, block_stride=2, flags=abi.SRT_FLAG_NO_TIMING)]
    rows = [ds.rows(p) for p in params]
    assert rows == [H, H // 2]
    hit = [torch.full((r, W), -5, dtype=torch.int32, device=dev) for r in rows]
    lin = [torch.zeros((r, W, 3), dtype=torch.float32, device=dev) for r in rows]
    rgb8 = [torch.zeros((r, W, 3), dtype=torch.uint8, device=dev) for r in rows]

    def chain():
        cur = torch.cuda.current_stream().cuda_stream
        vbuf[:, 1] = v0[:, 1] + 6.0 * torch.sin(0.05 * v0[:, 0] + phase)
        ds.refit_device(vbuf.data_ptr(), stride=4, n_verts=nV, stream=cur)
        for k, p in enumerate(params):
            ds.render_device(p, cur, hit_id=hit[k].data_ptr(), rgb_linear=lin[k].data_ptr(), rgb8=rgb8[k].data_ptr())

    def result():
        torch.cuda.synchronize()
        out = (ds.records(), vbuf.cpu().numpy().copy(), [x.cpu().numpy().copy() for x in hit], [x.cpu().numpy().copy() for x in lin],
               [x.cpu().numpy().copy() for x in rgb8])
        for k in range(len(params)):
            hit[k].fill_(-5); lin[k].zero_(); rgb8[k].zero_()
        vbuf.copy_(v0)
        ds.update(g.flat); ds.sync()                             # back to the created scene, so that a replay that did nothing would show ...
        ds.refit_prepare(tv, nV)                                 # ... (the update has discarded the preparation)
        torch.cuda.synchronize()
        return out

    phases = (0.6, 3.3)
    side = torch.cuda.Stream(device=dev)
    eager = []
    for ph in phases:
        phase.fill_(ph)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            chain()
        side.synchronize()
        eager.append(result())
    assert not np.array_equal(eager[0][1], eager[1][1]) and not np.array_equal(eager[0][2][0], eager[1][2][0]), "the phases differ"
    assert (eager[0][2][0] >= 0).any() and not np.array_equal(eager[0][1], verts)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        chain()
    torch.cuda.synchronize()
    assert (hit[0].cpu().numpy() == -5).all(), "a captured launch does not run"
    for rep, k in enumerate((0, 1, 0)):
        phase.fill_(phases[k])
        gph.replay()
        got = result()
        what = f"replay {rep}, phase {phases[k]}"
        refit_ref.same_bytes(got[0], eager[k][0], what)
        assert np.array_equal(got[1].view(np.uint32), eager[k][1].view(np.uint32)), (what, "vertices")
        for f in range(len(params)):
            assert np.array_equal(got[2][f], eager[k][2][f]), (what, f, "hit ids")
            assert np.array_equal(got[3][f].view(np.uint32), eager[k][3][f].view(np.uint32)), (what, f, "linear")
            assert np.array_equal(got[4][f], eager[k][4][f]), (what, f, "rgb8")
    print("refit graph case: ok")


if __name__ == "__main__":
    main()
