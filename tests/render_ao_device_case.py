"""Run by tests/test_gpu_render_ao.py in its own process (torch initialises HIP first): the _device forms of the ambient-occlusion frame
calls on torch tensors -- a second stream; a device rotation table; results equal to the host forms' (which tests/test_gpu_render_ao.py pins
against tests/render_ao_ref.py and the shipped srt_ao_rays); a shared handle; a render pending on another stream stays untouched; both
calls captured into one hipGraph and replayed twice to the eager bits."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import ao_ref as ar                            # noqa: E402
import golden_util as gu                       # noqa: E402
import render_ao_ref as ra                     # noqa: E402
from query_device_common import UntouchedRender, bits, through_shared_handle      # noqa: E402

SCENE, T_MAX = "cubes4_a40", 60.0
DIRS = ar.directions(40)                       # two words a row, a partial chunk
ROT = ra.rotations(3, 5)


class Outputs:
    def __init__(self, dev, shape, words):
        self.hit = torch.empty(shape, dtype=torch.int32, device=dev); self.t = torch.empty(shape, dtype=torch.float32, device=dev)
        self.cnt = torch.empty(shape, dtype=torch.int32, device=dev); self.ao = torch.empty(shape, dtype=torch.float32, device=dev)
        self.words = torch.empty(shape + (words,), dtype=torch.int32, device=dev); self.bent = torch.empty(shape + (3,), dtype=torch.float32, device=dev)
        self.ao8 = torch.empty(shape, dtype=torch.uint8, device=dev)
        self.fill()

    def fill(self):
        self.hit.fill_(-5); self.t.fill_(-1.0); self.cnt.fill_(-5); self.ao.fill_(-1.0); self.words.fill_(-5); self.bent.fill_(-1.0); self.ao8.fill_(7)
        torch.cuda.synchronize()

    def ptrs(self):
        return dict(n_occluded=self.cnt.data_ptr(), ao=self.ao.data_ptr(), occ_bits=self.words.data_ptr(), bent=self.bent.data_ptr(), ao8=self.ao8.data_ptr())

    def untouched(self):
        return (self.cnt.cpu().numpy() == -5).all() and (self.words.cpu().numpy() == -5).all() and (self.hit.cpu().numpy() == -5).all() and \
            (self.bent.cpu().numpy() == -1.0).all() and (self.ao8.cpu().numpy() == 7).all()

    def same(self, want, what, hits=True):
        if hits:
            assert np.array_equal(self.hit.cpu().numpy(), want["hit_id"]), (what, "hit ids")
            assert np.array_equal(bits(self.t.cpu().numpy()), bits(want["t"])), (what, "t")
        assert np.array_equal(self.cnt.cpu().numpy().view(np.uint32), want["n_occluded"]), (what, "n_occluded")
        assert np.array_equal(bits(self.ao.cpu().numpy()), bits(want["ao"])), (what, "ao")
        assert np.array_equal(self.words.cpu().numpy().view(np.uint32), want["occ_bits"]), (what, "occ_bits")
        assert np.array_equal(bits(self.bent.cpu().numpy()), bits(want["bent"])), (what, "bent")
        assert np.array_equal(self.ao8.cpu().numpy(), want["ao8"]), (what, "ao8")
        self.fill()


def main():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(SCENE)
    flat, p = ra.case(SCENE)
    k = DIRS.shape[0]
    ds = lib.DeviceScene(flat)
    host = ds.render_ao(p, DIRS, ROT, t_max=T_MAX, skip_self=True)
    plain = ds.render_ao(p, DIRS, None, t_max=T_MAX, skip_self=True)
    assert 0 < (host["n_occluded"] > 0).sum() < (host["hit_id"] >= 0).sum() < host["hit_id"].size and (host["occ_bits"] != plain["occ_bits"]).any()
    d_dirs, d_rot = torch.from_numpy(DIRS).to(dev), torch.from_numpy(ROT).to(dev)
    d_hit, d_t = torch.from_numpy(host["hit_id"]).to(dev), torch.from_numpy(host["t"]).to(dev)
    shape = host["hit_id"].shape
    out, out_h = Outputs(dev, shape, (k + 31) // 32), Outputs(dev, shape, (k + 31) // 32)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def both(handle, stream, count=False, rot=True):
        table = dict(rot=d_rot.data_ptr(), rot_w=ROT.shape[1], rot_h=ROT.shape[0]) if rot else {}
        handle.render_ao_device(p, d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, hit_id=out.hit.data_ptr(), t=out.t.data_ptr(),
                                **table, **out.ptrs())
        handle.render_ao_hits_device(p, d_hit.data_ptr(), d_t.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **table,
                                     **out_h.ptrs())

    def same(what, want=host):
        out.same(want, what); out_h.same(want, what + ", the hits form", hits=False)

    render = UntouchedRender(dev, g, ds)
    for count in (False, True):
        render.pending_beside(count, side, lambda: both(ds, side.cuda_stream, count))
        same(f"second stream beside a pending render, counting {count}")
    render.after()
    both(ds, side.cuda_stream, rot=False); side.synchronize()
    same("no rotation table", plain)
    through_shared_handle(ds, lambda sh: (both(sh, side.cuda_stream), side.synchronize()))
    same("a shared handle")
    # both calls in one captured graph, replayed twice
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        both(ds, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert out.untouched() and out_h.cnt.cpu().numpy().min() == -5, "a captured launch does not run"
    for rep in range(2):
        gph.replay(); torch.cuda.synchronize()
        same(f"replay {rep}")
    render.after()
    ds.close()
    print("render ao device case: ok")


if __name__ == "__main__":
    main()
