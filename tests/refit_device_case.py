"""Run by tests/test_gpu_refit.py in its own process (torch initialises HIP first): srt_scene_refit_device on torch tensors.
`torch`: the welded bunny displaced by a non-affine torch expression on the device, every load shape, twice the same bits.
`stream`: write vertices -> refit -> render -> write other vertices -> refit -> render on ONE torch stream, one wait at the end."""
import os, sys
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
from oracle import pyoracle as oracle          # noqa: E402
import golden_util as gu                       # noqa: E402
import gpu_frames as gf                        # noqa: E402
import refit_ref                               # noqa: E402

W, H = 128, 96


def setup():
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    oracle.oracle_lib()
    g = gu.GoldenScene("ground_bunny")
    verts, tv = refit_ref.weld(g.flat)
    ds = lib.DeviceScene(g.flat)
    ds.refit_prepare(tv, verts.shape[0])
    return dev, g, ds, verts, tv, torch.from_numpy(verts).to(dev)


def wave(v, phase):
    """A travelling sine along x lifts y, and z swings with the product of the two other coordinates: no matrix does this.  v: n x 4
    on the device; w stays."""
    out = v.clone()
    out[:, 1] = v[:, 1] + 6.0 * torch.sin(0.05 * v[:, 0] + phase)
    out[:, 2] = v[:, 2] + 4.0 * torch.cos(1.0e-4 * v[:, 0] * v[:, 1] + 0.5 * phase)
    return out


def check(ds, g, pts, p, what, o=None):
    """The scene's records and a frame against refit_ref's flat scene of `pts` (n_tris x 3 x 4, from the tensor copied back)."""
    want = refit_ref.refit_flat(g.flat, pts)
    if o is None:
        fresh = lib.DeviceScene(want)
        refit_ref.same_records(ds.records(), fresh.records(), what)
        fresh.close()
        o = ds.render(p)
    c = oracle.render(want, p, pow="device")
    if "stats" not in o:
        o["stats"] = c["stats"]                                  # (a frame rendered into tensors: the pixels are what is checked)
    gf.compare_exact(lib, o, c, gf.owned(p), want, p, what)
    return o


def torch_case():
    dev, g, ds, verts, tv, v0 = setup()
    nV = verts.shape[0]
    p = g.params(W, H, 2)
    st = torch.cuda.Stream(device=dev)
    idx = torch.from_numpy(tv.astype(np.int64)).to(dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        v4 = wave(v0, 0.7)
        v3 = v4[:, :3].contiguous()
        d3 = v3[idx].reshape(-1).contiguous()                    # n_tris x 3 x 3: the direct form's buffer
        odd = torch.empty(d3.numel() + 1, dtype=torch.float32, device=dev)
        odd[1:].copy_(d3)
    st.synchronize()
    assert v3.data_ptr() % 16 == 0 and v4.data_ptr() % 16 == 0 and d3.data_ptr() % 16 == 0 and odd[1:].data_ptr() % 16 == 4
    h4, h3 = v4.cpu().numpy(), v3.cpu().numpy()
    assert not np.array_equal(h4, verts) and np.array_equal(h4[:, 3], verts[:, 3])
    pts = refit_ref.expand(h3, tv, 3)
    assert np.array_equal(refit_ref.bits(pts), refit_ref.bits(refit_ref.expand(h4, tv, 4))), "w = 1 on both routes"
    assert np.array_equal(refit_ref.bits(pts), refit_ref.bits(refit_ref.direct(d3.cpu().numpy(), 3)))
    seen = []
    for what, kw in (("indexed xyz", dict(points=v3.data_ptr(), stride=3, n_verts=nV)),
                     ("indexed xyzw", dict(points=v4.data_ptr(), stride=4, n_verts=nV)),
                     ("direct xyz, float-aligned", dict(points=odd[1:].data_ptr(), stride=3)),
                     ("direct xyz, 16-byte aligned", dict(points=d3.data_ptr(), stride=3))):
        ds.update(g.flat); ds.sync()                             # back to the created scene: every form starts from other records ...
        ds.refit_prepare(tv, nV)                                 # ... and the update has discarded the preparation
        for rep in range(2):
            ds.refit_device(stream=st.cuda_stream, **kw)
            st.synchronize()
            seen.append(ds.records())
        refit_ref.same_bytes(seen[-1], seen[-2], what + ", twice")
        refit_ref.same_bytes(seen[-1], seen[0], what + " against the first form")
        check(ds, g, pts, p, what)
    print("refit torch case: ok")


def stream_case():
    dev, g, ds, verts, tv, v0 = setup()
    nV = verts.shape[0]
    p = g.params(W, H, 2)
    st = torch.cuda.Stream(device=dev)
    vbuf = torch.empty_like(v0)
    out = [(torch.full((H, W), -5, dtype=torch.int32, device=dev), torch.zeros((H, W), dtype=torch.float32, device=dev),
            torch.zeros((H, W, 3), dtype=torch.float32, device=dev), torch.zeros((H, W, 3), dtype=torch.uint8, device=dev)) for _ in range(2)]
    phases = (0.4, 2.9)
    kept = []
    with torch.cuda.stream(st):
        vbuf.copy_(wave(v0, 0.0))
        ds.refit_device(vbuf.data_ptr(), stride=4, n_verts=nV, stream=st.cuda_stream)
        ds.render_device(p, st.cuda_stream, *[x.data_ptr() for x in out[0]])          # warm: workspace and lights are allocated
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for k, ph in enumerate(phases):
            vbuf.copy_(wave(v0, ph))                             # ONE vertex buffer: the second write is ordered behind the first refit's reads
            kept.append(vbuf.clone())
            ds.refit_device(vbuf.data_ptr(), stride=4, n_verts=nV, stream=st.cuda_stream)
            ds.render_device(p, st.cuda_stream, *[x.data_ptr() for x in out[k]])
    st.synchronize()
    frames = [{"hit_id": h.cpu().numpy(), "t": t.cpu().numpy(), "rgb_linear": l.cpu().numpy(), "rgb8": r.cpu().numpy()} for h, t, l, r in out]
    assert not np.array_equal(frames[0]["hit_id"], frames[1]["hit_id"])
    want = [x.cpu().numpy() for x in kept]                       # the reference is built from the tensors copied back
    for k, name in enumerate(("first", "second")):
        check(ds, g, refit_ref.expand(want[k], tv, 4), p, f"{name} frame of the stream", frames[k])
    print("refit stream case: ok")


if __name__ == "__main__":
    {"torch": torch_case, "stream": stream_case}[sys.argv[1]]()
