"""Run by tests/test_gpu_render_ao.py in its own process (torch initialises HIP first): the _device forms of the ambient-occlusion frame
calls on torch tensors -- a second stream; a device rotation table; results equal to the host forms' (which tests/test_gpu_render_ao.py pins
against tests/render_ao_ref.py and the shipped srt_ao_rays); a shared handle; a render pending on another stream stays untouched; both
calls captured into one hipGraph and replayed twice to the eager bits."""
import numpy as np

from query_device_common import QUERY_FILL, Outputs, captured, open_case, through_shared_handle
from simple_raytracer_amd import lib
import ao_ref as ar
import render_ao_ref as ra

SCENE, T_MAX = "cubes4_a40", 60.0
DIRS = ar.directions(40)                       # two words a row, a partial chunk
ROT = ra.rotations(3, 5)


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, p = ra.case(SCENE)
    k = DIRS.shape[0]
    ds = lib.DeviceScene(flat)
    host = ds.render_ao(p, DIRS, ROT, t_max=T_MAX, skip_self=True)
    plain = ds.render_ao(p, DIRS, None, t_max=T_MAX, skip_self=True)
    assert 0 < (host["n_occluded"] > 0).sum() < (host["hit_id"] >= 0).sum() < host["hit_id"].size and (host["occ_bits"] != plain["occ_bits"]).any()
    d_dirs, d_rot, d_hit, d_t = c.put(DIRS, ROT, host["hit_id"], host["t"])
    shape = host["hit_id"].shape
    ao = {"n_occluded": (shape, np.uint32), "ao": (shape, np.float32), "occ_bits": (shape + ((k + 31) // 32,), np.uint32), "bent": (shape + (3,), np.float32),
          "ao8": (shape, np.uint8)}
    out, out_h = Outputs(dev, {"hit_id": (shape, np.int32), "t": (shape, np.float32), **ao}, QUERY_FILL), Outputs(dev, ao, QUERY_FILL)

    def both(handle, stream, count=False, rot=True):
        table = dict(rot=d_rot.data_ptr(), rot_w=ROT.shape[1], rot_h=ROT.shape[0]) if rot else {}
        handle.render_ao_device(p, d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **table, **out.ptrs())
        handle.render_ao_hits_device(p, d_hit.data_ptr(), d_t.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **table,
                                     **out_h.ptrs())

    def same(what, want=host):
        out.same(want, what); out_h.same(want, what + ", the hits form")

    render = c.render(ds)
    for count in (False, True):
        render.pending_beside(count, side, lambda: both(ds, side.cuda_stream, count))
        same(f"second stream beside a pending render, counting {count}")
    render.after()
    both(ds, side.cuda_stream, rot=False); side.synchronize()
    same("no rotation table", plain)
    through_shared_handle(ds, lambda sh: (both(sh, side.cuda_stream), side.synchronize()))
    same("a shared handle")
    # both calls in one captured graph, replayed twice
    captured(lambda stream: both(ds, stream), (out, out_h), (host, host), ("replay {rep}", "replay {rep}, the hits form"),
             [(out, ("n_occluded", "occ_bits", "hit_id", "bent", "ao8")), (out_h, ("n_occluded",))])
    render.after()
    ds.close()
    print("render ao device case: ok")


if __name__ == "__main__":
    main()
