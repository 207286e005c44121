"""Run by tests/test_gpu_ao.py in its own process (torch initialises HIP first): the _device forms of the ambient-occlusion calls on torch
tensors -- a second stream; results equal to the host forms' (which tests/test_gpu_ao.py pins against tests/ao_ref.py on the same batch);
rays at an address that is only float-aligned; a shared handle; a render pending on another stream stays untouched; both calls captured
into one hipGraph and replayed twice to the eager bits."""
import numpy as np

from query_device_common import QUERY_FILL, Outputs, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import ao_ref as ar

SCENE, T_MAX = "cubes4_a40", 60.0
DIRS = ar.directions(40)                       # two words a row, a partial chunk


def batch():
    """(flat, rays): every other ray of the lamp case's frame."""
    flat, rays = ar.case_rays(SCENE)
    return flat, np.ascontiguousarray(rays[::2])


def main():
    c = open_case(SCENE)
    dev, side = c.dev, c.side
    flat, rays = batch()
    n, k = rays.shape[0], DIRS.shape[0]
    ds = lib.DeviceScene(flat)
    host = ds.ao_rays(rays, DIRS, t_max=T_MAX, skip_self=True)
    assert 0 < (host["n_occluded"] > 0).sum() < (host["hit_id"] >= 0).sum()
    d_rays, d_dirs, d_hit, d_t = c.put(rays, DIRS, host["hit_id"], host["t"])
    ao = {"n_occluded": ((n,), np.uint32), "ao": ((n,), np.float32), "occ_bits": ((n, (k + 31) // 32), np.uint32)}
    out, out_h = Outputs(dev, {"hit_id": ((n,), np.int32), "t": ((n,), np.float32), **ao}, QUERY_FILL), Outputs(dev, ao, QUERY_FILL)

    def both(handle, r, stream, count=False):
        handle.ao_rays_device(n, r.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **out.ptrs())
        handle.ao_hits_device(n, r.data_ptr(), d_hit.data_ptr(), d_t.data_ptr(), d_dirs.data_ptr(), k, t_max=T_MAX, skip_self=True, count=count, stream=stream, **out_h.ptrs())

    def same(what):
        out.same(host, what); out_h.same(host, what + ", ao_hits")

    render = c.render(ds)
    for count in (False, True):
        render.pending_beside(count, side, lambda: both(ds, d_rays, side.cuda_stream, count))
        same(f"second stream beside a pending render, counting {count}")
    render.after()
    both(ds, float_aligned(dev, d_rays), side.cuda_stream); side.synchronize()
    same("rays only float-aligned")
    through_shared_handle(ds, lambda sh: (both(sh, d_rays, side.cuda_stream), side.synchronize()))
    same("a shared handle")
    # both calls in one captured graph, replayed twice
    captured(lambda stream: both(ds, d_rays, stream), (out, out_h), (host, host), ("replay {rep}", "replay {rep}, ao_hits"),
             [(out, ("n_occluded", "occ_bits", "hit_id")), (out_h, ("n_occluded",))])
    render.after()
    ds.close()
    print("ao device case: ok")


if __name__ == "__main__":
    main()
