"""Run by tests/test_gpu_ray_multi.py in its own process (torch initialises HIP first): srt_trace_rays_multi_device on torch tensors.
A second stream, results equal to the host form's (which the parent pins against the yardstick), rays and t_range at addresses that are
only float-aligned, the scene's own stream, a counting call, a shared handle, and one call captured into a hipGraph and replayed twice.
Exits non-zero on the first mismatch."""
import numpy as np

from query_device_common import INF, QUERY_FILL, Outputs, bits, captured, float_aligned, open_case, through_shared_handle
from simple_raytracer_amd import lib
import ray_query_ref as rq

N, K = 257, 4


def main():
    c = open_case("cubes4_a40")
    dev, g, side = c.dev, c.g, c.side
    ds = lib.DeviceScene(g.flat)
    rays = rq.unrelated_rays(g.flat, N, seed=5)
    plain = ds.trace_rays(rays)
    t1 = np.where(plain["hit_id"] >= 0, plain["t"], np.float32(50.0)).astype(np.float32)
    kind = np.arange(N) % 4                    # from the second hit on; nothing; the first hit alone; around the first hit
    tr = np.empty((N, 2), np.float32)
    tr[:, 0] = np.select([kind == 0, kind == 1, kind == 2], [np.nextafter(t1, INF), 0.0, t1], t1 * np.float32(0.5))
    tr[:, 1] = np.select([kind == 0, kind == 1, kind == 2], [INF, np.nextafter(t1, -INF), t1], t1 * np.float32(1.5))
    host, open_ = ds.trace_rays_multi(rays, K, t_range=tr), ds.trace_rays_multi(rays, K)
    assert (host["n_hits"] > 0).sum() > N // 4 and not np.array_equal(host["hit_id"], open_["hit_id"]) and (open_["n_hits"] >= K).any() and (open_["n_hits"] == 0).any()

    d_rays, d_tr = c.put(rays, tr)
    assert d_rays.data_ptr() % 8 == 0 and d_tr.data_ptr() % 8 == 0
    out = Outputs(dev, {"n_hits": ((N,), np.uint32, 99), "hit_id": ((N, K), np.int32), "t": ((N, K), np.float32), "bary": ((N, K, 3), np.float32)}, QUERY_FILL)

    def call(h, r_ptr, tr_ptr, stream, count=False):
        h.trace_rays_multi_device(N, r_ptr, K, stream=stream, count=count, t_range=tr_ptr, **out.ptrs())

    for count in (False, True):
        call(ds, d_rays.data_ptr(), d_tr.data_ptr(), side.cuda_stream, count)
        side.synchronize()
        out.same(host, f"second stream, counting {count}")
    call(ds, d_rays.data_ptr(), None, side.cuda_stream)
    side.synchronize()
    out.same(open_, "NULL t_range")
    call(ds, d_rays.data_ptr(), d_tr.data_ptr(), 0)            # NULL stream = the scene's own stream
    ds.occluded(rays)                                          # (a host call on the same stream waits for it)
    out.same(host, "own stream")
    odd_rays, odd_tr = float_aligned(dev, d_rays), float_aligned(dev, d_tr)      # 4 bytes further: the narrow loads
    call(ds, odd_rays.data_ptr(), odd_tr.data_ptr(), side.cuda_stream)
    side.synchronize()
    out.same(host, "float-aligned rays and t_range")
    # only some outputs
    ds.trace_rays_multi_device(N, d_rays.data_ptr(), K, stream=side.cuda_stream, t_range=d_tr.data_ptr(), **out.ptrs(keys=("t",)))
    side.synchronize()
    assert np.array_equal(bits(out.t["t"].cpu().numpy()), bits(host["t"])) and out.untouched(("hit_id", "n_hits"))
    out.reset()

    def shared(sh):
        call(sh, d_rays.data_ptr(), d_tr.data_ptr(), side.cuda_stream)
        side.synchronize()
        out.same(host, "shared handle")
    through_shared_handle(ds, shared)

    # one call captured into a graph (one launch, nothing allocated or copied), replayed twice
    captured(lambda stream: call(ds, d_rays.data_ptr(), d_tr.data_ptr(), stream), out, host, "replay {rep}", [(out, ("hit_id", "n_hits"))])
    print("ray multi device case: ok")


if __name__ == "__main__":
    main()
