"""CPU: the yardstick of srt_trace_rays_multi (tests/ray_multi_ref.py) pinned against ray_range_ref.closest -- its column 0 is the
closest hit, with and without intervals -- and the input conditions that make the GPU cases of tests/test_gpu_ray_multi.py say
something: ties several deep, rays whose hits are one +0 and one -0, a tie-free family with deep rows, a scene that overflows k = 16."""
import inspect

import numpy as np
import pytest

import golden_util as gu
import ray_multi_ref as rm
import ray_query_ref as rq
import ray_range_ref as rr
import tree_shapes as ts
from simple_raytracer_amd import lib


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene_and_rays(name):
    if name in ts.FAMILIES:
        return ts.family(name), ts.ray_batch(name)
    flat = gu.GoldenScene(name).flat
    return flat, rq.unrelated_rays(flat, 130 if name == "cube" else 257, seed=5)


@pytest.mark.parametrize("name", ["cube", "cubes4_a40", "ties", "sliced"])
def test_column_0_is_the_closest_hit(oracle, name):
    """Unbounded and on a mixed interval batch, for k = 1, 4 and 16: column 0 is ray_range_ref.closest, n_hits > 0 iff it hits, a row at
    a smaller k is a prefix of the row at a larger k, rows ascend in (t, id), and the padding follows the hits."""
    flat, rays = scene_and_rays(name)
    c = rr.candidates(oracle, flat, rays)
    for tr in (None, rr.mixed_intervals(c, 17)[0]):
        want_hit, want_t = rr.closest(c, tr)
        n16, hit16, t16 = rm.multi(c, 16, tr)
        assert (want_hit >= 0).sum() >= 20
        for k in (1, 4, 16):
            n_hits, hit, t = rm.multi(c, k, tr)
            assert np.array_equal(hit[:, 0], want_hit) and np.array_equal(bits(t[:, 0]), bits(want_t)), (name, k)
            assert np.array_equal(n_hits > 0, want_hit >= 0) and np.array_equal(n_hits, n16)
            assert np.array_equal(hit, hit16[:, :k]) and np.array_equal(bits(t), bits(t16[:, :k]))
            filled = np.arange(k)[None, :] < np.minimum(n_hits, k)[:, None]
            assert np.array_equal(hit >= 0, filled) and (t[~filled] == np.inf).all() and np.isfinite(t[filled]).all()
        key = (t16 + np.float32(0.0)).astype(np.float64)
        both = (hit16[:, 1:] >= 0)
        assert ((key[:, 1:] > key[:, :-1]) | ((key[:, 1:] == key[:, :-1]) & (hit16[:, 1:] > hit16[:, :-1])))[both].all()


def test_ties_batch_has_deep_ties(oracle):
    c = rr.candidates(oracle, ts.family("ties"), ts.ray_batch("ties"))
    groups, deepest = rm.equal_t_groups(c)
    n_hits = rm.multi(c, 1)[0]
    print("ties batch: equal-t groups", groups, "deepest", deepest, "most hits on a ray", int(n_hits.max()))
    assert ts.ray_batch("ties").shape[0] == 364 and groups >= 300 and deepest >= 2 and n_hits.max() >= 10


def test_ties_frame_has_signed_zero_pairs(oracle):
    rays = ts.frame_rays()
    c = rr.candidates(oracle, ts.family("ties"), rays)
    pairs = rm.zero_pairs(c)
    print("ties frame: rays", rays.shape[0], "whose hits are one +0 and one -0:", int(pairs.sum()))
    assert rays.shape[0] == 4032 and pairs.sum() >= 2000


def test_sliced_batch_is_tie_free_and_deep(oracle):
    c = rr.candidates(oracle, ts.family("sliced"), ts.ray_batch("sliced"))
    groups, _ = rm.equal_t_groups(c)
    n_hits = rm.multi(c, 1)[0]
    print("sliced batch: equal-t groups", groups, "most hits on a ray", int(n_hits.max()))
    assert groups == 0 and n_hits.max() >= 7


def test_stack_batch_overflows_every_row(oracle):
    flat, rays = rm.stack_scene(), rm.stack_rays()
    assert flat.n_tris == 40 and sorted(flat.node_count[flat.node_left < 0].tolist()) == [9, 31] and rays.shape[0] == 65
    c = rr.candidates(oracle, flat, rays)
    n_hits, hit, t = rm.multi(c, 16)
    assert (n_hits == 40).all() and (hit >= 0).all() and (np.diff(t, axis=1) > 0).all()
    assert rm.equal_t_groups(c)[0] == 0
    for layers in (16, 17, 15):
        assert (rm.multi(c, 16, rm.stack_segment(layers))[0] == layers).all(), layers


def test_the_definition_on_a_hand_made_set():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    t = np.array([2.0, 1.0, 1.0, -inf, inf, nan, 0.0, -0.0, 3.0], np.float32)
    c = rr.Candidates(2, np.zeros(t.size, np.int64), np.arange(t.size, dtype=np.int64) + 10, t)      # ray 1 has no candidate
    n_hits, hit, tt = rm.multi(c, 4)
    assert n_hits.tolist() == [6, 0] and hit.tolist() == [[16, 17, 11, 12], [-1] * 4]
    assert bits(tt[0]).tolist() == bits(np.float32([0.0, -0.0, 1.0, 1.0])).tolist() and (tt[1] == inf).all()
    n_hits, hit, tt = rm.multi(c, 8, np.float32([[1.0, 2.0], [0.0, inf]]))
    assert n_hits.tolist() == [3, 0] and hit[0].tolist() == [11, 12, 10] + [-1] * 5 and (tt[0, 3:] == inf).all()
    assert rm.multi(c, 2, np.float32([[nan, nan], [nan, nan]]))[0].tolist() == [6, 0]


def test_python_interface():
    assert {"srt_trace_rays_multi_device", "srt_trace_rays_multi"} <= set(lib.ABI_SYMBOLS) and lib.MULTI_HIT_MAX == 16
    p = inspect.signature(lib.DeviceScene.trace_rays_multi).parameters
    assert list(p)[1:3] == ["rays", "k"] and p["want"].default == ("n_hits", "hit_id", "t", "bary") and p["count"].default is False and p["t_range"].default is None
    assert "t_range" in inspect.signature(lib.DeviceScene.trace_rays_multi_device).parameters


def test_argument_errors_without_device_work():
    """A NULL handle, k = 0 and k = 17 are refused before anything is touched, on a machine without a device too."""
    import ctypes as C
    from simple_raytracer_amd import abi, build
    build.build_all()
    L = lib.load()
    assert L.srt_trace_rays_multi(None, 0, None, None, 1, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi_device(None, 4, None, None, 1, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    fake = C.c_void_p(8)                       # (never dereferenced: the refusals below come first)
    rays = np.zeros((4, 6), np.float32)
    r = rays.ctypes.data_as(C.POINTER(C.c_float))
    assert L.srt_trace_rays_multi(fake, 4, r, None, 0, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi(fake, 4, r, None, 17, 0, None, None, None, None, None) == abi.SRT_ERR_LIMIT
    assert L.srt_trace_rays_multi_device(fake, 4, C.c_void_p(8), None, 0, 0, None, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_trace_rays_multi_device(fake, 4, C.c_void_p(8), None, 17, 0, None, None, None, None, None) == abi.SRT_ERR_LIMIT
