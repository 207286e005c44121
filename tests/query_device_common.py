"""What the tests/*_device_case.py children share: the way in (the repository on sys.path, torch's device initialised before the library's,
a side stream), the tensors a _device call writes and their comparison with the host form's result, the capture of a call into a
hipGraph, the render that must stay untouched around a query, rays at a float-aligned address, a shared handle.  A case imports this
module before simple_raytracer_amd: run as a script it has tests/ on sys.path, and the repository's root comes from here."""
import os, sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simple_raytracer_amd import abi           # noqa: E402

W, H, FOCAL = 192, 108, 40.0
STAT_KEYS = ("primary_rays", "hit_rays", "shadow_rays", "node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow", "rows")
TORCH = {np.int32: torch.int32, np.uint32: torch.int32, np.float32: torch.float32, np.uint8: torch.uint8}      # (a uint32 result lives in an int32 tensor)
QUERY_FILL = {np.int32: -5, np.uint32: -5, np.float32: -1.0, np.uint8: 7}      # the sentinels of the query cases, by type
INF, NAN = np.float32(np.inf), np.float32(np.nan)
UNBOUNDED = (None, (0.0, INF), (-INF, INF), (NAN, NAN))      # a NULL t_range and the three intervals that bound nothing
SHARE = dict(block_rows=8, block_cols=8, block_first=1, block_stride=2)      # the tile share of the frame cases


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def open_case(scene):
    """The way into a case: torch's device first, the golden scene, a second stream.  c.render(ds): the UntouchedRender of the scene;
    c.put(arrays...): the arrays as device tensors, arrived."""
    import golden_util as gu
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    g = gu.GoldenScene(scene)

    def put(*arrays):
        tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]
        torch.cuda.synchronize()
        return tensors
    return SimpleNamespace(dev=dev, g=g, side=torch.cuda.Stream(device=dev), render=lambda ds: UntouchedRender(dev, g, ds), put=put)


def shade_spec(n):
    """The Outputs spec of srt_shade_rays on n rays."""
    return {"hit_id": ((n,), np.int32), "t": ((n,), np.float32), "rgb_linear": ((n, 3), np.float32), "rgb8": ((n, 3), np.uint8)}


def path_spec(shape, depth, side_rows=False):
    """The Outputs spec of a path call on `shape` rays or pixels: rgb_linear, rgb8, the seg_* rows and, with side_rows, the side rays'."""
    spec = {"rgb_linear": (shape + (3,), np.float32), "rgb8": (shape + (3,), np.uint8)}
    rows = [("seg_" + k, f) for k, f in abi.PATH_FIELDS.items()]
    rows += [("fresnel" if k == "fresnel" else "side_" + k, f) for k, f in abi.FRESNEL_FIELDS.items()] if side_rows else []
    for k, (ty, c) in rows:
        spec[k] = ((depth,) + shape + (() if c == 1 else (c,)), ty)
    return spec


class Outputs:
    """The tensors a _device call writes, under the keys of the host form's result.  spec: key -> (shape, numpy type[, sentinel]); `fill` is
    the sentinel of every other key, one value or one per numpy type.  Every tensor holds its sentinel between two calls."""

    def __init__(self, dev, spec, fill):
        self.ty = {k: s[1] for k, s in spec.items()}
        self.fill = {k: s[2] if len(s) > 2 else fill[s[1]] if isinstance(fill, dict) else fill for k, s in spec.items()}
        self.t = {k: torch.empty(tuple(s[0]), dtype=TORCH[s[1]], device=dev) for k, s in spec.items()}
        self.reset()

    def reset(self):
        for k, v in self.t.items():
            v.fill_(self.fill[k])
        torch.cuda.synchronize()

    def ptrs(self, rename={}, keys=None):
        """The pointers as keyword arguments: argument rename.get(key, key) for every key (of `keys`)."""
        return {rename.get(k, k): v.data_ptr() for k, v in self.t.items() if keys is None or k in keys}

    def untouched(self, keys=None):
        return all((v.cpu().numpy() == self.fill[k]).all() for k, v in self.t.items() if keys is None or k in keys)

    def same(self, host, what, untouched=(), keys=None):
        """Every tensor (of `keys`) against host[key] -- floats by their bits, integers by value -- except those of `untouched`, which
        must still hold their sentinel.  Then the sentinels again."""
        for k, v in self.t.items():
            if keys is not None and k not in keys:
                continue
            if k in untouched:
                assert self.untouched((k,)), (what, k, "an output that was not asked for was written")
                continue
            got, want = v.cpu().numpy().view(self.ty[k]), host[k]
            assert np.array_equal(bits(got), bits(want)) if self.ty[k] is np.float32 else np.array_equal(got, want), (what, k)
        self.reset()


def captured(call, outs, hosts, what, probe, replays=2):
    """call(stream) captured into a hipGraph on torch's current stream: it does not run (every (Outputs, keys) of `probe` still holds its
    sentinels); then replayed, and after each replay outs[i] is hosts[i] under the label what[i].format(rep=...).  One Outputs, result
    and label may stand without their tuple.  Returns the graph."""
    if isinstance(outs, Outputs):
        outs, hosts, what = (outs,), (hosts,), (what,)
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph, capture_error_mode="thread_local"):
        call(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert all(o.untouched(keys) for o, keys in probe), "a captured launch does not run"
    for rep in range(replays):
        gph.replay(); torch.cuda.synchronize()
        for o, host, label in zip(outs, hosts, what):
            o.same(host, label.format(rep=rep))
    return gph


class UntouchedRender:
    """A counting render of the scene on torch's current stream: its pixels, statistics and pipeline string are the same before a query,
    with a query pending beside it on another stream, and after."""

    def __init__(self, dev, g, ds):
        self.ds = ds
        self.p = g.params(W, H, 2, flags=abi.SRT_FLAG_COUNT_WORK)
        self.fhit = torch.zeros((H, W), dtype=torch.int32, device=dev); self.flin = torch.zeros((H, W, 3), dtype=torch.float32, device=dev)
        self.cur = torch.cuda.current_stream().cuda_stream
        self.base = [self.render(), self.render()]                 # both alternating counter sets
        assert self.base[0][2] == self.base[1][2] and self.base[0][2]["node_tests_primary"] > 0

    def enqueue(self):
        self.fhit.fill_(-5); self.flin.zero_(); torch.cuda.synchronize()
        self.ds.render_device(self.p, stream=self.cur, hit_id=self.fhit.data_ptr(), rgb_linear=self.flin.data_ptr())

    def render(self):
        self.enqueue()
        st = self.ds.sync()
        torch.cuda.synchronize()
        return self.fhit.cpu().numpy().copy(), self.flin.cpu().numpy().copy(), {k: st[k] for k in STAT_KEYS}, self.ds.pipeline

    def pending_beside(self, rep, side, queries):
        """The render is enqueued, queries() runs on the second stream while it is pending, then srt_sync: the render's statistics."""
        base, ds = self.base, self.ds
        self.enqueue()
        queries()
        pipe = ds.pipeline
        st = ds.sync()
        side.synchronize(); torch.cuda.synchronize()
        assert {k: st[k] for k in STAT_KEYS} == base[0][2], (rep, st, base[0][2])
        assert pipe == base[0][3] == ds.pipeline
        assert np.array_equal(self.fhit.cpu().numpy(), base[0][0]) and np.array_equal(bits(self.flin.cpu().numpy()), bits(base[0][1])), rep

    def after(self):
        after, base = self.render(), self.base
        assert after[2] == base[0][2] and np.array_equal(after[0], base[0][0]) and np.array_equal(bits(after[1]), bits(base[0][1]))


def float_aligned(dev, d):
    """The same 4-byte words at an address that is only 4-byte aligned (rays and intervals there take the narrow loads)."""
    odd = torch.empty(d.numel() + 1, dtype=d.dtype, device=dev)
    odd[1:].copy_(d.reshape(-1))
    assert odd[1:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    return odd[1:]


def through_shared_handle(ds, query):
    """query(handle) on a handle made with srt_scene_share: the one copy of the records."""
    sh = ds.share()
    query(sh)
    assert sh.device_bytes == ds.device_bytes
    sh.close()
