"""What tests/ray_query_device_case.py and tests/shade_query_device_case.py share: the frame of rays, the render that must stay untouched
around a query, rays at a float-aligned address, a shared handle."""
import numpy as np
import torch

from simple_raytracer_amd import abi

W, H, FOCAL = 192, 108, 40.0
STAT_KEYS = ("primary_rays", "hit_rays", "shadow_rays", "node_tests_primary", "tri_tests_primary", "node_tests_shadow", "tri_tests_shadow", "rows")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


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


def float_aligned(dev, d_rays):
    """The same rays at an address that is only float-aligned (they take the narrow loads)."""
    odd = torch.empty(d_rays.numel() + 1, dtype=torch.float32, device=dev)
    odd[1:].copy_(d_rays.reshape(-1))
    assert odd[1:].data_ptr() % 8 == 4
    torch.cuda.synchronize()
    return odd[1:]


def through_shared_handle(ds, query):
    """query(handle) on a handle made with srt_scene_share: the one copy of the records."""
    sh = ds.share()
    query(sh)
    assert sh.device_bytes == ds.device_bytes
    sh.close()
