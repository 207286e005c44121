"""Helpers of the GPU mode tests (tests/test_gpu_modes.py): srt_render_device into pinned host buffers (srt_host_alloc) that carry
sentinels and one guard row, and the comparison with the oracle at the suite's bars."""
import ctypes as C

import numpy as np

from simple_raytracer_amd import abi

TOL_LINEAR = 1e-4          # as tests/test_gpu_parity.py: max per-pixel |dRGB| before tone mapping
SENTINEL_HIT = -7
SENTINEL_F32 = 0x7FC0DEAD  # a quiet NaN with a payload: no kernel computes these bits
SENTINEL_U8 = 0xA5


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_rgb8(got, want, max_frac=1e-3):
    """<= 1 LSB everywhere, and on at most max_frac of the pixels (at least one)."""
    got = np.asarray(got).reshape(-1, 3); want = np.asarray(want).reshape(-1, 3)
    if got.shape[0] == 0:
        return 0
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert diff.max() <= 1, f"rgb8 differs by {diff.max()} LSB"
    nbad = int((diff.max(-1) > 0).sum())
    assert nbad <= max(1, int(max_frac * got.shape[0])), f"{nbad} of {got.shape[0]} pixels differ by 1 LSB"
    return nbad


def owned(p):
    """Image pixel of every local output pixel of a call with these params (-1 = padding of a tile deal)."""
    return abi.owned_pixels(p.width, p.height, p.block_rows, p.block_first, p.block_stride, p.block_cols)


class PinnedFrame:
    """The four outputs of one frame in pinned host memory (the device writes them directly), rows + 1 rows each: the last row is
    a guard row no call may write.  Filled with sentinels at construction and by fill()."""

    def __init__(self, lib, rows, cols):
        self.L, self.rows, self.cols = lib, rows, cols
        self._ptrs = []
        self.hit = self._alloc((rows + 1, cols), np.int32)
        self.t = self._alloc((rows + 1, cols), np.uint32)
        self.lin = self._alloc((rows + 1, cols, 3), np.uint32)
        self.rgb8 = self._alloc((rows + 1, cols, 3), np.uint8)
        self.fill()

    def _alloc(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        ptr = self.L.srt_host_alloc(n)
        assert ptr, "srt_host_alloc failed"
        self._ptrs.append(ptr)
        return np.frombuffer((C.c_uint8 * n).from_address(ptr), dtype=dtype).reshape(shape)

    def fill(self):
        self.hit[...] = SENTINEL_HIT
        self.t[...] = SENTINEL_F32
        self.lin[...] = SENTINEL_F32
        self.rgb8[...] = SENTINEL_U8

    @property
    def ptrs(self):
        return [a.ctypes.data for a in (self.hit, self.t, self.lin, self.rgb8)]

    def out(self):
        """Copies of the frame's rows (guard row excluded), as DeviceScene.render returns them."""
        r = self.rows
        return {"hit_id": self.hit[:r].copy(), "t": self.t[:r].view(np.float32).copy(),
                "rgb_linear": self.lin[:r].view(np.float32).copy(), "rgb8": self.rgb8[:r].copy()}

    def check_untouched(self, own, what=""):
        """Every padding element (own == -1) and the whole guard row still hold the sentinels."""
        assert own.shape == (self.rows, self.cols), (own.shape, self.rows, self.cols)
        pad = np.concatenate([own == -1, np.ones((1, self.cols), bool)])
        for name, a, s in (("hit_id", self.hit, SENTINEL_HIT), ("t", self.t, SENTINEL_F32), ("rgb_linear", self.lin, SENTINEL_F32),
                           ("rgb8", self.rgb8, SENTINEL_U8)):
            bad = int((a[pad] != s).sum())
            assert bad == 0, f"{what}: {bad} {name} elements of the padding / guard row were written"

    def free(self):
        for ptr in self._ptrs:
            self.L.srt_host_free(ptr)
        self._ptrs = []


def render_pinned(lib, ds, p):
    """srt_render_device on the null stream into sentinel-filled pinned buffers, then srt_sync: (outputs, stats, pipeline).  The
    padding and the guard row are checked before the buffers are freed."""
    L = lib.load()
    f = PinnedFrame(L, ds.rows(p), ds.cols(p))
    try:
        ds.render_device(p, 0, *f.ptrs)
        st = ds.sync()
        f.check_untouched(owned(p), ds.pipeline)
        o = f.out()
    finally:
        f.free()
    o["stats"] = st
    return o, ds.pipeline


def compare(o, c, own, what=""):
    """A frame against the oracle on its live pixels: hit id and t bit for bit, pre-tone-map RGB within TOL_LINEAR relative to the
    frame's maximum, rgb8 <= 1 LSB on at most 1e-3 of the pixels, ray counts equal."""
    live = own >= 0
    assert np.array_equal(o["hit_id"][live], c["hit_id"][live]), f"{what}: {int((o['hit_id'][live] != c['hit_id'][live]).sum())} hit ids differ"
    assert np.array_equal(bits(o["t"][live]), bits(c["t"][live])), f"{what}: t differs"
    if live.any():
        cl = c["rgb_linear"][live]
        scale = max(1.0, float(np.abs(cl).max()))
        d = float(np.abs(o["rgb_linear"][live] - cl).max())
        assert d < TOL_LINEAR * scale, f"{what}: rgb_linear differs by {d}"
        check_rgb8(o["rgb8"][live], c["rgb8"][live])
    for k in ("primary_rays", "hit_rays", "shadow_rays"):
        assert o["stats"][k] == c["stats"][k], (what, k, o["stats"][k], c["stats"][k])
