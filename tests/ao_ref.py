"""The yardstick of the ambient-occlusion queries (include/srt.h, "Ambient occlusion": srt_ao_rays, srt_ao_hits).  It adds no walk of its
own and calls nothing of the code under test:

  * the hit: visibility_ref.closest on ray_range_ref.candidates, with the call's interval and the mask vis.primary;
  * P and N: surface_ref.surface's `point` and `normal` (the smooth one under smooth=True), obj its `obj`;
  * frame(d, N) and ao_rays(P, T, B, Nf, dirs): the header's definition restated in numpy float32, every step its own array operation
    (nothing is contracted);
  * blocked: ray_range_ref.candidates on the AO rays, then visibility_ref.occluded with the interval (t_min, t_max), the mask vis.shadow and
    skip_obj = obj under skip_self;
  * n_occluded, ao = (float32)(K - n_occluded) / (float32)K, occ_bits: bit k & 31 of word k >> 5.

The candidate set of an AO ray depends on neither the interval, the skip nor a mask, so a Case asks for it once and answers every variant
from it.  tests/test_ao_ref.py pins the frame and the input conditions of the GPU cases on this file alone."""
import numpy as np

import ray_range_ref as rr
import shadow_rule_ref as sh
import surface_ref as sf
import visibility_ref as vr

F32 = np.float32
ALL = 0xFFFFFFFF
FIELDS = ("n_occluded", "ao", "occ_bits")
T_MIN = 1e-3


def directions(n, cosine=True):
    """lib.ao_directions restated: float64, rounded once."""
    i = np.arange(int(n), dtype=np.float64)
    u = (i + 0.5) / float(n)
    if cosine:
        r = np.sqrt(u); z = np.sqrt(1.0 - r * r)
    else:
        z = 1.0 - u; r = np.sqrt(1.0 - z * z)
    phi = (i + 0.5) * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def frame(d, N, dtype=np.float32):
    """(T, B, Nf) of the header's definition for directions d and normals N (n x 3 each), in `dtype`."""
    d, N = np.ascontiguousarray(d, dtype).reshape(-1, 3), np.ascontiguousarray(N, dtype).reshape(-1, 3)
    one = dtype(1.0)
    with np.errstate(all="ignore"):
        k = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
        Nf = np.where((k > 0)[:, None], -N, N).astype(dtype)
        x, y, z = Nf[:, 0], Nf[:, 1], Nf[:, 2]
        s = np.copysign(one, z).astype(dtype)
        a = (-one) / (s + z)
        b = (x * y) * a
        T = np.stack([one + ((s * x) * x) * a, s * b, (-s) * x], axis=1).astype(dtype)
        B = np.stack([b, s + (y * y) * a, -y], axis=1).astype(dtype)
    return T, B, Nf


def ao_rays(P, T, B, Nf, dirs):
    """The n x K AO rays (n x K x 6, float32): origin P, direction (T * u + B * v) + Nf * w for (u, v, w) = dirs[j]."""
    P, T, B, Nf = (np.ascontiguousarray(a, np.float32).reshape(-1, 1, 3) for a in (P, T, B, Nf))
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(1, -1, 3)
    with np.errstate(all="ignore"):
        tu = T * dirs[:, :, 0:1]
        bv = B * dirs[:, :, 1:2]
        nw = Nf * dirs[:, :, 2:3]
        w = ((tu + bv) + nw).astype(np.float32)
    return np.concatenate([np.broadcast_to(P, w.shape), w], axis=2).astype(np.float32)


def pack(blocked):
    """n x K bool -> (n_occluded n uint32, ao n float32, occ_bits n x W uint32)."""
    n, K = blocked.shape
    W = (K + 31) // 32
    padded = np.zeros((n, W * 32), bool); padded[:, :K] = blocked
    words = (padded.reshape(n, W, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)
    cnt = blocked.sum(axis=1).astype(np.uint32)
    ao = ((np.uint32(K) - cnt).astype(np.float32) / np.float32(K)).astype(np.float32)
    return cnt, ao, words


def unpack(occ_bits, K):
    """n x W uint32 -> n x K bool."""
    w = np.ascontiguousarray(occ_bits, np.uint32)
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool).reshape(w.shape[0], -1)[:, :K]


class Case:
    """One batch of rays, one table, one set of hits: the surface, the AO rays and their candidate sets, asked for once.  hits: (hit_id, t)
    a caller brings (srt_ao_hits), else the closest hits under (t_range, primary mask, obj_mask)."""

    def __init__(self, oracle, flat, rays, dirs, t_range=None, primary=None, obj_mask=None, smooth=False, hits=None):
        self.flat, self.obj_mask = flat, obj_mask
        self.rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        self.dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        if hits is None:
            tr = None if t_range is None else np.ascontiguousarray(t_range, np.float32).reshape(-1, 2)
            self.hit, self.t = vr.closest(rr.candidates(oracle, flat, self.rays), flat, primary, obj_mask, tr)
        else:
            self.hit, self.t = np.asarray(hits[0], np.int32).reshape(-1), np.asarray(hits[1], np.float32).reshape(-1)
        s = sf.surface(oracle, flat, self.rays, self.hit, self.t, smooth)
        self.sel = np.flatnonzero(s["obj"] >= 0)
        self.obj = s["obj"][self.sel].astype(np.int64)
        self.T, self.B, self.Nf = frame(self.rays[self.sel, 3:6], s["normal"][self.sel])
        self.ao_rays = ao_rays(s["point"][self.sel], self.T, self.B, self.Nf, self.dirs)
        self.cand = rr.candidates(oracle, flat, self.ao_rays.reshape(-1, 6))

    def blocked(self, t_min=T_MIN, t_max=np.inf, skip_self=False, shadow=None, obj_mask="case"):
        """n_hits x K bool: srt_occluded_masked's answer for every AO ray."""
        K = self.dirs.shape[0]
        tr = np.tile(np.array([t_min, t_max], np.float32), (self.sel.size * K, 1))
        skip = np.repeat(self.obj, K) if skip_self else None
        table = self.obj_mask if isinstance(obj_mask, str) else obj_mask
        return vr.occluded(self.cand, self.flat, shadow, table, tr, skip).astype(bool).reshape(self.sel.size, K)

    def reference(self, t_min=T_MIN, t_max=np.inf, skip_self=False, shadow=None, obj_mask="case"):
        """The rows of the call: dict of hit_id, t, n_occluded, ao, occ_bits (a miss row: 0, 1.0, 0)."""
        n, K = self.rays.shape[0], self.dirs.shape[0]
        full = np.zeros((n, K), bool)
        full[self.sel] = self.blocked(t_min, t_max, skip_self, shadow, obj_mask)
        cnt, ao, words = pack(full)
        return {"hit_id": self.hit, "t": self.t, "n_occluded": cnt, "ao": ao, "occ_bits": words}


def ao(oracle, flat, rays, dirs, t_min=T_MIN, t_max=np.inf, t_range=None, skip_self=False, vis=None, obj_mask=None, smooth=False, hits=None):
    """srt_ao_rays (hits=None) / srt_ao_hits by the yardstick.  vis: None, or (primary, bounce, shadow)."""
    primary, shadow = (None, None) if vis is None else (vis[0], vis[2])
    return Case(oracle, flat, rays, dirs, t_range, primary, obj_mask, smooth, hits).reference(t_min, t_max, skip_self, shadow)


def conditions(ref, K):
    """The input conditions of a case (counts over its hits): rows fully open, rows with 0 < n_occluded < K, rows fully blocked."""
    cnt = ref["n_occluded"][ref["hit_id"] >= 0].astype(np.int64)
    return {"hits": int(cnt.size), "open": int((cnt == 0).sum()), "partial": int(((cnt > 0) & (cnt < K)).sum()), "closed": int((cnt == K).sum())}


# ---- the cases of tests/test_gpu_ao.py -------------------------------------------------------------------------------------------------
# The frames of shadow_rule_ref's lamp cases (the lamp itself plays no part), 16 cosine directions, t_min 1e-3, two radii.  ground_bunny
# costs the yardstick about 75 s for its 2304 rays, so that case takes every third ray.
N_DIRS = 16
RADII = (20.0, 60.0)
STRIDE = {"cube_ground": 1, "cubes4_a40": 1, "ground_bunny": 3}
_cases = {}


def case_rays(name):
    flat, rays, _, _ = sh.lamp_case(name)
    return flat, np.ascontiguousarray(rays[::STRIDE[name]])


def case(oracle, name):
    """The Case of a lamp case: computed once, shared, never changed."""
    if name not in _cases:
        flat, rays = case_rays(name)
        _cases[name] = Case(oracle, flat, rays, directions(N_DIRS))
    return _cases[name]


def assert_same(got, want, what, keys=None):
    """surface_ref.assert_same on the rows of an AO call."""
    sf.assert_same(got, want, what, keys if keys is not None else [k for k in want if k in got])
