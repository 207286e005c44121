"""The yardstick of ambient occlusion in a frame (include/srt.h, "Ambient occlusion in a frame": srt_render_ao, srt_render_ao_hits).  It
adds no walk and calls nothing of the code under test:

  * the rays are render_paths_ref.frame_rays_owned(p, k): the local pixels of a call with params p, sub-sample k;
  * rotate(dirs, c, s): the header's rotation in numpy float32, every product and sum its own array operation;
  * the pixels are grouped by their entry of the rotation table -- (y % rot_h) * rot_w + x % rot_w of the IMAGE pixel --, each group is
    answered by ao_ref.Case with that group's table, and the rows are scattered back;
  * bent: ao_ref.Case's AO rays (ao_ref.frame / ao_ref.ao_rays) and the unblocked bits, summed one direction after the other in ascending
    j, float32;
  * ao8 and the spp rule as the header states them.

Padding pixels (owned_pixels == -1) carry no ray and come back as `fill`."""
import numpy as np

import ao_ref as ar
import render_paths_ref as rp

F32 = np.float32
FIELDS = ("n_occluded", "ao", "occ_bits", "bent", "ao8")
ALL = ("hit_id", "t") + FIELDS
DTYPE = {"hit_id": np.int32, "t": np.float32, "n_occluded": np.uint32, "ao": np.float32, "occ_bits": np.uint32, "bent": np.float32, "ao8": np.uint8}
GOLDEN = 0.6180339887498949


def rotations(w, h):
    """lib.ao_rotations restated: entry k = iy * w + ix has the angle 2 pi frac((k + 0.5) * 0.6180339887498949), float64, rounded once."""
    k = np.arange(int(w) * int(h), dtype=np.float64)
    a = 2.0 * np.pi * np.modf((k + 0.5) * GOLDEN)[0]
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32).reshape(int(h), int(w), 2)


def rotate(dirs, c, s):
    """The table of a pixel whose rotation is (c, s): u' = c * u - s * v, v' = s * u + c * v, w' = w; each product rounded on its own."""
    d = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    c, s = F32(c), F32(s)
    with np.errstate(all="ignore"):
        cu = (c * d[:, 0]).astype(np.float32)
        sv = (s * d[:, 1]).astype(np.float32)
        su = (s * d[:, 0]).astype(np.float32)
        cv = (c * d[:, 1]).astype(np.float32)
        u = (cu - sv).astype(np.float32)
        v = (su + cv).astype(np.float32)
    return np.ascontiguousarray(np.stack([u, v, d[:, 2]], axis=1), np.float32)


def rot_entry(p, rot):
    """[rows_local, cols_local]: the entry of the rotation table (rot_h x rot_w x 2) of each local pixel, by its IMAGE pixel; 0 without a
    table; -1 = padding."""
    own = rp.owned(p)
    if rot is None:
        return np.where(own >= 0, 0, -1)
    rh, rw = rot.shape[:2]
    x, y = own % int(p.width), own // int(p.width)
    return np.where(own >= 0, (y % rh) * rw + x % rw, -1)


def bent_sum(w, blocked):
    """n x K x 3 directions, n x K blocked -> n x 3: from (+0, +0, +0), the unblocked directions added in ascending j, one float32 add a
    component."""
    acc = np.zeros((w.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for j in range(w.shape[1]):
            acc = np.where(blocked[:, j, None], acc, (acc + w[:, j]).astype(np.float32)).astype(np.float32)
    return acc


def ao8_of(ao):
    with np.errstate(all="ignore"):
        x = (np.asarray(ao, np.float32) * F32(255.0)).astype(np.float32)
        x = (x + F32(0.5)).astype(np.float32)
    return x.astype(np.int32).astype(np.uint8)


def sub_sample(oracle, flat, p, k, dirs, rot, t_min, t_max, skip_self, vis, obj_mask, smooth, hits):
    """The flat rows (n local pixels; padding rows are miss rows) of sub-sample k."""
    rays, live = rp.frame_rays_owned(p, k)
    rays = rays.reshape(-1, 6)
    entry = rot_entry(p, rot).reshape(-1)
    n, K = rays.shape[0], np.asarray(dirs).reshape(-1, 3).shape[0]
    W = (K + 31) // 32
    out = {"hit_id": np.full(n, -1, np.int32), "t": np.full(n, np.inf, np.float32), "n_occluded": np.zeros(n, np.uint32), "ao": np.ones(n, np.float32),
           "occ_bits": np.zeros((n, W), np.uint32), "bent": np.zeros((n, 3), np.float32)}
    primary, shadow = (None, None) if vis is None else (vis[0], vis[2])
    for e in np.unique(entry[entry >= 0]):
        idx = np.flatnonzero(entry == e)
        table = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3) if rot is None else rotate(dirs, *rot.reshape(-1, 2)[e])
        given = None if hits is None else (np.asarray(hits[0]).reshape(-1)[idx], np.asarray(hits[1]).reshape(-1)[idx])
        c = ar.Case(oracle, flat, rays[idx], table, None, primary, obj_mask, smooth, given)
        blocked = c.blocked(t_min, t_max, skip_self, shadow)
        full = np.zeros((idx.size, K), bool)
        full[c.sel] = blocked
        cnt, ao, words = ar.pack(full)
        bent = np.zeros((idx.size, 3), np.float32)
        bent[c.sel] = bent_sum(c.ao_rays[:, :, 3:6], blocked)
        for key, v in (("hit_id", c.hit), ("t", c.t), ("n_occluded", cnt), ("ao", ao), ("occ_bits", words), ("bent", bent)):
            out[key][idx] = v
    return out, live.reshape(-1)


def render_ao(oracle, flat, p, dirs, rot=None, t_min=ar.T_MIN, t_max=np.inf, skip_self=False, vis=None, obj_mask=None, smooth=False, hits=None, fill=None):
    """srt_render_ao (hits=None) / srt_render_ao_hits (hits = (hit_id, t), frame-shaped) by the yardstick: dict of hit_id, t, n_occluded,
    ao, ao8 [rows, cols], occ_bits [rows, cols, W], bent [rows, cols, 3], and 'hit_rays': the hits of all sub-samples walked."""
    spp = 1 if hits is not None else int(p.spp)
    first, live = sub_sample(oracle, flat, p, 0, dirs, rot, t_min, t_max, skip_self, vis, obj_mask, smooth, hits)
    total = first["ao"].copy()
    hit_rays = int((first["hit_id"][live] >= 0).sum()) if hits is None else int(((first["hit_id"] >= 0) & (first["hit_id"] < flat.n_tris))[live].sum())
    for k in range(1, spp):
        o, _ = sub_sample(oracle, flat, p, k, dirs, rot, t_min, t_max, skip_self, vis, obj_mask, smooth, None)
        total = (total + o["ao"]).astype(np.float32)
        hit_rays += int((o["hit_id"][live] >= 0).sum())
    if spp > 1:
        total = (total / F32(spp)).astype(np.float32)
    first["ao"] = total
    first["ao8"] = ao8_of(total)
    shape = rp.owned(p).shape
    out = {}
    for key in ALL:
        v = first[key].copy()
        if fill is not None:
            v[~live] = fill
        elif key in ("hit_id", "t", "ao", "ao8"):
            v[~live] = 0
        out[key] = v.reshape(shape + v.shape[1:])
    out["hit_rays"] = hit_rays
    return out


def conditions(ref, K):
    """The input conditions of a frame case: live pixels, hits, rows with 0 < n_occluded < K."""
    hit = ref["hit_id"] >= 0
    cnt = ref["n_occluded"][hit].astype(np.int64)
    return {"pixels": int(hit.size), "hits": int(hit.sum()), "partial": int(((cnt > 0) & (cnt < K)).sum())}


# ---- the cases of tests/test_gpu_render_ao.py ------------------------------------------------------------------------------------------
# ao_ref's lamp frames (shade_path_ref.FRAMES at 48 x 27, camera mode), 16 cosine directions, a 4 x 4 table of rotations, two radii.
NAMES = ("cube_ground", "cubes4_a40")
SIZE = (48, 27)
N_DIRS = ar.N_DIRS
RADII = ar.RADII
ROT = (4, 4)
_refs = {}


def case(name, **kw):
    """(flat, params) of a frame case."""
    import shadow_rule_ref as sh
    flat, _, lights, _ = sh.lamp_case(name)
    return flat, rp.camera_params(name, lights, SIZE[0], SIZE[1], **kw)


def case_reference(oracle, name, t_max, rotated=True):
    """The yardstick's frame of a case: computed once, shared, never changed."""
    key = (name, float(t_max), rotated)
    if key not in _refs:
        flat, p = case(name)
        ref = render_ao(oracle, flat, p, ar.directions(N_DIRS), rotations(*ROT) if rotated else None, t_max=t_max)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def assert_same(got, want, what, keys=ALL, where=None):
    """Frame-shaped rows equal: ints by value, floats by bits (a NaN of the reference: any NaN), everywhere or where `where` holds."""
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if where is not None:
            g, w = g[where], w[where]
        if w.dtype == np.float32:
            gb, wb = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
            ok = (gb == wb) | (np.isnan(g) & np.isnan(w))
        else:
            ok = g == w
        assert ok.all(), (what, k, int((~ok).sum()), "differ")
