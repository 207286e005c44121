"""The yardstick of the surface queries (include/srt.h, srt_surface_rays / srt_surface_hits), built on the existing helpers and the
oracle's leaf functions only -- nothing here calls the code under test:

  * hit_id, t: ray_range_ref (with an interval) or ray_query_ref.oracle_trace (without);
  * point: numpy float32 o + d * t, the product first, every step its own array operation (nothing is contracted);
  * obj, material and the object's colour: the flat scene's arrays at the hit;
  * the texel (softShadow:350-361): pyoracle.barycentric at the point, the two (a + b) + c sums, int() truncation, the index clamped to
    [0, w * h * 3 - 3], / 255.0f -- the restatement of tests/test_oracle_golden.py::_pixel_phong_rows, with the ray's own origin;
  * the flat normal: oracle/srt_oracle.c face_normal in numpy float32 -- raw xyz differences, glm::cross (a.y * b.z - b.y * a.z, ...),
    1.0f / sqrtf((x * x + y * y) + z * z), scale;
  * the smooth normal: pyoracle.interp_normal on the triangle's nine normals and pyoracle.barycentric at the point;
  * the mirrored ray: origin = point, r_i = d_i - (N_i * k) * 2 with k = (d.x * N.x + d.y * N.y) + d.z * N.z, numpy float32.

A miss row: obj -1, every float 0.  tests/test_surface_ref.py ties the colour, the material and the normal to the oracle's own shading."""
import numpy as np

import ray_query_ref as rq
import ray_range_ref as rr

F32 = np.float32
FIELDS = {"obj": 1, "point": 3, "normal": 3, "color": 3, "material": 3, "bounce": 6}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hits(oracle, flat, rays, t_range=None):
    """(hit_id, t) of every ray: the oracle's 1 x 1 frames, or ray_range_ref's closest hit inside the ray's interval."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    if t_range is None:
        return rq.oracle_trace(oracle, flat, rays)
    return rr.closest(rr.candidates(oracle, flat, rays), np.ascontiguousarray(t_range, np.float32).reshape(-1, 2))


def points(rays, t):
    """o + d * t in float32: one multiply, one add per component."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    with np.errstate(all="ignore"):
        dt = rays[:, 3:6] * np.asarray(t, np.float32).reshape(-1, 1)
        return (rays[:, 0:3] + dt).astype(np.float32)


def face_normal(pts12):
    """calculateTriangleNormal:32-37 as oracle/srt_oracle.c restates it, on n x 12 raw points (xyzw a vertex)."""
    p = np.ascontiguousarray(pts12, np.float32).reshape(-1, 12)
    with np.errstate(all="ignore"):
        ax, ay, az = p[:, 4] - p[:, 0], p[:, 5] - p[:, 1], p[:, 6] - p[:, 2]
        bx, by, bz = p[:, 8] - p[:, 0], p[:, 9] - p[:, 1], p[:, 10] - p[:, 2]
        cx = ay * bz - by * az
        cy = az * bx - bz * ax
        cz = ax * by - bx * ay
        s = F32(1.0) / np.sqrt((cx * cx + cy * cy) + cz * cz)
        return np.stack([cx * s, cy * s, cz * s], axis=1).astype(np.float32)


def reflect(d, N):
    """glm::reflect's association in float32: d - (N * dot(N, d)) * 2, dot = (x + y) + z."""
    d, N = np.ascontiguousarray(d, np.float32).reshape(-1, 3), np.ascontiguousarray(N, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        k = (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]
        nk = N * k[:, None]
        return (d - nk * F32(2.0)).astype(np.float32)


def texel(oracle, flat, h, P):
    """The colour softShadow:350-361 reads for triangle h (textured) at point P."""
    tex = int(flat.tri_tex[h])
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 12)[h]
    bc = oracle.barycentric(np.concatenate([pts, P]).astype(np.float32)[None])[0]
    tc = np.asarray(flat.tri_texcoord, np.float32).reshape(-1, 6)[h]
    tx = (bc[0] * tc[0] + bc[1] * tc[2]) + bc[2] * tc[4]
    ty = (bc[0] * tc[1] + bc[1] * tc[3]) + bc[2] * tc[5]
    w, hh = int(flat.tex_w[tex]), int(flat.tex_h[tex])
    i = min(max((int(ty) * w + int(tx)) * 3, 0), w * hh * 3 - 3)
    td = flat.tex_rgb[int(flat.tex_off[tex]) + i:][:3]
    return td.astype(np.float32) / F32(255.0)


def surface(oracle, flat, rays, hit, t, smooth=False):
    """The rows of srt_surface_out for the hits (hit, t) of `rays`: dict of obj n int32, point / normal / color / material n x 3,
    bounce n x 6."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    hit = np.asarray(hit, np.int32).reshape(-1)
    n = rays.shape[0]
    out = {"obj": np.full(n, -1, np.int32)}
    for k in ("point", "normal", "color", "material"):
        out[k] = np.zeros((n, 3), np.float32)
    out["bounce"] = np.zeros((n, 6), np.float32)
    sel = np.flatnonzero((hit >= 0) & (hit < flat.n_tris))
    if sel.size == 0:
        return out
    h = hit[sel].astype(np.int64)
    obj = flat.tri_obj[h].astype(np.int64)
    P = points(rays[sel], np.asarray(t, np.float32).reshape(-1)[sel])
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 12)[h]
    out["obj"][sel] = obj
    out["point"][sel] = P
    out["material"][sel] = np.asarray(flat.obj_material, np.float32).reshape(-1, 3)[obj]
    color = np.asarray(flat.obj_color, np.float32).reshape(-1, 3)[obj].copy()
    if flat.tri_tex is not None:
        for k in np.flatnonzero(flat.tri_tex[h] >= 0):
            color[k] = texel(oracle, flat, int(h[k]), P[k])
    out["color"][sel] = color
    if smooth:
        bc = oracle.barycentric(np.concatenate([pts, P], axis=1))
        n9 = np.asarray(flat.tri_normals, np.float32).reshape(-1, 9)[h]
        N = oracle.interp_normal(np.concatenate([n9, bc], axis=1))
    else:
        N = face_normal(pts)
    out["normal"][sel] = N
    out["bounce"][sel, 0:3] = P
    out["bounce"][sel, 3:6] = reflect(rays[sel, 3:6], N)
    return out


def surface_rays(oracle, flat, rays, t_range=None, smooth=False):
    """srt_surface_rays by the yardstick: dict of hit_id, t and the six fields."""
    hit, t = hits(oracle, flat, rays, t_range)
    out = surface(oracle, flat, rays, hit, t, smooth)
    out["hit_id"], out["t"] = hit, t
    return out


def assert_same(got, want, what, keys=None):
    """Every array of `want` named in keys (default: those `got` holds) equals `got`'s: ints by value, floats by bits; where the
    yardstick is NaN the device must be NaN."""
    for k in (keys if keys is not None else [k for k in want if k in got]):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if w.dtype == np.float32:
            nan = np.isnan(w)
            bad = np.where(nan, ~np.isnan(g), bits(g) != bits(w))
        else:
            bad = g != w
        if bad.any():
            rows = np.flatnonzero(bad.reshape(bad.shape[0], -1).any(axis=1))
            r = int(rows[0])
            raise AssertionError(f"{what}: {k} differs in {rows.size} of {bad.shape[0]} rows, first at row {r}: got {g[r]}, want {w[r]}")
