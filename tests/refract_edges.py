"""A goniometer for refract_dir (include/srt.h, "Refracting paths"): one flat scene and one ray batch that put the formula's edges -- the
selects on k and c, the scaling by L, overflow, underflow and denormals -- through srt_shade_paths_refract.  Segment 1's ray in seg_rays IS
refract_dir's output, bit for bit, so no hook is needed.  Plain numpy; tests/test_refract_edges_ref.py proves on the yardstick that the
rows reach the cases, tests/test_gpu_refract_edges.py runs them on the device.

THE SCENE.  16 sheets side by side in x, each one axis-aligned quad of two triangles in the plane z = 0, of side S = 2^28: the triangle
test calls a ray parallel below |det| = 1e-12, and det is about |d| * 2 * area, so only a huge sheet is hit by a direction of length 1e-25.
Powers of two keep the face normal exactly (0, 0, +-1) (even sheets +1, odd sheets -1 by the winding).  Sheets 0..7 carry that face normal
at every vertex; sheets 8..10 carry (1, 0, 0) -- under the smooth build c is exactly +0 for d = (0, 0, s) -- and sheets 11..15 a different
tilted normal at every vertex.  Two mirrors (objects 16, 17) lie at z = -G and z = +G so that segment 1 hits something; they reach one sheet's side beyond the sheets and no
further, so that their own triangle test does not overflow under the longest directions.
The ior table holds 1, 1.5, 2, 0.5, nextafter(1, 2), 1e-20, a denormal (1e-40), 1e20, +inf and one 0 (a mirror, the control).

THE RAYS.  Every ray is aimed at a fixed interior point of its sheet from D = 2^18 away (between the sheet and a mirror), in the plane y = 0:
  * `angles`: per sheet 0, 1, 30, 60, 89 and 89.99 degrees from the normal, from both sides, each at |d| = 1, 1e-18, 1e-25 (d . d underflows:
    L = 0, inv = inf), 1e15, 1e19 (d . d = 1e38 is still finite) and 3e19 (d . d overflows: L = inf, inv = 0, I = 0, c = +0, r infinite or NaN);
  * `sweeps`: on the sheets with the exact normal and ior 1.5, 2, nextafter(1, 2) (their leaving side) and 0.5 (its entering side, the one
    that has a critical angle), 65 rays whose x component steps by one ulp across the place where the yardstick's k changes sign, found by
    bisection over the float's bits on the yardstick's own arithmetic.
Directions hold +0 only.  Everything is built once and read-only."""
import functools

import numpy as np

import refract_ref as rf
import tree_shapes as ts
from simple_raytracer_amd import abi

F32 = np.float32
S, G, D = 2.0 ** 28, 2.0 ** 20, 2.0 ** 18
N_SHEETS, BEHIND, FRONT = 16, 16, 17
ANGLES = (0.0, 1.0, 30.0, 60.0, 89.0, 89.99)
SCALES = (1.0, 1e-18, 1e-25, 1e15, 1e19, 3e19)
SWEEP = 65
DEPTH, BOUNCE_T_MIN = 3, 1e-3
ONE_UP = np.nextafter(F32(1.0), F32(2.0))
#            the exact normal (0, 0, +-1) at every vertex                      (1, 0, 0)        tilted
IOR = F32([1.0, 1.5, 2.0, 0.5, ONE_UP, 1e-40, 1e20, np.inf,                    1.0, 0.5, 2.0,   1.5, 1e-20, 1e20, ONE_UP, 0.0,   0.0, 0.0])
EXACT, C_ZERO, TILTED = range(0, 8), range(8, 11), range(11, 16)
SWEPT = (1, 2, 4, 3)                      # the sheets with a sweep; sheet 3 (ior 0.5) on its entering side
REFLECTANCE = (F32(0.2) + F32(0.15) * (np.arange(18) % 5).astype(np.float32)).astype(np.float32)
LIGHT = (7.3 * S, 0.3 * S, 0.6 * G)
KIND_ANGLE, KIND_SWEEP = 0, 1


def quad(x0, x1, y0, y1, z, up):
    """Two triangles sharing the diagonal (x0, y0) - (x1, y1); up: the face normal is (0, 0, +1), else (0, 0, -1)."""
    a, b, c, d = (x0, y0, z, 1.0), (x1, y0, z, 1.0), (x1, y1, z, 1.0), (x0, y1, z, 1.0)
    return np.float32([[a, b, c], [a, c, d]] if up else [[a, c, b], [a, d, c]])


def sheet_normal_sign(k):
    return 1.0 if k % 2 == 0 else -1.0


@functools.lru_cache(maxsize=None)
def scene():
    """The flat scene (with vertex normals: the smooth build reads them, the flat build the face normals)."""
    rng = np.random.default_rng(77)
    objs = []
    for k in range(N_SHEETS):
        sg = sheet_normal_sign(k)
        if k in EXACT:
            nrm = np.tile(F32([0.0, 0.0, sg]), (2, 3))
        elif k in C_ZERO:
            nrm = np.tile(F32([1.0, 0.0, 0.0]), (2, 3))
        else:
            v = rng.uniform(-0.5, 0.5, (2, 3, 3)); v[..., 2] = sg
            nrm = (v / np.linalg.norm(v, axis=2, keepdims=True)).reshape(2, 9)
        objs.append(dict(tris=quad(k * S, (k + 1) * S, 0.0, S, 0.0, sg > 0), leaves=(2,), shape="root_leaf", color=ts.COLORS[k % 5], material=ts.MATERIALS[k % 3],
                         normals=np.float32(nrm)))
    for z, up in ((-G, True), (G, False)):
        objs.append(dict(tris=quad(-S, 17 * S, -S, 2 * S, z, up), leaves=(2,), shape="root_leaf", color=ts.COLORS[3], material=ts.MATERIALS[1],
                         normals=np.tile(F32([0.0, 0.0, 1.0 if up else -1.0]), (2, 3))))
    flat = ts.flat_scene(objs)
    for a in (flat.tri_points, flat.tri_normals, flat.node_min, flat.node_max):
        a.setflags(write=False)
    return flat


def target(k):
    """The point of sheet k the rays are aimed at: inside its first triangle, away from the diagonal."""
    return np.float64([(k + 0.7) * S, 0.2 * S, 0.0])


def aimed(k, unit, scale=1.0):
    """The ray at target(k) along `unit` (float64, about unit length) from D away; its direction is float32(unit) * float32(scale)."""
    u = np.asarray(unit, np.float64)
    o = target(k) - u / np.linalg.norm(u) * D
    with np.errstate(all="ignore"):
        d = u.astype(np.float32) * F32(scale)
    return np.concatenate([o.astype(np.float32), np.where(d == 0, F32(0.0), d)]).astype(np.float32)


def k_negative(sx_bits, dz, nz, n):
    d = F32([[np.uint32(sx_bits).view(np.float32), 0.0, dz]])
    return bool(rf.refract_parts(d, F32([[0.0, 0.0, nz]]), F32([n]))[2][0] < 0)


def sweep_rays(k):
    """65 rays at sheet k on the side that has a critical angle, d = (sx, +0, dz): dz the critical angle's cosine, sx one ulp apart, the
    middle one the last whose k (on the yardstick, with the face normal) is not negative."""
    n, nz = float(IOR[k]), sheet_normal_sign(k)
    leaving = n > 1.0
    sin_c = 1.0 / n if leaving else n
    dz = F32(np.sqrt(1.0 - sin_c * sin_c)) * F32(nz if leaving else -nz)          # leaving: along the normal
    lo, hi = 0, int(F32(4.0 * sin_c).view(np.uint32))
    assert not k_negative(lo, dz, nz, IOR[k]) and k_negative(hi, dz, nz, IOR[k])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if k_negative(mid, dz, nz, IOR[k]):
            hi = mid
        else:
            lo = mid
    half = SWEEP // 2
    return np.stack([aimed(k, [float(np.uint32(b).view(np.float32)), 0.0, float(dz)]) for b in range(lo - half, lo + half + 1)])


@functools.lru_cache(maxsize=None)
def batch():
    """(rays n x 6, kind n, sheet n, scale n): the `angles` rays -- angle, side, scale, sheet, the sheet changing fastest, so that any
    leading part of the batch holds every ior -- then the sweeps."""
    rays, kind, sheet, scale = [], [], [], []
    for a in ANGLES:
        s, c = np.sin(np.radians(a)), np.cos(np.radians(a))
        for side in (1.0, -1.0):                                                  # from z > 0 heading down, from z < 0 heading up
            for sc in SCALES:
                for k in range(N_SHEETS):
                    rays.append(aimed(k, [s, 0.0, -side * c], sc)); kind.append(KIND_ANGLE); sheet.append(k); scale.append(sc)
    for k in SWEPT:
        r = sweep_rays(k)
        rays += list(r); kind += [KIND_SWEEP] * len(r); sheet += [k] * len(r); scale += [1.0] * len(r)
    out = (np.ascontiguousarray(np.stack(rays), np.float32), np.int32(kind), np.int32(sheet), np.float64(scale))
    assert not (np.signbit(out[0][:, 3:6]) & (out[0][:, 3:6] == 0)).any(), "a -0 direction component"
    for a in out:
        a.setflags(write=False)
    return out


def lights(n):
    return abi.light_staircase(np.float32(LIGHT), n)


def frame_params(n_lights=3, **kw):
    """A 16 x 16 camera-mode frame from half way between the sheets and the front mirror, looking down: pixel (i, j)'s direction is
    (i - 8, (j - 8) / 32, -2^-9), which reaches z = 0 at t = 2^28 = S -- column i on sheet i, every row inside the sheets' y range, the
    middle pixel at normal incidence and the outer columns at 83 degrees."""
    m = np.zeros(16, np.float32)
    m[0], m[5], m[10] = 1.0, 1.0 / 32, -1.0
    m[12:16] = [8.37 * S, 0.45 * S, 0.5 * G, 1.0]
    return abi.make_params(16, 16, lights(n_lights), focal=2.0 ** -9, ray_matrix=m, **kw)


def first_hits(oracle, smooth):
    """Segment 0 of the batch on the yardstick, and refract_ref.refract_steps for the rows that hit glass: (rows -- indices into the
    batch --, steps, d, N, n)."""
    import surface_ref as sf
    import visibility_ref as vr
    flat, rays = scene(), batch()[0]
    hit, t = vr.closest(vr.CandidateMemo(oracle, flat)(rays), flat, None, None)
    s = sf.surface(oracle, flat, rays, hit, t, smooth)
    with np.errstate(invalid="ignore"):
        rows = np.flatnonzero((s["obj"] >= 0) & (IOR[np.maximum(s["obj"], 0)] > 0))
    d, N, n = rays[rows, 3:6], s["normal"][rows], IOR[s["obj"][rows]]
    return rows, rf.refract_steps(d, N, n), d, N, n, s["obj"]
