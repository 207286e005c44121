"""A goniometer for the frame of the ambient-occlusion queries (include/srt.h, "Ambient occlusion"): one flat scene and its batches that
put the arithmetic srt_ao_rays / srt_ao_hits add -- the dot k and the flip to the facing normal, the branch-free tangent frame, the
three-term ray w = (T * u + B * v) + Nf * w, the closed AO interval -- at its edges.  Plain numpy and the yardstick (tests/ao_ref.py);
tests/test_ao_edges_ref.py proves on the yardstick that the rows reach the cases and that a subtly wrong kernel would be seen,
tests/test_gpu_ao_edges.py runs them on the device.

THE SCENE.  A grid of cells SPACING = 64 apart (5 x 5 a layer, the layers at z = 0, -64, 64, ...), every batch's t_max at most T_MAX = 16:
an AO ray of a unit table never leaves its cell.  A cell holds
  * one small FACET at its centre (legs of length 1, v0 = centre - (a + b) / 4), carrying vertex normals, so the smooth builds run on the
    same scene; the facet and the first coarse blocker are one object, so that SRT_AO_SKIP_SELF changes rows;
  * its blockers, a second object: N_COARSE - 1 more coarse triangles, each in a plane 5 to 8 from the centre, bunched on one side of the
    sphere (roughly half of any hemisphere is covered, anisotropically), and the AIMED triangles of its hits (below).
The facets, by kind (a row's CLASS is decided by the yardstick's Nf: classify()):
  pole       a = (1, 0, 0), b = (0, 1, 0): the face normal is exactly (0, 0, 1); hit from both sides: Nf = (0, 0, +1) and (-0, -0, -1)
  equator    the planes x = 0 and y = 0 in either winding: N = (+-1, 0, +-0) and (+-0, +-1, +-0); hit from both sides, so that N and
             neg(N) both face a ray: Nf.z = +0 and -0
  tilt       a = (1, 0, -ex), b = (0, 1, -ey): N = normalize(ex, ey, 1) for (e, 0), (0, e), (e, -e), e = 2^-8, 2^-12, 2^-13, 2^-20, 2^-30;
             every such vertex is exact in float32 (these cells lie in the layer z = 0).  From 2^-12 on z rounds to +-1 with x, y != 0
  general    64 face normals over the sphere (a Fibonacci lattice); a slightly different normal at every vertex, so that under the smooth
             build every row has a frame of its own
  and, telling only under SRT_FLAG_SMOOTH_NORMALS (under the flat build they are four more poles):
  b_sub      equal vertex normals (2^-70, +-2^-70, +-1): b = (x * y) * a is a nonzero subnormal
  b_zero     equal vertex normals (2^-80, 2^-80, +-1): x * y underflows, b == 0 with x * y != 0
  per_vertex a different tilted normal at every vertex (four facets)
  zero       every vertex normal zero: normalize3 gives 0 * inf = NaN
  nan        one vertex normal NaN
  and two cells without rays of the main batch: a ZERO-AREA triangle (three collinear points) and a triangle with a NaN vertex, each an
  object of its own (srt_scene_create validates no coordinate; a NaN box is never entered), named by rows of the hits batch.

THE MAIN BATCH (batch()).  Per facet 4 points inside it (2 on a general facet), each hit from both sides from 0.5 away by a ray of length
2 (t = 0.25) that leans away from the normal: every ray hits its facet, nothing else is nearer.

THE HITS BATCH (hits_batch()): rows for srt_ao_hits only, each with a VALID id.
  sweep      on four general facets 65 rays each, o = the facet's centroid, t = 0, d.x stepping by one ulp across the place where the
             yardstick's k changes sign (bisection over the float's bits, as refract_edges.k_negative does)
  k_zero     on the facets whose face normal is (0, 0, +-1): d = (1, 0, 0), (1, 0, -0.0), (0, 1, 0) (k = +0) and (-1, -1, -0.0) (k = -0)
  k_nan      d with an inf component against a zero of N; P = o + d * 0 has ONE NaN component (the rows that found the slab filter
             dropping a NaN origin axis: test_gpu_ao_edges.py::test_a_nan_origin_component_goes_to_the_exact_slab_test)
  odd_t      main rays with their own facet's id and t = NaN, +inf, -inf, 0, -0, -3, 1e30 and the t of the NEXT triangle on the ray
             (a point off the facet: the smooth build extrapolates the normal from barycentrics outside the triangle)
  degenerate rows naming the zero-area triangle and the triangle with a NaN vertex
  flush      on the b_sub facets, o an exact point, d = (0, 0, -+1), t = 0: the rows of the subnormal flush (below)

AIMED EDGES (aimed()).  For a pair (row, entry j of T16) whose bit is open among the coarse blockers, the yardstick's own AO ray (P, w) gets a
triangle of its own AIM_AT = 10 along w: one edge passes the point P + 10 w, from A (0.05 before it along the edge) to B (3 beyond it), the
third vertex 2.5 inside.  B's offset across the edge is bisected in float64 -- the vertices rounded to float32 -- on oracle.ray_triangle
until it flips between hit and miss; the last offset that still hits is kept.  B's lever (one ulp of B moves the edge 1/60 ulp at the ray)
makes the margin finer than a vertex's ulp, which at these coordinates is larger than the step of a ray whose w moves by one ulp.  Pairs come
from the flat frames of the main batch (one or two a row), from its smooth frames on the kinds that differ there (two or three a row) (srt_ao_rays) and from the two ends of every sweep (srt_ao_hits); a pair is KEPT if the
yardstick calls it blocked on the finished scene and clear with its own triangle cut from the candidates.
THE SUBNORMAL FLUSH (flush()).  b = -+2^-141 is absorbed by every sum of a T16 entry, so no T16 pair can see it.  T_ODD's entries (0, 1, 0)
and (1, 0, 0) give w = (b, ., .) and (., s * b, .): the ray from an exact P drifts off the plane x = P.x (y = P.y) by a subnormal, and a
triangle FLUSH_AT = 2 along the ray with an edge IN that plane, lying on the other side, is missed (v is a negative subnormal) -- with b
flushed to zero v = 0 hits.  These triangles lie inside the shell of the coarse blockers, and the hits batch runs T_ODD with t_max =
FLUSH_T_MAX = 4, short of the shell: nothing else can decide these bits.

TABLES.  T16 = ao_ref.directions(16); T7 its first 7 entries (below SRT_AO_SPREAD_FROM = 8: the other deal); T_ODD 40 entries: the horizon
with +0 and -0 components, below the horizon, the zero vector, NaN, +-inf, lengths 1e-20, 1e20 and 3e19, denormal components, and five
entries of T16; T33 and T1024 = directions(., cosine=False) (a second word with one live bit; sixteen chunks, W = 32) on small_batch(), 70
rays.  INTERVALS (intervals()): the calls of (e) around t*, the yardstick's t of one kept pair's own blocker, on interval_batch().
Everything is built once and read-only."""
import functools
import types

import numpy as np

import ao_ref as ar
import ray_range_ref as rr
import surface_ref as sf
import tree_shapes as ts

F32, F64 = np.float32, np.float64
SPACING, T_MAX, T_MIN, AIM_AT = 64.0, 16.0, ar.T_MIN, 10.0
FLUSH_AT, FLUSH_T_MAX = 2.0, 4.0      # the flush triangles lie inside the shell of the coarse blockers; their call stops short of it
N_COARSE, LEAF = 10, 24
SWEEP = 65
K = 16
T16 = ar.directions(K)
T7 = T16[:7]
T33, T1024 = ar.directions(33, cosine=False), ar.directions(1024, cosine=False)
TILT_E = (2.0 ** -8, 2.0 ** -12, 2.0 ** -13, 2.0 ** -20, 2.0 ** -30)
NAN, INF = F32(np.nan), F32(np.inf)
ODD_T = (NAN, INF, -INF, F32(0.0), F32(-0.0), F32(-3.0), F32(1e30))
CLASSES = ("pole+", "pole-", "equator+0", "equator-0", "tilt+", "tilt-", "b_sub", "b_zero", "nan", "general")
SMOOTH_KINDS = ("b_sub", "b_zero", "per_vertex", "zero", "nan")
for _t in (T16, T7, T33, T1024):
    _t.setflags(write=False)


def _odd_table():
    d = 1e-40
    rows = [(0, 1, 0), (1, 0, 0), (0, 0, 1), (-0.0, 1, 0), (1, -0.0, -0.0), (0, -1, 0.0), (-1, 0, 0),                  # the horizon, +0 / -0
            (0.3, 0.2, -0.9), (0, 0, -1), (0.6, -0.6, -0.5), (-0.7, 0.1, -0.1),                                         # below the horizon
            (0, 0, 0), (-0.0, -0.0, -0.0),                                                                             # the zero vector
            (NAN, 0, 1), (0, NAN, 0.5), (0.2, 0.3, NAN), (NAN, NAN, NAN),
            (INF, 0, 1), (0, -INF, 1), (0, 0, INF), (0, 0, -INF), (INF, INF, INF), (-INF, 0.5, 0.5),
            (d, 0.5, 0.8), (0.5, -1e-42, 0.7), (0.3, 0.4, 1e-45), (1e-45, -1e-45, 1e-45)]                               # denormal components
    t = [F32(r) for r in rows]
    with np.errstate(over="ignore"):
        for j, s in ((3, 1e-20), (12, 1e-20), (5, 1e20), (10, 1e20), (9, 3e19), (1, 3e19), (14, 3e19), (7, 1e20)):      # lengths: 3e19 squared overflows
            t.append(T16[j] * F32(s))
    t += [T16[j] for j in (0, 4, 8, 12, 15)]
    out = np.ascontiguousarray(np.stack(t), np.float32)
    out.setflags(write=False)
    return out


T_ODD = _odd_table()
ODD_UP, ODD_RIGHT = 0, 1                                    # T_ODD's (0, 1, 0) and (1, 0, 0): the entries of the subnormal flush
ODD_FINITE = np.flatnonzero(np.isfinite(T_ODD).all(axis=1) & (T_ODD != 0).any(axis=1))


def cell_centre(c):
    layer = (0, -1, 1, -2, 2)[c // 25]
    return F64([(c % 5 - 2) * SPACING, (c // 5 % 5 - 2) * SPACING, layer * SPACING])


def tangents(n):
    """Two unit vectors a, b with a x b = n / |n| (float64)."""
    n = F64(n) / np.linalg.norm(n)
    h = F64([1.0, 0.0, 0.0]) if abs(n[0]) < 0.6 else F64([0.0, 1.0, 0.0])
    a = np.cross(h, n); a /= np.linalg.norm(a)
    return a, np.cross(n, a)


def fibonacci(n):
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * np.pi * (3.0 - np.sqrt(5.0))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def facet_specs():
    """[(kind, a, b, vertex normals 3 x 3 or None: the face normal)] in cell order; the exact kinds first (the layer z = 0)."""
    X, Y, Z = F64([1, 0, 0]), F64([0, 1, 0]), F64([0, 0, 1])
    specs = [("pole", X, Y, None), ("pole", Y, X, None), ("equator", Y, Z, None), ("equator", Z, X, None)]
    for e in TILT_E:
        for ex, ey in ((e, 0.0), (0.0, e), (e, -e)):
            specs.append(("tilt", F64([1, 0, -ex]), F64([0, 1, -ey]), None))
    eq = lambda v: np.tile(F32(v), (3, 1))
    specs += [("b_sub", X, Y, eq([2.0 ** -70, 2.0 ** -70, 1.0])), ("b_sub", X, Y, eq([2.0 ** -70, -2.0 ** -70, -1.0])),
              ("b_zero", X, Y, eq([2.0 ** -80, 2.0 ** -80, 1.0])), ("b_zero", Y, X, eq([2.0 ** -80, 2.0 ** -80, -1.0])),
              ("zero", X, Y, eq([0.0, 0.0, 0.0])), ("nan", X, Y, F32([[0, 0, 1], [NAN, 0, 1], [0, 0, 1]]))]
    assert len(specs) == 25
    rng = np.random.default_rng(9)
    for n in fibonacci(64):
        a, b = tangents(n)
        v = n + rng.uniform(-0.15, 0.15, (3, 3))
        specs.append(("general", a, b, F32(v / np.linalg.norm(v, axis=1, keepdims=True))))
    for n in fibonacci(4) * 0.8 + 0.1:
        a, b = tangents(n)
        v = n / np.linalg.norm(n) + rng.uniform(-0.4, 0.4, (3, 3))
        specs.append(("per_vertex", a, b, F32(v / np.linalg.norm(v, axis=1, keepdims=True))))
    specs += [("equator", Z, Y, None), ("equator", X, Z, None)]                      # N = (-1, 0, 0) and (0, -1, 0) (exact in any layer)
    return specs


def facet_points(c, a, b):
    """The facet of cell c: 3 x 4 float32."""
    v0 = cell_centre(c) - (a + b) / 4
    p = np.ones((3, 4), np.float32)
    p[:, :3] = np.stack([v0, v0 + a, v0 + b]).astype(np.float32)
    return p


def coarse_blockers(c):
    """N_COARSE triangles, each in a plane 5..8 from the cell's centre, bunched about one direction."""
    rng = np.random.default_rng(1000 + c)
    lean = rng.standard_normal(3); lean /= np.linalg.norm(lean)
    out = np.ones((N_COARSE, 3, 4), np.float32)
    for k in range(N_COARSE):
        u = rng.standard_normal(3) * F64([1.0, 0.6, 1.0]) + 0.9 * lean
        u /= np.linalg.norm(u)
        p, q = tangents(u)
        ang = rng.uniform(0, 2 * np.pi) + F64([0.0, 2.1, 4.2]) + rng.uniform(-0.4, 0.4, 3)
        R = rng.uniform(3.0, 6.5)
        out[k, :, :3] = (cell_centre(c) + u * rng.uniform(5.0, 8.0) + (np.outer(np.cos(ang), p) + np.outer(np.sin(ang), q)) * R).astype(np.float32)
    return out


TARGETS = ((0.2, 0.3), (0.5, 0.2), (0.25, 0.6), (0.4, 0.4))


def main_rays(specs):
    """(rays n x 6, cell n, side n): per facet its targets from both sides."""
    rays, cell, side = [], [], []
    rng = np.random.default_rng(21)
    for c, (kind, a, b, _) in enumerate(specs):
        n = np.cross(a, b); n /= np.linalg.norm(n)
        v0 = cell_centre(c) - (a + b) / 4
        for (s, t) in TARGETS[:2 if kind == "general" else 4]:
            for sg in (1.0, -1.0):
                q = v0 + s * a + t * b
                o = q + sg * 0.5 * n + (a * rng.uniform(-0.2, 0.2) + b * rng.uniform(-0.2, 0.2))
                o32 = o.astype(np.float32)
                d = ((q - o32.astype(F64)) * 4.0).astype(np.float32)              # t = 0.25
                rays.append(np.concatenate([o32, np.where(d == 0, F32(0.0), d)])); cell.append(c); side.append(sg)
    return np.ascontiguousarray(np.stack(rays), np.float32), np.int32(cell), np.float64(side)


def degenerate_tris(c0):
    """The zero-area triangle (cell c0) and the triangle with a NaN vertex (cell c0 + 1)."""
    z = np.ones((1, 3, 4), np.float32); n = np.ones((1, 3, 4), np.float32)
    z[0, :, :3] = (cell_centre(c0) + F64([[0, 0, 0], [1, 1, 0], [2, 2, 0]])).astype(np.float32)
    n[0, :, :3] = (cell_centre(c0 + 1) + F64([[0, 0, 0], [1, 0, 0], [0, 1, 0]])).astype(np.float32)
    n[0, 1, 1] = NAN
    return z, n


def build_flat(specs, extra):
    """The flat scene: per cell the object (facet, coarse 0) and the object of the other blockers (`extra[c]`: more triangles of cell c),
    then the two degenerate objects."""
    objs = []
    for c, (kind, a, b, nrm) in enumerate(specs):
        f = facet_points(c, a, b)
        coarse = coarse_blockers(c)
        fn = sf.face_normal(f.reshape(1, 12))[0]
        flat_n = lambda tris: np.repeat(sf.face_normal(tris.reshape(-1, 12)), 3, axis=0).reshape(-1, 9)
        first = np.stack([f, coarse[0]])
        n_first = np.concatenate([(np.tile(fn, (3, 1)) if nrm is None else nrm).reshape(1, 9), flat_n(coarse[:1])]).astype(np.float32)
        objs.append(dict(tris=first, leaves=(2,), shape="root_leaf", color=ts.COLORS[c % 5], material=ts.MATERIALS[c % 3], normals=n_first))
        rest = np.concatenate([coarse[1:]] + ([extra[c]] if c in extra else []))
        sizes = [min(LEAF, rest.shape[0] - k) for k in range(0, rest.shape[0], LEAF)]
        objs.append(dict(tris=rest, leaves=tuple(sizes), shape="root_leaf" if len(sizes) == 1 else "left_comb", color=ts.COLORS[(c + 2) % 5],
                         material=ts.MATERIALS[(c + 1) % 3], normals=np.nan_to_num(flat_n(rest)).astype(np.float32)))
    for tri in degenerate_tris(len(specs)):
        objs.append(dict(tris=tri, leaves=(1,), shape="root_leaf", color=ts.COLORS[0], material=ts.MATERIALS[0], normals=np.tile(F32([0, 0, 1]), (1, 3))))
    return ts.flat_scene(objs)


def tri_ids(flat, tris):
    """The ids of `tris` (m x 3 x 4) in the flat scene, by their bits."""
    key = {p.tobytes(): i for i, p in enumerate(np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 12))}
    return np.int32([key[np.ascontiguousarray(t, np.float32).reshape(12).tobytes()] for t in tris])


# ---- the frame's pieces, for looking at a row -------------------------------------------------------------------------------------------
def dot_k(d, N):
    """The definition's k, float32."""
    d, N = np.ascontiguousarray(d, np.float32).reshape(-1, 3), np.ascontiguousarray(N, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2]


def b_of(Nf):
    """(b, x * y in float64) of the definition for facing normals Nf."""
    Nf = np.ascontiguousarray(Nf, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = np.copysign(F32(1.0), Nf[:, 2]).astype(np.float32)
        a = F32(-1.0) / (s + Nf[:, 2])
        return ((Nf[:, 0] * Nf[:, 1]) * a).astype(np.float32), Nf[:, 0].astype(F64) * Nf[:, 1].astype(F64)


TINY = float(np.finfo(np.float32).tiny)


def classify(Nf):
    """The class of every row by its facing normal (indices into CLASSES)."""
    Nf = np.ascontiguousarray(Nf, np.float32).reshape(-1, 3)
    x, y, z = Nf[:, 0], Nf[:, 1], Nf[:, 2]
    b, xy = b_of(Nf)
    with np.errstate(invalid="ignore"):
        near = (np.abs(z) >= F32(1.0 - 2.0 ** -15)) & ((x != 0) | (y != 0))
        conds = [(x == 0) & (y == 0) & (z == 1), (x == 0) & (y == 0) & (z == -1), (z == 0) & ~np.signbit(z), (z == 0) & np.signbit(z),
                 near & (b != 0) & (np.abs(b) < TINY), near & (b == 0) & (xy != 0), np.isnan(Nf).any(axis=1), near & (z > 0), near & (z < 0)]
    order = [0, 1, 2, 3, 6, 7, 8, 4, 5]
    return np.select(conds, order, default=CLASSES.index("general")).astype(np.int32)


# ---- bisections -------------------------------------------------------------------------------------------------------------------------
def to_ord(f):
    """float32 -> an integer that orders as the float does."""
    i = int(np.float32(f).view(np.int32))
    return i if i >= 0 else -(i & 0x7FFFFFFF)


def from_ord(i):
    return np.uint32(i if i >= 0 else ((-i) | 0x80000000)).view(np.float32)


def sweep_dirs(N, seed):
    """SWEEP directions d = (dx, dy, dz) against the normal N (N.x != 0): dx one ulp apart, the middle one the last whose k (the
    yardstick's arithmetic) is not positive."""
    rng = np.random.default_rng(seed)
    dy, dz = F32(rng.uniform(0.3, 1.0)), F32(-rng.uniform(0.3, 1.0))
    x0 = -(float(N[1]) * float(dy) + float(N[2]) * float(dz)) / float(N[0])
    pos = lambda i: bool(dot_k(F32([[from_ord(i), dy, dz]]), N)[0] > 0)
    lo, hi = to_ord(x0 - 0.5), to_ord(x0 + 0.5)
    if pos(lo):
        lo, hi = hi, lo
    assert not pos(lo) and pos(hi)
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if pos(mid):
            hi = mid
        else:
            lo = mid
    half = SWEEP // 2
    return np.stack([F32([from_ord(i), dy, dz]) for i in range(lo - half, lo + half + 1)])


def aim(oracle, P, w, seed):
    """One triangle per ray (P, w) (n x 3 float32 each), an edge of it within the lever's resolution of the ray: (tris n x 3 x 4, ok n)."""
    n = P.shape[0]
    rng = np.random.default_rng(seed)
    P64, w64 = P.astype(F64), w.astype(F64)
    u = w64 / np.linalg.norm(w64, axis=1, keepdims=True)
    h = np.where((np.abs(u[:, 0]) < 0.6)[:, None], F64([1.0, 0.0, 0.0]), F64([0.0, 1.0, 0.0]))
    p = np.cross(h, u); p /= np.linalg.norm(p, axis=1, keepdims=True)
    q = np.cross(u, p)
    ang = rng.uniform(0, 2 * np.pi, (n, 1))
    e1, e2 = p * np.cos(ang) + q * np.sin(ang), -p * np.sin(ang) + q * np.cos(ang)
    c = P64 + AIM_AT * w64
    rays = np.concatenate([P, w], axis=1).astype(np.float32)

    def tris(beta):
        t = np.ones((n, 3, 4), np.float32)
        t[:, 0, :3] = (c - 0.05 * e2).astype(np.float32)
        t[:, 1, :3] = (c + beta[:, None] * e1 + 3.0 * e2).astype(np.float32)
        t[:, 2, :3] = (c - 2.5 * e1 + 1.5 * e2).astype(np.float32)
        return t

    hits = lambda beta: oracle.ray_triangle(rays, tris(beta).reshape(n, 12)) != -np.inf
    lo, hi = np.full(n, -1.0), np.full(n, 1.0)
    ok = hits(hi) & ~hits(lo)
    for _ in range(64):
        mid = (lo + hi) / 2
        h_ = hits(mid)
        hi = np.where(h_, mid, hi); lo = np.where(h_, lo, mid)
    return tris(hi), ok & hits(hi)


def flush_tri(oracle, o, w, entry):
    """The triangle of the subnormal flush for the ray (o, w): FLUSH_AT along the ray's main axis (y for ODD_UP, x for ODD_RIGHT), an edge in
    the plane of o across the drift axis (x, y), the triangle on that side of the plane on which the ray as it stands misses it and the
    ray without its drift (on the edge: v = 0) hits."""
    travel, drift = (1, 0) if entry == ODD_UP else (0, 1)
    e = np.eye(3)
    base = o.astype(F64) + FLUSH_AT * np.sign(float(w[travel])) * e[travel]
    still = F32(w).copy(); still[drift] = 0.0
    for side in (-1.0, 1.0):
        t = np.ones((3, 4), np.float32)
        t[:, :3] = np.stack([base - 0.5 * e[2], base + 0.5 * e[2], base + 0.5 * side * e[drift]]).astype(np.float32)
        got = oracle.ray_triangle(np.stack([np.concatenate([o, w]), np.concatenate([o, still])]).astype(np.float32), np.tile(t.reshape(1, 12), (2, 1)))
        if got[0] == -np.inf and got[1] != -np.inf:
            break
    return t


# ---- everything, once -------------------------------------------------------------------------------------------------------------------
def _freeze(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _own_t(case, row, entry, tri):
    """The yardstick's t of triangle `tri` on the AO ray (row, entry) of a Case (row: index into case.sel)."""
    c = case.cand
    at = np.flatnonzero((c.ray == row * case.dirs.shape[0] + entry) & (c.tri == tri))
    return c.t[at[0]] if at.size else F32(-np.inf)


def blocked_without(case, pairs_row, pairs_entry, pairs_tri, t_min=T_MIN, t_max=T_MAX):
    """Per pair: (blocked, blocked with the pair's own triangle cut from the candidates), on the yardstick."""
    c, Kd = case.cand, case.dirs.shape[0]
    ray = np.asarray(pairs_row, np.int64) * Kd + np.asarray(pairs_entry, np.int64)
    own = dict(zip(ray.tolist(), np.asarray(pairs_tri, np.int64).tolist()))
    mine = np.fromiter((own.get(int(r), -1) == int(t) for r, t in zip(c.ray, c.tri)), bool, c.ray.size)
    tr = np.tile(F32([t_min, t_max]), (c.n_rays, 1))
    full = rr.occluded(c, case.flat, tr).astype(bool)
    cut = rr.occluded(rr.Candidates(c.n_rays, c.ray[~mine], c.tri[~mine], c.t[~mine]), case.flat, tr).astype(bool)
    return full[ray], cut[ray]


@functools.lru_cache(maxsize=None)
def build():
    from oracle import pyoracle as oracle
    specs = facet_specs()
    kinds = [s[0] for s in specs]
    rays, cell, side = main_rays(specs)
    coarse = build_flat(specs, {})
    facet_of = lambda flat: tri_ids(flat, np.stack([facet_points(c, s[1], s[2]) for c, s in enumerate(specs)]))
    fid = facet_of(coarse)

    # -- the sweeps and the flush rows need no blocker to exist: their rays are fixed here
    general = [c for c, k in enumerate(kinds) if k == "general"]
    pts = np.ascontiguousarray(coarse.tri_points, np.float32).reshape(-1, 3, 4)
    fnorm = sf.face_normal(pts[fid].reshape(-1, 12))
    swept = sorted(general, key=lambda c: -abs(float(fnorm[c][0])) * (1 - abs(float(fnorm[c][0]))))[:4]
    centroid = lambda c: pts[fid[c], :, :3].astype(F64).mean(0).astype(np.float32)
    h_rays, h_cell, h_kind, h_t = [], [], [], []

    def add(kind, c, o, d, t):
        h_rays.append(np.concatenate([F32(o), F32(d)])); h_cell.append(c); h_kind.append(kind); h_t.append(F32(t))

    for j, c in enumerate(swept):
        for d in sweep_dirs(fnorm[c], 300 + j):
            add("sweep", c, centroid(c), d, 0.0)
    flat_poles = [c for c, k in enumerate(kinds) if k in ("pole", "b_sub", "b_zero", "zero", "nan")]
    for c in flat_poles:
        for d in ((1, 0, 0), (1, 0, -0.0), (0, 1, 0), (-1, -1, -0.0)):
            add("k_zero", c, centroid(c), d, 0.0)
    for c in flat_poles[:2]:
        for d in ((INF, 0, -1), (0, -INF, 1)):
            add("k_nan", c, centroid(c), d, 0.0)
    flush_rows = []
    for c in [c for c, k in enumerate(kinds) if k == "b_sub"]:
        down = -float(specs[c][3][0][2])
        for off in ((0.125, 0.125, 0.0), (-0.125, 0.25, 1.25)):
            flush_rows.append(len(h_rays))
            add("flush", c, (cell_centre(c) + F64(off)).astype(np.float32), (0.0, 0.0, down), 0.0)
    n_fixed = len(h_rays)
    fixed = (np.stack(h_rays), fid[np.int32(h_cell)], F32(h_t))

    # -- the pairs to aim at: open bits among the coarse blockers, of the flat and the smooth frames and of the sweeps' ends
    extra, plan = {}, []                      # plan: (source, smooth, row, entry, class, triangle)
    sources = {("rays", False): ar.Case(oracle, coarse, rays, T16), ("rays", True): ar.Case(oracle, coarse, rays, T16, smooth=True),
               ("hits", False): ar.Case(oracle, coarse, fixed[0], T16, hits=fixed[1:])}
    for (src, smooth), case in sources.items():
        assert case.sel.size == case.rays.shape[0]
        open_ = ~case.blocked(t_max=T_MAX)
        finite = np.isfinite(case.ao_rays).all(axis=2)
        rows_, ents = [], []
        for r in range(case.sel.size):
            c = int(cell[r]) if src == "rays" else int(h_cell[r])
            if src == "hits":
                take = 4 if (h_kind[r] == "sweep" and r % SWEEP in (0, SWEEP - 1)) else 0
            elif smooth:
                take = 2 if kinds[c] in SMOOTH_KINDS else 3 if kinds[c] == "general" else 0
            else:
                take = 1 + (r % 2)
            free = np.flatnonzero(open_[r] & finite[r])
            for e in free[(np.arange(take) * 5 + r) % max(free.size, 1)][:free.size] if free.size else []:
                if (r, int(e)) not in zip(rows_, ents):
                    rows_.append(r); ents.append(int(e))
        rows_, ents = np.int64(rows_), np.int64(ents)
        tris, ok = aim(oracle, case.ao_rays[rows_, ents, 0:3], case.ao_rays[rows_, ents, 3:6], 40 + len(plan))
        cls = classify(case.Nf)
        for r, e, t, good in zip(rows_, ents, tris, ok):
            if good:
                c = int(cell[r]) if src == "rays" else int(h_cell[r])
                extra.setdefault(c, []).append(t)
                plan.append((src, smooth, int(r), int(e), int(cls[r]), t))
    # -- the flush triangles: the yardstick's own w for T_ODD's two horizon entries on the flush rows, smooth build
    fcase = ar.Case(oracle, coarse, fixed[0][flush_rows], T_ODD, smooth=True, hits=(fixed[1][flush_rows], fixed[2][flush_rows]))
    flush_plan = []
    for i, r in enumerate(flush_rows):
        for e in (ODD_UP, ODD_RIGHT):
            t = flush_tri(oracle, fixed[0][r, 0:3], fcase.ao_rays[i, e, 3:6], e)
            extra.setdefault(int(h_cell[r]), []).append(t)
            flush_plan.append((r, e, t))
    flat = build_flat(specs, {c: np.stack(v) for c, v in extra.items()})
    fid = facet_of(flat)
    assert flat.n_tris <= 4000
    zero_id, nan_id = tri_ids(flat, np.concatenate(degenerate_tris(len(specs))))

    # -- the rest of the hits batch: odd t on valid ids, the degenerate triangles
    main = ar.Case(oracle, flat, rays, T16)
    assert np.array_equal(main.hit, fid[cell]), "every main ray hits its own facet"
    nxt, t_nxt = rr.closest(rr.candidates(oracle, flat, rays), np.stack([rr.next_up(main.t), np.full(main.t.shape, INF)], axis=1))
    donors = [int(np.flatnonzero((cell == c) & (nxt >= 0))[0]) for c in
              (kinds.index("pole"), kinds.index("equator"), kinds.index("tilt") + 8, general[5], general[40], kinds.index("per_vertex"), kinds.index("b_sub"),
               kinds.index("nan"))]
    for r in donors:
        for t in ODD_T + (t_nxt[r],):
            add("odd_t", int(cell[r]), rays[r, 0:3], rays[r, 3:6], t)
    hid = list(fid[np.int32(h_cell)])
    for k, tid in enumerate((zero_id, nan_id)):
        o = (cell_centre(len(specs) + k) + F64([0.3, 0.2, 0.5])).astype(np.float32)
        for d, t in (((0, 0, -1), 0.5), ((0.1, 0.2, -1), 0.5), ((0, 0, 1), 0.0), ((1, 0, 0), 2.0)):
            add("degenerate", len(specs) + k, o, d, t); hid.append(tid)
    hits = types.SimpleNamespace(rays=np.ascontiguousarray(np.stack(h_rays), np.float32), hit_id=np.int32(hid), t=F32(h_t), kind=np.array(h_kind),
                                 cell=np.int32(h_cell), swept=tuple(swept), flush_rows=np.int64(flush_rows))
    assert (hits.hit_id >= 0).all() and (hits.hit_id < flat.n_tris).all() and np.array_equal(hits.hit_id[:n_fixed], fid[np.int32(h_cell[:n_fixed])])

    # -- which pairs the finished scene keeps
    finals = {("rays", False): main, ("rays", True): ar.Case(oracle, flat, rays, T16, smooth=True),
              ("hits", False): ar.Case(oracle, flat, hits.rays, T16, hits=(hits.hit_id, hits.t))}
    ids = tri_ids(flat, [p[5] for p in plan])
    keep = np.zeros(len(plan), bool)
    t_star = np.full(len(plan), -np.inf, np.float32)
    for key, case in finals.items():
        at = np.flatnonzero([(p[0], p[1]) == key for p in plan])
        assert np.array_equal(case.sel, np.arange(case.rays.shape[0]))
        full, cut = blocked_without(case, [plan[i][2] for i in at], [plan[i][3] for i in at], ids[at])
        keep[at] = full & ~cut
        for i in at[full & ~cut]:
            t_star[i] = _own_t(case, plan[i][2], plan[i][3], int(ids[i]))
    at = np.flatnonzero(keep)
    aimed_ = types.SimpleNamespace(source=np.array([plan[i][0] for i in at]), smooth=np.array([plan[i][1] for i in at], bool), row=np.int64([plan[i][2] for i in at]),
                                   entry=np.int64([plan[i][3] for i in at]), cls=np.int32([plan[i][4] for i in at]), tri=ids[at], t=t_star[at],
                                   planned=len(plan))
    fl = types.SimpleNamespace(row=np.int64([p[0] for p in flush_plan]), entry=np.int64([p[1] for p in flush_plan]), tri=tri_ids(flat, [p[2] for p in flush_plan]))
    out = types.SimpleNamespace(flat=flat, rays=rays, cell=cell, side=side, kinds=tuple(kinds), facet_id=fid, hits=hits, aimed=aimed_, flush=fl, cases=finals,
                                zero_id=int(zero_id), nan_id=int(nan_id))
    _freeze(flat.tri_points, flat.tri_normals, flat.node_min, flat.node_max, rays, cell, side, fid, *vars(hits).values(), *vars(aimed_).values(), *vars(fl).values())
    return out


def scene():
    return build().flat


def batch():
    """(rays n x 6, cell n, kind of the cell's facet n): the main batch."""
    g = build()
    return g.rays, g.cell, np.array(g.kinds)[g.cell]


def hits_batch():
    """The rows for srt_ao_hits only: a namespace of rays, hit_id, t, kind, cell, swept (the four swept cells), flush_rows."""
    return build().hits


def aimed():
    """The kept pairs: a namespace of source ("rays": the main batch through srt_ao_rays, "hits": the hits batch), smooth (the build whose
    frame the pair was aimed with), row, entry (of T16), cls (classify() of the row), tri (the pair's own blocker), t (the yardstick's t
    of that blocker on the pair's AO ray), planned (pairs before the ones another blocker interferes with were dropped)."""
    return build().aimed


def flush():
    """The pairs of the subnormal flush: row (of the hits batch), entry (of T_ODD), tri."""
    return build().flush


def case(source="rays", smooth=False):
    """The shared ao_ref.Case of the main batch ("rays") or the hits batch ("hits", flat build) at T16: computed once, never changed."""
    return build().cases[(source, smooth)]


def small_batch():
    """70 rows of the main batch across the kinds, for T33 and T1024."""
    g = build()
    return np.arange(g.rays.shape[0])[:: g.rays.shape[0] // 70][:70]


def interval_batch():
    """(rows of the main batch -- at most 128, each with a kept flat pair --, the chosen pair's index into aimed())."""
    a = aimed()
    mine = np.flatnonzero((a.source == "rays") & ~a.smooth)
    rows = np.unique(a.row[mine])[:128]
    chosen = int(mine[np.isin(a.row[mine], rows)][0])
    return rows, chosen


def intervals():
    """[(name, t_min, t_max)] of (e), around t* of the chosen pair."""
    a = aimed()
    t = F32(a.t[interval_batch()[1]])
    down, up = np.nextafter(t, F32(0.0)), np.nextafter(t, INF)
    return [("t_max = t*", T_MIN, t), ("t_max just below t*", T_MIN, down), ("t_min = t*", t, F32(T_MAX)), ("t_min just above t*", up, F32(T_MAX)),
            ("t_min > t_max", F32(12.0), F32(4.0)), ("(NaN, NaN)", NAN, NAN), ("(NaN, 16)", NAN, F32(T_MAX)), ("(1e-3, NaN)", T_MIN, NAN),
            ("(-inf, +inf)", -INF, INF), ("t_min = 0", F32(0.0), F32(T_MAX)), ("t_min = -1", F32(-1.0), F32(T_MAX))]
