"""Scenes built to hit the tie-breaks and the degenerate arithmetic, and ray batches aimed at what they contain -- the inputs of
tests/test_gpu_parity.py::test_adversarial_scenes_match_oracle (the scenes), tests/test_adversarial_ref.py (CPU: the batches reach the
cases) and tests/test_gpu_adversarial_queries.py (the ray-query family on them).  Plain numpy and the host mirror's scene builder.

scene(seed), seed 1, 2, 3: six objects of random triangles at scale 1, 1e-3 and 3e5; in every object up to three axis-aligned quads whose
diagonal belongs to two triangles (flat boxes), a triangle whose plane y = 0 passes through the origin, a sliver; the first half of
object 1's triangles again in objects 3 and 4 (equal t across objects: the lowest id wins).  scene(4) is scene(1) with vertex normals.
rays(seed): at most 600 rays in classes (A .. H below), each tagged with its class.  Everything is built once and read-only."""
import dataclasses
import functools

import numpy as np

import ray_query_ref as rq
import surface_ref as sf

SEEDS = (1, 2, 3, 4)
SCALES = (1.0, 1e-3, 3e5)
W, H, FOCAL = 161, 121, 400.0
A, B, C, D, E, F, G, NONFINITE = range(8)
CLASS_NAMES = ("frame sub-grid", "unrelated", "quad diagonals and corners", "duplicated centroids", "origins on a triangle", "in-plane", "slivers", "non-finite")
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def with_vertex_normals(flat):
    """The scene with vertex normals (it has none): at every vertex the normalised sum of the face normals of the triangles that share
    its position."""
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 3, 4)[..., :3].reshape(-1, 3)
    fn = np.nan_to_num(sf.face_normal(np.asarray(flat.tri_points, np.float32).reshape(-1, 12)).astype(np.float64))
    _, inv = np.unique(pts, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    acc = np.zeros((int(inv.max()) + 1, 3), np.float64)
    np.add.at(acc, inv, np.repeat(fn, 3, axis=0))
    length = np.linalg.norm(acc, axis=1, keepdims=True)
    vn = np.where(length > 0, acc / np.maximum(length, 1e-30), np.float64([0.0, 0.0, 1.0]))
    return dataclasses.replace(flat, tri_normals=np.ascontiguousarray(vn[inv].reshape(-1, 9), np.float32))


def scale_of(seed):
    return SCALES[(1 if seed == 4 else seed) - 1]


@functools.lru_cache(maxsize=None)
def generate(seed):
    """(flat, light, what the generator put in): quads -- (object, x0, x1, y0, y1, z) --, the plane triangles and the slivers as 3 x 3
    points per object that has them."""
    from simple_raytracer_amd import build, host
    import scenes
    build.build_host()
    rng = np.random.default_rng(seed)
    scale = [1.0, 1e-3, 3e5][seed - 1]
    n_obj = 6
    recipe = scenes.Recipe(); meshes = {}
    shared = None
    quads, planes, slivers = [], [], []
    for k in range(n_obj):
        n = int(rng.integers(1, 90))
        c = rng.uniform(-120, 120, (n, 1, 3)); c[..., 2] += 320
        pts = np.ones((n, 3, 4), np.float32)
        pts[..., :3] = (c + rng.uniform(-60, 60, (n, 3, 3))) * scale
        # axis-aligned quads at integer-friendly depths: flat boxes and exact ties between their two triangles' edges
        m = min(n, 6)
        for q in range(0, m - 1, 2):
            z = float(rng.integers(200, 400)) * scale; x0, x1 = sorted(rng.integers(-100, 100, 2) * scale); y0, y1 = sorted(rng.integers(-80, 80, 2) * scale)
            pts[q, :, :3] = [[x0, y0, z], [x1, y0, z], [x1, y1, z]]
            pts[q + 1, :, :3] = [[x0, y0, z], [x1, y1, z], [x0, y1, z]]
            quads.append((k,) + tuple(float(v) for v in pts[q, (0, 2), :2].T.reshape(-1)) + (float(pts[q, 0, 2]),))
        if n > 8:
            pts[7, :, :3] = [[-50 * scale, 0, 100 * scale], [50 * scale, 0, 100 * scale], [0, 0, 900 * scale]]     # plane through the origin
            pts[8, 2, :3] = pts[8, 0, :3] + (pts[8, 1, :3] - pts[8, 0, :3]) * np.float32(1 + 1e-6)                # sliver
            planes.append(pts[7, :, :3].copy()); slivers.append(pts[8, :, :3].copy())
        if k == 1:
            shared = pts[: max(1, n // 2)].copy()
        if k in (3, 4) and shared is not None:
            pts = np.concatenate([pts, shared])          # the same triangles again in other objects: equal t across objects
        meshes[f"m{k}"] = pts
        recipe.load(f"obj{k}", f"m{k}"); recipe.color(f"obj{k}", rng.uniform(0, 1, 3)); recipe.bvh(f"obj{k}")
    recipe.light = tuple(float(x) for x in rng.uniform(-400, 400, 3) * scale)
    flat = host.build_flat_scene(recipe, meshes)
    return flat, recipe.light, dict(quads=quads, planes=planes, slivers=slivers)


@functools.lru_cache(maxsize=None)
def scene(seed):
    """(flat, light) of a seed; seed 4: seed 1's with vertex normals."""
    flat, light, _ = generate(1 if seed == 4 else seed)
    return (with_vertex_normals(flat) if seed == 4 else flat), light


def points_of(flat):
    return np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)[..., :3]


@functools.lru_cache(maxsize=None)
def duplicates(seed):
    """The triangles that occur in more than one object: (groups -- lists of ids with the same nine coordinates, ascending --, is_dup per
    triangle, lowest -- per triangle the lowest id of its group, itself when alone)."""
    flat = scene(seed)[0]
    P = points_of(flat).reshape(flat.n_tris, 9)
    _, inv = np.unique(P.view(np.uint32), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    groups = [np.flatnonzero(inv == g) for g in np.unique(inv)]
    groups = [g for g in groups if np.unique(flat.tri_obj[g]).size > 1]
    is_dup = np.zeros(flat.n_tris, bool)
    lowest = np.arange(flat.n_tris)
    for g in groups:
        is_dup[g] = True; lowest[g] = g.min()
    return groups, is_dup, lowest


def towards(points, origins, stretch=1.0):
    """Rays from `origins` at `points`: d = (point - origin) * stretch in float32, +0 only."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = ((np.asarray(points, np.float32).reshape(-1, 3) - o) * np.float32(stretch)).astype(np.float32)
    return np.concatenate([o, np.where(d == 0, np.float32(0.0), d)], axis=1).astype(np.float32)


def along(points, direction, back):
    """Rays at `points` along `direction` from `back` lengths of it behind them."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    d = np.broadcast_to(np.asarray(direction, np.float32), p.shape)
    return np.concatenate([(p - d * np.float32(back)).astype(np.float32), np.where(d == 0, np.float32(0.0), d)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def rays(seed):
    """(rays n x 6, class n) of a seed (seed 4: seed 1's)."""
    if seed == 4:
        return rays(1)
    flat, _, made = generate(seed)
    s = np.float32(scale_of(seed))
    rng = np.random.default_rng(1000 + seed)
    P = points_of(flat)
    groups, _, _ = duplicates(seed)
    out = []
    # A: a sub-grid of the 161 x 121 frame, with the column dx = 0 and the row dy = 0
    frame = rq.frame_rays(W, H, np.eye(4, dtype=np.float32).reshape(16), FOCAL).reshape(H, W, 6)
    out.append((A, frame[0:H:30, 0:W:20].reshape(-1, 6)))                    # 5 rows x 9 columns: few enough for the hit share of A and B to stay below 0.8
    assert (out[-1][1][:, 3] == 0).any() and (out[-1][1][:, 4] == 0).any()
    # B: rays that share nothing
    out.append((B, rq.unrelated_rays(flat, 150)))
    # C: the shared diagonal (its middle) and the two shared corners of every quad, from outside: along +z, and from the origin
    pts = np.float32([[((x0 + x1) / 2, (y0 + y1) / 2, z), (x0, y0, z), (x1, y1, z)] for _, x0, x1, y0, y1, z in made["quads"]]).reshape(-1, 3)
    out.append((C, np.concatenate([along(pts, [0.0, 0.0, float(s)], 150.0), towards(pts, np.zeros_like(pts), 0.5)])))
    # D: the centroid of a duplicated triangle, from a point off its plane
    ids = np.array([g[0] for g in groups], np.int64)[:40]
    cen = P[ids].astype(np.float64).mean(1)
    nrm = np.cross(P[ids, 1] - P[ids, 0], P[ids, 2] - P[ids, 0]).astype(np.float64)
    nrm = np.nan_to_num(nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300))
    off = (nrm * rng.uniform(3.0, 9.0, (ids.size, 1)) * np.where(rng.random((ids.size, 1)) < 0.5, -1.0, 1.0) + rng.uniform(-2.0, 2.0, (ids.size, 3))) * float(s)
    out.append((D, towards(cen, cen + off, 1.0)))
    # E: origins ON a triangle -- a vertex, an edge's middle, the centroid -- of duplicated and other triangles, looking anywhere
    pick = np.concatenate([ids[:4], rng.integers(0, flat.n_tris, 4)])
    on = np.concatenate([P[pick, 0], ((P[pick, 0] + P[pick, 1]) * np.float32(0.5)).astype(np.float32), P[pick].mean(1).astype(np.float32)])
    d = rng.standard_normal((on.shape[0], 3)).astype(np.float32)
    out.append((E, np.concatenate([on, d], axis=1).astype(np.float32)))
    # F: rays lying in the plane of a quad (d.z = 0 at z = the quad's) and in the plane y = 0 through the origin: det = 0
    q = made["quads"][:6]
    inq = np.float32([[x0 - 30 * float(s), (y0 + y1) / 2, z, float(s) * (1 + j), float(s) * 0.25 * j, 0.0] for j, (_, x0, x1, y0, y1, z) in enumerate(q)])
    iny = np.float32([[x * float(s), 0.0, 50 * float(s), dx * float(s), 0.0, float(s)] for x, dx in ((0.0, 0.0), (-20.0, 0.05), (30.0, -0.02), (0.0, 0.1), (60.0, 0.0), (-45.0, 0.04))])
    out.append((F, np.concatenate([inq, iny])))
    # G: the slivers -- at the centroid from the origin and along z, and along the long edge
    sl = np.float32(made["slivers"]).reshape(-1, 3, 3)
    cen = sl.mean(1).astype(np.float32)
    edge = towards(sl[:, 1], sl[:, 0] - (sl[:, 1] - sl[:, 0]), 1.0)
    out.append((G, np.concatenate([towards(cen, np.zeros_like(cen), 2.0), along(cen, [0.0, 0.0, float(s)], 90.0), edge])))
    # H: eight rays that are not finite, or go nowhere
    c0 = P[0].mean(0)
    h = np.float32([[NAN, 0, 0, 0, 0, 1], [INF, 0, 0, -1, 0, 0], [-INF, c0[1], c0[2], 1, 0, 0], [0, 0, 0, 0, 0, INF], [0, 0, 0, INF, INF, INF],
                    [0, 0, 0, 0, 0, 0], [c0[0], c0[1], c0[2], 0, 0, 0], [0, 0, 0, NAN, 0, 1]])
    out.append((NONFINITE, h))
    r = np.ascontiguousarray(np.concatenate([v for _, v in out]), np.float32)
    cls = np.concatenate([np.full(v.shape[0], k, np.int32) for k, v in out])
    r[:, 3:6] = np.where(r[:, 3:6] == 0, np.float32(0.0), r[:, 3:6])
    assert r.shape[0] <= 600 and not (np.signbit(r[:, 3:6]) & (r[:, 3:6] == 0)).any()
    r.setflags(write=False); cls.setflags(write=False)
    return r, cls


def finite(r):
    """The rays whose six numbers are finite and whose direction is not zero: those a 1 x 1 oracle frame stands for."""
    return np.isfinite(r).all(axis=1) & (r[:, 3:6] != 0).any(axis=1)


def lights(seed, n):
    from simple_raytracer_amd import abi
    return abi.light_staircase(np.float32(scene(seed)[1]), n)


# ---- what the tests share: computed once per seed, never changed ---------------------------------------------------------------------
DEPTH, N_LIGHTS, BOUNCE_T_MIN = 3, 3, 1e-3
REFLECTANCE = np.float32([0.6, 0.25, 0.4, 0.8, 0.35, 0.5])
GLASS = 1.5
_cands, _memo = {}, {}


def scene_key(seed):
    return 1 if seed == 4 else seed                      # seed 4 differs in its normals only: the walks are seed 1's


def candidates(oracle, seed):
    """ray_range_ref.candidates of rays(seed)."""
    import ray_range_ref as rr
    k = scene_key(seed)
    if k not in _cands:
        _cands[k] = rr.candidates(oracle, scene(k)[0], rays(k)[0])
        for a in (_cands[k].ray, _cands[k].tri, _cands[k].t):
            a.setflags(write=False)
    return _cands[k]


def memo(oracle, seed):
    """One visibility_ref.CandidateMemo per scene, shared by every path yardstick of it."""
    import visibility_ref as vr
    k = scene_key(seed)
    if k not in _memo:
        _memo[k] = vr.CandidateMemo(oracle, scene(k)[0])
    return _memo[k]


def nearest_ties(flat, c):
    """Per ray: (tied -- the closest hit's t bits (-0 keyed as +0) are shared by candidates of at least two objects --, the object of the
    winner, which holds the lowest id)."""
    import ray_range_ref as rr
    hit, t = rr.closest(c)
    with np.errstate(invalid="ignore"):
        ok = (c.t != -np.inf) & (c.t < np.inf)
    key = lambda a: (a + np.float32(0.0)).view(np.uint32)
    at_min = ok & (key(c.t) == key(t)[c.ray]) & (hit[c.ray] >= 0)
    pairs = np.unique(np.stack([c.ray[at_min], flat.tri_obj[c.tri[at_min]].astype(np.int64)], axis=1), axis=0)
    tied = np.bincount(pairs[:, 0], minlength=c.n_rays) >= 2
    return tied, np.where(hit >= 0, flat.tri_obj[np.maximum(hit, 0)], -1).astype(np.int32)


def lower_copy_objects(seed):
    """(the objects that hold the lowest-id copy of a triangle the generator repeated, the two objects it appended the copies to).  The flat
    scene lists the objects in reverse, so the lowest ids are in the LAST object the copies went to.  The triangle in the plane y = 0 is
    the same in every object that has one and is left out here."""
    flat = scene(seed)[0]
    P = points_of(flat)
    low = sorted({int(flat.tri_obj[g[0]]) for g in duplicates(scene_key(seed))[0] if not (P[g[0], :, 1] == 0).all()})
    return low, sorted(flat.names.index(n) for n in ("obj3", "obj4"))


def glass_ior(seed):
    """The two objects that carry the copies are glass, everything else mirrors."""
    ior = np.zeros(scene(seed)[0].n_objects, np.float32)
    ior[lower_copy_objects(seed)[1]] = GLASS
    return ior


def intervals(oracle, seed):
    """ray_range_ref.mixed_intervals over the batch -- second hits, just below the first hit, closed points, empty and random intervals, NaN
    bounds, dealt round robin -- with the closed point (t, t) on every other tied ray: (t_range n x 2, kind n)."""
    import ray_range_ref as rr
    c = candidates(oracle, seed)
    tr, kind, _ = rr.mixed_intervals(c, 50 + scene_key(seed))
    tied, _ = nearest_ties(scene(seed)[0], c)
    _, t = rr.closest(c)
    pick = np.flatnonzero(tied)[::2]
    tr, kind = tr.copy(), kind.copy()
    tr[pick, 0] = tr[pick, 1] = t[pick]; kind[pick] = 2
    return tr, kind
