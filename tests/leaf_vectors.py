"""Input families for the leaf functions (slab test, triangle test, barycentric coordinates, normal interpolation, triangle records)
beyond scene-scale inputs.  numpy only: the same arrays go to the oracle, to the live reference where it is built, and to the device
(tests/test_oracle_golden.py, tests/test_gpu_leaf.py, tests/golden/make_golden.make_leaf_kat).

Layouts as in tests/golden/kat.npz: ray = n x (origin xyz, direction xyz), box = n x (min xyz, max xyz), tri = n x 3 x xyzw flattened
to 12.  Coordinates are drawn as make_golden.make_kat draws them (boxes of 0..80 around (+-100, +-100, 300 +- 100), triangles of +-20
around (+-50, +-50, 300 +- 50)) and then multiplied by 2^e, e in SCALES: a power of two changes no quotient until a subnormal or an
overflow appears, so every scale asks the same question of the arithmetic until the format's ends are reached -- which is where the
families are meant to go.  The triangle test is NOT scale-free: its |det| < 1e-12 cut-off is absolute.

Every family is a Family record; `always` names the families whose answer is the same on every row, with the reason (any other family
must hold at least 5 % passes and 5 % misses, tests/test_oracle_golden.py checks both claims with the oracle).  Every array is finite
unless the family is marked `nonfinite`; rows that a scale would push out of the format are dropped, and finiteness is asserted.
"""
from dataclasses import dataclass, field

import numpy as np

SCALES = (-120, -100, -60, -20, 0, 20, 60, 100, 116)
ORDINARY_SCALES = (-60, -20, 0, 20, 60)          # where the "ordinary" ray / box families must show decided AND ambiguous rows
N = 2048
F32_MAX = np.float32(3.4028235e38)
SUBSAMPLE = 48                                    # rows of every family recorded in tests/golden/leaf_kat.npz


@dataclass
class Family:
    name: str
    kind: str                      # "box": ray + box; "tri": ray + tri
    ray: np.ndarray
    box: np.ndarray = None
    tri: np.ndarray = None
    always: str = ""               # "" or "pass: <reason>" / "miss: <reason>"
    ordinary: bool = False         # the filter must decide some rows and leave some ambiguous (box families)
    nonfinite: bool = False
    tags: dict = field(default_factory=dict)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def _scaled(a, e):
    with np.errstate(all="ignore"):
        return np.ldexp(f32(a), e).astype(np.float32)


def _finish(fam):
    """drop the rows a scale pushed out of the format; assert the rest is finite (unless the family says otherwise)"""
    arrs = [fam.ray, fam.box if fam.kind == "box" else fam.tri]
    if not fam.nonfinite:
        keep = np.isfinite(arrs[0]).all(1) & np.isfinite(arrs[1]).all(1)
        if fam.kind == "box" and fam.tags.get("empty"):
            keep[:] = True
        fam.ray = f32(arrs[0][keep])
        if fam.kind == "box":
            fam.box = f32(arrs[1][keep])
        else:
            fam.tri = f32(arrs[1][keep])
        for k, v in list(fam.tags.items()):
            if isinstance(v, np.ndarray) and v.shape[0] == keep.shape[0]:
                fam.tags[k] = v[keep]
        assert np.isfinite(fam.ray).all() and np.isfinite(fam.box if fam.kind == "box" else fam.tri).all(), fam.name
        assert fam.ray.shape[0] >= keep.shape[0] // 4, (fam.name, "a scale dropped most rows")
    return fam


# ---- ray / box ---------------------------------------------------------------------------------------------------------------
def _boxes(rng, n):
    lo = rng.uniform(-100, 100, (n, 3)).astype(np.float32); lo[:, 2] += 300
    hi = lo + rng.uniform(0, 80, (n, 3)).astype(np.float32)
    return lo, hi


def _aim(rng, lo, hi, sd=30.0):
    return (lo + hi) * np.float32(0.5) + rng.normal(0, sd, lo.shape).astype(np.float32)


def _graze(rng, ray, lo, hi, rows):
    """move the boxes of `rows` so that an edge (two axes) or a corner (three) of each lies on its ray, at t in [0.5, 2]: where two
    slab planes are crossed at once the filter's tnear and tfar meet"""
    m = len(rows)
    t = rng.uniform(0.5, 2.0, (m, 1)).astype(np.float32)
    P = ray[rows, :3] + ray[rows, 3:] * t
    size = hi[rows] - lo[rows]
    on = np.ones((m, 3), bool)
    edge = rng.integers(0, 2, m) == 1
    on[np.flatnonzero(edge), rng.integers(0, 3, int(edge.sum()))] = False
    side = rng.integers(0, 2, (m, 3)) == 1
    u = rng.uniform(0.1, 0.9, (m, 3)).astype(np.float32)
    nlo = np.where(on, np.where(side, P, P - size), P - size * u).astype(np.float32)
    lo[rows] = nlo; hi[rows] = nlo + size
    # a plane that is meant to lie on the ray does, bit for bit
    hi[rows] = np.where(on & ~side, P, hi[rows])


def _primary(rng, n):
    lo, hi = _boxes(rng, n)
    tgt = _aim(rng, lo, hi)
    ray = np.zeros((n, 6), np.float32)
    ray[:, 3] = np.rint(tgt[:, 0] * np.float32(400.0) / tgt[:, 2]); ray[:, 4] = np.rint(tgt[:, 1] * np.float32(400.0) / tgt[:, 2]); ray[:, 5] = 400.0
    k = n // 32
    ray[:k, 3] = 0.0; ray[k:2 * k, 4] = 0.0                       # the pixel column i = 0 and the pixel row j = 0 of every frame
    _graze(rng, ray, lo, hi, np.arange(2 * k, 2 * k + n // 8))
    return ray, np.concatenate([lo, hi], 1)


def _shadow(rng, n):
    """origin on a face, an edge or a corner of a box or inside it; even rows test that box (the ray's own: it passes), odd rows a
    neighbour 1..3 box sizes away, aimed at or past"""
    lo, hi = _boxes(rng, n)
    size = hi - lo
    sel = rng.integers(0, 3, (n, 3))
    o = np.where(sel == 0, lo, np.where(sel == 1, hi, lo + size * rng.uniform(0.05, 0.95, (n, 3)).astype(np.float32))).astype(np.float32)
    far = (10.0 ** rng.uniform(0, 4, (n, 1))).astype(np.float32)
    dirn = rng.normal(0, 1, (n, 3)); dirn /= np.linalg.norm(dirn, axis=1, keepdims=True)
    ray = np.zeros((n, 6), np.float32); ray[:, :3] = o
    tgt = o + (dirn * size.mean(1, keepdims=True) * far).astype(np.float32)
    odd = np.arange(n) % 2 == 1
    sh = size * rng.uniform(1, 3, (n, 3)).astype(np.float32) * rng.choice([-1.0, 0.0, 1.0], (n, 3)).astype(np.float32)
    sh[np.all(sh == 0, axis=1), 0] = 50.0
    lo2, hi2 = lo + sh.astype(np.float32), hi + sh.astype(np.float32)
    aim2 = _aim(rng, lo2, hi2, 25.0)
    tgt2 = o + (aim2 - o) * far
    ray[:, 3:] = np.where(odd[:, None], tgt2, tgt) - o
    lo = np.where(odd[:, None], lo2, lo); hi = np.where(odd[:, None], hi2, hi)
    return ray, np.concatenate([lo, hi], 1).astype(np.float32)


CAM_ORIGIN = np.array([37.5, -12.25, -80.0], np.float32)


def _cam_matrix():
    a, b, c = 0.3, -0.2, 0.1
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return (rz @ ry @ rx).astype(np.float32)        # columns = M[0], M[1], M[2] of srt_params.ray_matrix


def _camera(rng, n):
    """camera mode: one origin, direction = (M0 * dx + M1 * dy) + M2 * dz in float32 with integer (dx, dy) and dz = focal"""
    lo, hi = _boxes(rng, n)
    M = _cam_matrix()
    loc = (_aim(rng, lo, hi).astype(np.float64) - CAM_ORIGIN) @ M.astype(np.float64)        # M^T (target - o)
    dx = np.rint(loc[:, 0] * 400.0 / loc[:, 2]).astype(np.float32); dy = np.rint(loc[:, 1] * 400.0 / loc[:, 2]).astype(np.float32)
    dz = np.float32(400.0)
    ray = np.zeros((n, 6), np.float32); ray[:, :3] = CAM_ORIGIN
    for k in range(3):
        ray[:, 3 + k] = (M[k, 0] * dx + M[k, 1] * dy) + M[k, 2] * dz
    _graze(rng, ray, lo, hi, np.arange(n // 8))
    return ray, np.concatenate([lo, hi], 1)


def _corner(rng, n):
    """through a corner (even rows) or an edge (odd rows) of the box, +-3 ulp, from a non-zero origin"""
    lo, hi = _boxes(rng, n)
    o = rng.uniform(-80, 80, (n, 3)).astype(np.float32)
    corner = np.where(rng.integers(0, 2, (n, 3)) == 1, hi, lo)
    odd = np.flatnonzero(np.arange(n) % 2 == 1)
    ax = rng.integers(0, 3, len(odd))
    corner[odd, ax] = (lo + (hi - lo) * rng.uniform(0.1, 0.9, (n, 3)).astype(np.float32))[odd, ax]
    d = f32(corner - o)
    jig = rng.integers(-3, 4, (n, 3)).astype(np.int32)
    ray = np.zeros((n, 6), np.float32); ray[:, :3] = o
    ray[:, 3:] = (np.ascontiguousarray(d).view(np.int32) + jig).view(np.float32)
    return ray, np.concatenate([lo, hi], 1)


def _origins(rng, n):
    o = rng.uniform(-80, 80, (n, 3)).astype(np.float32)
    o[: n // 2] = 0.0
    return o


def _zero_dir(rng, n):
    """one, two or three direction components are +0 or -0; on such an axis the box's min, its max or both may equal the origin"""
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = f32(_aim(rng, lo, hi) - o)
    nz = rng.integers(1, 4, n)
    zero = np.zeros((n, 3), bool)
    for i in range(n):
        zero[i, rng.permutation(3)[: nz[i]]] = True
    d = np.where(zero, np.where(rng.integers(0, 2, (n, 3)) == 1, np.float32(-0.0), np.float32(0.0)), d).astype(np.float32)
    mode = rng.integers(0, 4, (n, 3))
    size = hi - lo
    # half the untouched zero axes get a box that straddles the origin's coordinate (else every row would be rejected on that axis)
    strad = zero & (mode == 0) & (rng.integers(0, 2, (n, 3)) == 1)
    lo = np.where(strad, o - size * np.float32(0.5), lo); hi = np.where(strad, o + size * np.float32(0.5), hi)
    lo = np.where(zero & ((mode == 1) | (mode == 3)), o, lo)
    hi = np.where(zero & (mode == 1), o + size, hi)
    hi = np.where(zero & ((mode == 2) | (mode == 3)), o, hi)
    lo = np.where(zero & (mode == 2), o - size, lo)
    ray = np.concatenate([o, d], 1)
    return f32(ray), f32(np.concatenate([lo, hi], 1))


def _hole1(rng, n):
    """d.x = +-0 and the box flat on x AT the origin's x: both x quotients are 0 * inf = NaN.  The reference's comparisons with them
    are all false and -- x being the FIRST axis of its chain, whose NaN then replaces the running interval -- nothing can reject."""
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = f32(_aim(rng, lo, hi, 60.0) - o)
    d[:, 0] = np.where(rng.integers(0, 2, n) == 1, np.float32(-0.0), np.float32(0.0))
    lo[:, 0] = o[:, 0]; hi[:, 0] = o[:, 0]
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


def _flat(rng, n):
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    nf = rng.integers(1, 4, n)
    for i in range(n):
        ax = rng.permutation(3)[: nf[i]]
        hi[i, ax] = lo[i, ax]
    d = f32(_aim(rng, lo, hi, 12.0) - o)
    exact = np.arange(n) % 4 == 0                        # aimed at the flat box's own centre, up to rounding
    d[exact] = f32((lo + hi) * np.float32(0.5) - o)[exact]
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


def _empty(rng, n):
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = f32(_aim(rng, lo, hi) - o)
    d[: n // 8, 0] = 0.0
    box = np.concatenate([np.full((n, 3), F32_MAX), np.full((n, 3), -F32_MAX)], 1)
    return f32(np.concatenate([o, d], 1)), f32(box)


def _behind(rng, n):
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = -f32(_aim(rng, lo, hi) - o)
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


def _special_dir(rng, n):
    """scale 0 only: one to three direction components are subnormal, +-inf or NaN"""
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = f32(_aim(rng, lo, hi) - o)
    pick = rng.integers(0, 3, (n, 3))
    sub = np.ldexp(rng.uniform(1, 2, (n, 3)), rng.integers(-149, -126, (n, 3))).astype(np.float32) * rng.choice([-1.0, 1.0], (n, 3)).astype(np.float32)
    inf = np.where(rng.integers(0, 2, (n, 3)) == 1, np.float32(np.inf), np.float32(-np.inf))
    val = np.where(pick == 0, sub, np.where(pick == 1, inf, np.float32(np.nan)))
    rep = rng.integers(0, 3, (n, 3)) == 0
    rep[np.arange(n), rng.integers(0, 3, n)] = True
    d = np.where(rep, val, d)
    # a share of the boxes holds the origin's coordinate on the special axes, so that such an axis does not decide every row
    size = hi - lo
    strad = rep & (rng.integers(0, 2, (n, 3)) == 1)
    lo = np.where(strad, o - size * np.float32(0.5), lo); hi = np.where(strad, o + size * np.float32(0.5), hi)
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


def _inf_box(rng, n):
    """scale 0 only: box coordinates that are +-inf"""
    lo, hi = _boxes(rng, n)
    o = _origins(rng, n)
    d = f32(_aim(rng, lo, hi) - o)
    mode = rng.integers(0, 6, (n, 3))
    mode[np.arange(n), rng.integers(0, 3, n)] = rng.integers(1, 6, n)
    inf = np.float32(np.inf)
    lo = np.where((mode == 1) | (mode == 3) | (mode == 5), -inf, lo); hi = np.where((mode == 2) | (mode == 3), inf, hi)
    lo = np.where(mode == 4, inf, lo); hi = np.where(mode == 4, inf, hi); hi = np.where(mode == 5, -inf, hi)
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


def _dir_sweep(rng, n):
    """coordinates near 1, direction components from 2^-149 to 2^127: the whole direction at one such exponent (even rows), one
    component at another exponent of its own on top (odd rows)"""
    lo = rng.uniform(-2, 2, (n, 3)).astype(np.float32)
    hi = lo + rng.uniform(0, 2, (n, 3)).astype(np.float32)
    o = rng.uniform(-1, 1, (n, 3)).astype(np.float32); o[: n // 2] = 0.0
    a = _aim(rng, lo, hi, 0.7).astype(np.float64) - o
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    kb = rng.integers(-149, 128, (n, 1))
    with np.errstate(all="ignore"):
        d = np.ldexp(a, kb).astype(np.float32)
        odd = np.flatnonzero(np.arange(n) % 2 == 1)
        ax = rng.integers(0, 3, len(odd))
        d[odd, ax] = np.ldexp(a[odd, ax], rng.integers(-149, 128, len(odd))).astype(np.float32)
    return f32(np.concatenate([o, d], 1)), f32(np.concatenate([lo, hi], 1))


_BOX = [  # (name, generator, scales, ordinary, always, nonfinite)
    ("primary", _primary, SCALES, True, "", False),
    ("shadow", _shadow, SCALES, True, "", False),
    ("camera", _camera, SCALES, True, "", False),
    ("corner", _corner, SCALES, True, "", False),
    ("zero_dir", _zero_dir, SCALES, False, "", False),
    ("hole1_x", _hole1, SCALES, False, "pass: both x quotients are NaN, and no comparison of the reference's chain with a NaN on its first axis rejects", False),
    ("flat", _flat, SCALES, False, "", False),
    ("empty", _empty, (0,), False, "pass: the intervals [-FLT_MAX / |d|, FLT_MAX / |d|] of an empty leaf's box all hold 0", False),
    ("behind", _behind, SCALES, False, "", False),
    ("special_dir", _special_dir, (0,), False, "", True),
    ("inf_box", _inf_box, (0,), False, "", True),
    ("dir_sweep", _dir_sweep, (0,), False, "", False),
]


def box_families(seed=1, n=N):
    out = []
    for fi, (name, gen, scales, ordinary, always, nonfinite) in enumerate(_BOX):
        for e in scales:
            rng = np.random.default_rng([seed, fi, e + 200])
            ray, box = gen(rng, n)
            fam = Family(f"{name}@2^{e}", "box", _scaled(ray, e), box=_scaled(box, e) if name != "empty" else box, always=always,
                         ordinary=ordinary and e in ORDINARY_SCALES, nonfinite=nonfinite, tags={"empty": name == "empty", "scale": e})
            out.append(_finish(fam))
    return out


def box_quotients(ray, box):
    """the six quotients of a row as the reference computes them (float32 divide), for failure messages"""
    with np.errstate(all="ignore"):
        o, d = f32(ray[:3]), f32(ray[3:])
        return np.concatenate([(f32(box[:3]) - o) / d, (f32(box[3:]) - o) / d])


def filter_emulated(ray, box, ulp=0, poison=True):
    """The filtered slab test in numpy, float32: rcp as the quotient 1 / d shifted by `ulp` units, fmin / fmax that drop a NaN, the
    margin of srt_device.h.  poison: ray_rcp's rule (NaN reciprocals for a ray with a zero, subnormal, > 2^126 or non-finite direction
    component).  Returns (pass, ambiguous).  An aid for choosing test inputs on a host without the device -- never a reference."""
    ray, box = f32(ray), f32(box)
    o, d = ray[:, :3], ray[:, 3:]
    with np.errstate(all="ignore"):
        rc = (np.float32(1.0) / d).astype(np.float32)
        if ulp:
            rc = np.where(np.isfinite(rc) & (rc != 0), (rc.view(np.int32) + np.int32(ulp)).view(np.float32), rc)
        if poison:
            a = np.abs(d)
            ok = np.all((a >= np.float32(2.0 ** -126)) & (a <= np.float32(2.0 ** 126)), axis=1)
            rc = np.where(ok[:, None], rc, np.float32(np.nan)).astype(np.float32)
        q0 = ((box[:, :3] - o) * rc).astype(np.float32); q1 = ((box[:, 3:] - o) * rc).astype(np.float32)
        tnear = np.fmax(np.fmax(np.fmin(q0[:, 0], q1[:, 0]), np.fmin(q0[:, 1], q1[:, 1])), np.fmin(q0[:, 2], q1[:, 2]))
        tfar = np.fmin(np.fmin(np.fmax(q0[:, 0], q1[:, 0]), np.fmax(q0[:, 1], q1[:, 1])), np.fmax(q0[:, 2], q1[:, 2]))
        m = (np.float32(2.0e-6) * (np.abs(tnear) + np.abs(tfar)).astype(np.float32) + np.float32(1.0e-37)).astype(np.float32)
        df = (tfar - tnear).astype(np.float32)
        return df > 0, ~(np.abs(df) > m)


# ---- ray / triangle ----------------------------------------------------------------------------------------------------------
def _kat_rt(rng, n=1536):
    """the rows make_golden.make_kat draws for rt_*: shadow-like rays, rays through a vertex and an edge midpoint, degenerate
    triangles, w != 1, rays pointing away, zero direction components, the origin on a vertex, overflowing coordinates"""
    tri = np.ones((n, 3, 4), np.float32)
    c = rng.uniform(-50, 50, (n, 1, 3)).astype(np.float32); c[..., 2] += 300
    tri[..., :3] = c + rng.uniform(-20, 20, (n, 3, 3)).astype(np.float32)
    ray = np.zeros((n, 6), np.float32)
    tgt = (tri[:, :, :3] * rng.dirichlet([1, 1, 1], n).astype(np.float32)[:, :, None]).sum(1)
    ray[:, 3:] = tgt + rng.normal(0, 6, (n, 3)).astype(np.float32)
    k = n // 6
    ray[:k, :3] = rng.uniform(-30, 30, (k, 3)).astype(np.float32); ray[:k, 3:] = tgt[:k] - ray[:k, :3]
    ray[k:2 * k, 3:] = tri[k:2 * k, 0, :3]
    ray[2 * k:3 * k, 3:] = (tri[2 * k:3 * k, 0, :3] + tri[2 * k:3 * k, 1, :3]) * np.float32(0.5)
    tri[3 * k:3 * k + 32, 2] = tri[3 * k:3 * k + 32, 1]
    tri[3 * k + 32:3 * k + 64, :, 3] = rng.uniform(0.5, 2.0, (32, 3)).astype(np.float32)
    ray[3 * k + 64:3 * k + 96, 3:] *= -1
    ray[3 * k + 96:3 * k + 128, 3] = 0.0
    ray[3 * k + 128:3 * k + 160, 3:5] = 0.0
    ray[3 * k + 160:3 * k + 164, 3:] = 0.0
    ray[3 * k + 164:3 * k + 196, :3] = tri[3 * k + 164:3 * k + 196, 0, :3]
    sel = slice(3 * k + 196, 3 * k + 212)
    tri[sel, :, :3] *= np.float32(1e25); ray[sel, 3:] *= np.float32(1e20)
    return ray, tri.reshape(n, 12)


def _kat_rt2(rng, n=1024):
    """make_kat's rt2_*: integer pixel rays against scene-scale triangles"""
    ray = np.zeros((n, 6), np.float32)
    ray[:, 3] = rng.integers(-960, 960, n); ray[:, 4] = rng.integers(-540, 540, n); ray[:, 5] = 400.0
    tri = np.ones((n, 3, 4), np.float32)
    tt = rng.uniform(0.5, 3.0, (n, 1, 1)).astype(np.float32)
    tri[..., :3] = ray[:, None, 3:] * tt + rng.uniform(-40, 40, (n, 3, 3)).astype(np.float32)
    return ray, tri.reshape(n, 12)


def _tri_aimed(rng, n, sd=6.0):
    tri = np.ones((n, 3, 4), np.float32)
    c = rng.uniform(-50, 50, (n, 1, 3)).astype(np.float32); c[..., 2] += 300
    tri[..., :3] = c + rng.uniform(-20, 20, (n, 3, 3)).astype(np.float32)
    o = np.zeros((n, 3), np.float32); o[n // 2:] = rng.uniform(-30, 30, (n - n // 2, 3)).astype(np.float32)
    tgt = (tri[:, :, :3] * rng.dirichlet([1, 1, 1], n).astype(np.float32)[:, :, None]).sum(1)
    d = f32(tgt + rng.normal(0, sd, (n, 3)).astype(np.float32) - o)
    return np.concatenate([o, d], 1).astype(np.float32), tri


def _with_w(ray, tri, w):
    tri = tri.copy()
    tri[..., :3] = tri[..., :3] * w[..., None]        # the projected point p / w is the drawn one up to the divide's rounding
    tri[..., 3] = w
    return ray, tri.reshape(-1, 12)


def _w_pos(rng, n=1024):
    ray, tri = _tri_aimed(rng, n)
    return _with_w(ray, tri, rng.uniform(0.25, 4.0, (n, 3)).astype(np.float32))


def _w_neg(rng, n=1024):
    ray, tri = _tri_aimed(rng, n)
    return _with_w(ray, tri, -rng.uniform(0.25, 4.0, (n, 3)).astype(np.float32))


def _w_extreme(rng, n=1024):
    ray, tri = _tri_aimed(rng, n)
    w = np.ones((n, 3), np.float32)
    big = np.where(rng.integers(0, 2, n) == 1, 1e30, 1e-30) * rng.uniform(0.5, 2.0, n)
    w[np.arange(n), rng.integers(0, 3, n)] = big.astype(np.float32)
    return _with_w(ray, tri, w)


def _degenerate(rng, n=1024):
    """zero area (two equal vertices; three collinear ones) and slivers (the third vertex 1e-6 .. 1e-3 of an edge off that edge)"""
    ray, tri = _tri_aimed(rng, n, 0.5)
    k = n // 4
    tri[:k, 2] = tri[:k, 1]
    tri[k:2 * k, 2, :3] = tri[k:2 * k, 0, :3] + (tri[k:2 * k, 1, :3] - tri[k:2 * k, 0, :3]) * np.float32(2.0)
    e = tri[2 * k:, 1, :3] - tri[2 * k:, 0, :3]
    off = rng.normal(0, 1, e.shape).astype(np.float32) * (10.0 ** rng.uniform(-6, -1, (e.shape[0], 1))).astype(np.float32)
    tri[2 * k:, 2, :3] = tri[2 * k:, 0, :3] + e * rng.uniform(0.2, 1.5, (e.shape[0], 1)).astype(np.float32) + off * np.float32(20.0)
    # aim the sliver rows at their own (thin) triangle again
    tgt = (tri[2 * k:, :, :3] * rng.dirichlet([1, 1, 1], n - 2 * k).astype(np.float32)[:, :, None]).sum(1)
    ray[2 * k:, 3:] = f32(tgt - ray[2 * k:, :3])
    return ray, tri.reshape(n, 12)


def _origin_on(rng, n=1024):
    """the ray's origin on a vertex (even rows) or on an edge (odd rows) of the triangle"""
    ray, tri = _tri_aimed(rng, n)
    v = tri[np.arange(n), rng.integers(0, 3, n), :3]
    mid = (tri[:, 0, :3] + tri[:, 1, :3]) * np.float32(0.5)
    odd = (np.arange(n) % 2 == 1)[:, None]
    ray[:, :3] = np.where(odd, mid, v)
    ray[:, 3:] = rng.normal(0, 1, (n, 3)).astype(np.float32) * np.float32(30.0)
    return ray, tri.reshape(n, 12)


_TRI = [("kat_rt", _kat_rt, SCALES), ("kat_rt2", _kat_rt2, SCALES), ("w_pos", _w_pos, SCALES), ("w_neg", _w_neg, SCALES),
        ("w_extreme", _w_extreme, (-20, 0, 10)), ("degenerate", _degenerate, SCALES), ("origin_on", _origin_on, SCALES)]


def _tri_always(name, e):
    """|det| < 1e-12 is an absolute cut-off and det is cubic in the scale (edge x edge x direction, ~1e5 at scale 0; make_kat's pixel
    rays against nearer triangles, kat_rt2, ~1e7): at 2^-20 it decides most rows, below every row.  From 2^60 on the cross and dot
    products overflow, det is infinite or NaN and 1 / det is 0 or NaN.  For a triangle family "miss" means: no row returns a positive
    distance -- t is -inf, NaN, or the 0 that 0 * (1 / inf) leaves for a ray that starts on the triangle."""
    if e <= -60 or (e == -20 and name != "kat_rt2"):
        return "miss: every |det| is below the absolute cut-off 1e-12 at this scale"
    if e >= 60:
        return "miss: the cross and dot products overflow; t is NaN, -inf or 0 * (1 / inf)"
    return ""


def tri_families(seed=1):
    out = []
    for fi, (name, gen, scales) in enumerate(_TRI):
        for e in scales:
            rng = np.random.default_rng([seed, 100 + fi, e + 200])
            ray, tri = gen(rng)
            if name == "kat_rt" and e < 0:        # make_kat's sixteen rows of 1e25-sized triangles are ordinary triangles again at a
                big = np.abs(tri).max(1) > 1e20   # negative scale, and hits: left out, so that what the family is named stays true
                ray, tri = ray[~big], tri[~big]
            tri = f32(tri).reshape(-1, 3, 4).copy()
            with np.errstate(all="ignore"):
                tri[..., :3] = np.ldexp(tri[..., :3], e)
            fam = Family(f"{name}@2^{e}", "tri", _scaled(ray, e), tri=tri.reshape(-1, 12), always=_tri_always(name, e), tags={"scale": e})
            out.append(_finish(fam))
    return out


def origin0_rows(fams):
    """The rows of the triangle families as rays FROM THE ORIGIN, for the origin form of the test: a row whose origin is 0 as it is;
    any other with its origin set to 0 and, where every w is 1, the triangle moved by -origin so that the ray still meets it.
    Returns (dir n x 3, tri n x 12, name of each row's family)."""
    dirs, tris, names = [], [], []
    for f in fams:
        ray, tri = f.ray.copy(), f.tri.reshape(-1, 3, 4).copy()
        w1 = np.all(tri[..., 3] == 1.0, axis=1)
        with np.errstate(all="ignore"):
            moved = tri[..., :3] - ray[:, None, :3]
        ok = w1 & np.isfinite(moved).all((1, 2))
        tri[ok, :, :3] = moved[ok]
        dirs.append(ray[:, 3:]); tris.append(tri.reshape(-1, 12)); names += [f.name] * ray.shape[0]
    return f32(np.concatenate(dirs)), f32(np.concatenate(tris)), np.array(names)


def bary_inputs(fams):
    """calculateBarycentricCoords inputs (kat.npz bc_in layout) from the triangle families: the triangle and the point origin + direction"""
    rows = []
    for f in fams:
        with np.errstate(all="ignore"):
            rows.append(np.concatenate([f.tri, f.ray[:, :3] + f.ray[:, 3:]], 1))
    return f32(np.concatenate(rows))


def interp_inputs(fams, seed=5):
    """interpolateNormal inputs (kat.npz in_in layout): the vertices' xyz as the three normals (so that the scales reach the 1 / sqrt),
    Dirichlet weights"""
    rng = np.random.default_rng(seed)
    rows = []
    for f in fams:
        n = f.tri.shape[0]
        rows.append(np.concatenate([f.tri.reshape(n, 3, 4)[..., :3].reshape(n, 9), rng.dirichlet([1, 1, 1], n).astype(np.float32)], 1))
    return f32(np.concatenate(rows))


# ---- triangle records (points only) ------------------------------------------------------------------------------------------
def record_points(seed=1):
    """Triangles for derive_triangle: every triangle family at scales where the points are of ordinary size or w != 1 matters, plus
    triangles whose raw-xyz cross product overflows (normal inf / NaN) or underflows to 0 (1 / sqrt(0) = inf, 0 * inf = NaN) and
    subnormal coordinates.  Returns (points n x 3 x 4, w_is_one n)."""
    keep = [f.tri for f in tri_families(seed) if f.tags["scale"] in (-100, -20, 0, 20, 60)]
    rng = np.random.default_rng([seed, 999])
    _, base = _tri_aimed(rng, 512)
    extra = []
    for s in (1e25, 1e17, 1e-17, 1e-25, 1e-38, 1e-43):
        t = base.copy()
        with np.errstate(all="ignore"):
            t[..., :3] = (t[..., :3] * np.float32(s)).astype(np.float32)
        extra.append(t.reshape(-1, 12))
    pts = f32(np.concatenate(keep + extra)).reshape(-1, 3, 4)
    assert np.isfinite(pts).all()
    return pts, np.all(pts[..., 3] == 1.0, axis=1)


def subsample(n):
    """the fixed rows of a family of n rows that tests/golden/leaf_kat.npz records"""
    return np.unique(np.linspace(0, n - 1, min(n, SUBSAMPLE)).astype(np.int64))


def recorded_rows(fams):
    """(ray, box-or-tri, family name per row, row index inside its family) of the subsample of every family, concatenated"""
    rays, seconds, names, rows = [], [], [], []
    for f in fams:
        idx = subsample(f.ray.shape[0])
        rays.append(f.ray[idx]); seconds.append((f.box if f.kind == "box" else f.tri)[idx])
        names += [f.name] * len(idx); rows.append(idx)
    return f32(np.concatenate(rays)), f32(np.concatenate(seconds)), np.array(names), np.concatenate(rows)
