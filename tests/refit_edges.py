"""Points a refit or a pose meets when a caller's simulation misbehaves, and what srt_scene_refit_device / srt_scene_pose must leave
for them (include/srt.h, REFIT and POSE): NaN of both kinds, +-inf, +-FLT_MAX, zeros of both signs, subnormals, w != 1.  Plain numpy.

  fold_exact / boxes_exact   the reference's box fold restated literally: sequential strict compares from (+FLT_MAX, -FLT_MAX), exact
                             to the bit -- a NaN never enters, the first of equal values stays (the sign of a zero included)
  derive_ref                 derive_triangle / derive_triangle_origin restated in numpy, one array statement per operation; float32
                             for the second opinion on the records, float64 for the yardstick of that opinion
  FAMILIES                   point families: (rng, flat, points) -> (points, tags); the tags say what was touched
  tree(name)                 the flat scenes the families are applied to
  MATRIX_KINDS / matrices    one matrix per object for srt_scene_pose; at least half of the objects keep an ordinary rigid turn

Used by tests/test_refit_edges_ref.py (CPU: the families hold what they claim, the oracle still sees a frame) and
tests/test_gpu_refit_edges.py (the device)."""
import dataclasses
import functools

import numpy as np

import gpu_frames as gf
import leaf_vectors as lv
import pose_ref
import tree_shapes as ts

FLT_MAX = np.float32(3.4028234663852886e38)
BELOW_MAX = np.nextafter(FLT_MAX, np.float32(0.0))
TINY = np.float32(1.17549435e-38)                      # the smallest normal float32
QUIET_NAN, SIGNALLING_NAN, SIGN_BIT = 0x7FC00000, 0x7FA00000, 0x80000000
POSE_SUB_HEIGHT = 6                                    # srt_kernels.h: k_pose_boxes climbs to this height in LDS, k_pose_top above it


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def from_bits(u):
    return np.ascontiguousarray(u, np.uint32).view(np.float32)


# ---- the boxes ---------------------------------------------------------------------------------------------------------------------
def fold_exact(v):
    """The reference's fold over the rows of v (k x 3 float32), in order, from (+FLT_MAX, -FLT_MAX):
    `if (x < mn) mn = x; if (mx < x) mx = x;` per axis.  Values are moved, never computed: the result is exact to the bit."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 3)
    mn, mx = np.full(3, FLT_MAX, np.float32), np.full(3, -FLT_MAX, np.float32)
    with np.errstate(invalid="ignore"):
        for x in v:
            mn = np.where(x < mn, x, mn)
            mx = np.where(mx < x, x, mx)
    return mn, mx


def leaf_boxes(first, count, xyz):
    """fold_exact of every leaf at once: step s folds row s of every leaf that has one (rows = the leaf's triangles in visit order,
    points one, two, three).  The same sequence of compares per leaf, leaves side by side."""
    rows = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    first, n_rows = np.asarray(first, np.int64), 3 * np.asarray(count, np.int64)
    mn = np.full((first.size, 3), FLT_MAX, np.float32); mx = np.full((first.size, 3), -FLT_MAX, np.float32)
    with np.errstate(invalid="ignore"):
        for s in range(int(n_rows.max()) if n_rows.size else 0):
            sel = np.flatnonzero(n_rows > s)
            x = rows[3 * first[sel] + s]
            mn[sel] = np.where(x < mn[sel], x, mn[sel])
            mx[sel] = np.where(mx[sel] < x, x, mx[sel])
    return mn, mx


def combine(lmn, lmx, rmn, rmx):
    """combine(left, right): `r < l ? r : l` and `l < r ? r : l` -- the left operand stays on ties and against a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(rmn < lmn, rmn, lmn), np.where(lmx < rmx, rmx, lmx)


def boxes_exact(flat, points):
    """node_min / node_max (n_nodes x 3) of flat's trees over `points` (n_tris x 3 x 4): a leaf is fold_exact over its triangles, raw
    xyz; an inner node combine(left, right); an empty leaf keeps the start values.  Any node order."""
    xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3, 4)[..., :3]
    nN = flat.n_nodes
    mn = np.empty((nN, 3), np.float32); mx = np.empty((nN, 3), np.float32)
    leaf = np.flatnonzero(flat.node_left < 0)
    mn[leaf], mx[leaf] = leaf_boxes(flat.node_first[leaf], flat.node_count[leaf], xyz)
    done = np.zeros(nN, bool); done[leaf] = True
    for root in flat.obj_root:
        stack = [(int(root), False)]
        while stack:
            i, seen = stack.pop()
            if done[i]:
                continue
            l, r = int(flat.node_left[i]), int(flat.node_right[i])
            if not seen:
                stack.append((i, True)); stack.append((r, False)); stack.append((l, False))
            else:
                mn[i], mx[i] = combine(mn[l], mx[l], mn[r], mx[r])
                done[i] = True
    assert done.all()
    return mn, mx


def edge_flat(flat, points, normals=None):
    """The flat scene a refit with `points` (n_tris x 3 x 4) must leave: flat's order and trees, the points, boxes_exact, the normals."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3, 4)
    assert pts.shape[0] == flat.n_tris
    mn, mx = boxes_exact(flat, pts)
    kw = dict(tri_points=pts, node_min=mn, node_max=mx)
    if normals is not None:
        kw["tri_normals"] = np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
    return dataclasses.replace(flat, **kw)


def pose_flat(flat, mats):
    """What srt_scene_pose must leave: pose_ref.transform (bit-true) per object, then boxes_exact."""
    return edge_flat(flat, pose_ref.transform_objects(flat, mats))


def node_height(flat):
    """0 for a leaf, 1 + max(children) for an inner node."""
    h = np.zeros(flat.n_nodes, np.int64)
    for root in flat.obj_root:
        stack = [(int(root), False)]
        while stack:
            i, seen = stack.pop()
            l, r = int(flat.node_left[i]), int(flat.node_right[i])
            if l < 0:
                continue
            if not seen:
                stack.append((i, True)); stack.append((r, False)); stack.append((l, False))
            else:
                h[i] = 1 + max(h[l], h[r])
    return h


# ---- the records -------------------------------------------------------------------------------------------------------------------
def clamp_to_float32_range(v):
    """A float64 value where float32 would have overflowed or underflowed: +-inf from 2^128 - 2^103 on (where rounding to float32
    reaches inf), +-0 up to 2^-150 (where it reaches 0); every other value keeps its float64 precision."""
    a = np.abs(v)
    out = np.where(a >= 2.0 ** 128 - 2.0 ** 103, np.copysign(np.inf, v), v)
    return np.where(a <= 2.0 ** -150, np.copysign(0.0, v), out)


def derive_ref(points, dtype=np.float32, clamp=None, parts=False):
    """derive_triangle and derive_triangle_origin (csrc/srt_kernels.h) on points n x 3 x 4, every operation its own array statement in
    `dtype`, the header's association: the nine divides by w, edges of the divided points, the normal from raw xyz with
    (cx * cx + cy * cy) + cz * cz and 1.0f / sqrt.  Returns (tris n x 12, tris_o n x 12) in record order; with parts=True also every
    named intermediate.  clamp: applied to the result of every operation (the float64 yardstick clamped to float32's range)."""
    with np.errstate(invalid="ignore"):
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3, 4).astype(dtype)
    one, zero = dtype(1.0), dtype(0.0)
    c = clamp if clamp is not None else (lambda v: v)
    (x1, y1, z1, w1), (x2, y2, z2, w2), (x3, y3, z3, w3) = [[p[:, j, a] for a in range(4)] for j in range(3)]
    with np.errstate(all="ignore"):
        p1x = c(x1 / w1); p1y = c(y1 / w1); p1z = c(z1 / w1)
        p2x = c(x2 / w2); p2y = c(y2 / w2); p2z = c(z2 / w2)
        p3x = c(x3 / w3); p3y = c(y3 / w3); p3z = c(z3 / w3)
        e1x = c(p2x - p1x); e1y = c(p2y - p1y); e1z = c(p2z - p1z)
        e2x = c(p3x - p1x); e2y = c(p3y - p1y); e2z = c(p3z - p1z)
        ax = c(x2 - x1); ay = c(y2 - y1); az = c(z2 - z1)
        bx = c(x3 - x1); by = c(y3 - y1); bz = c(z3 - z1)
        m0 = c(ay * bz); m1 = c(by * az); cx = c(m0 - m1)
        m2 = c(az * bx); m3 = c(bz * ax); cy = c(m2 - m3)
        m4 = c(ax * by); m5 = c(bx * ay); cz = c(m4 - m5)
        q0 = c(cx * cx); q1 = c(cy * cy); q2 = c(cz * cz)
        s0 = c(q0 + q1); s1 = c(s0 + q2)
        root = c(np.sqrt(s1))
        s = c(one / root)
        nx = c(cx * s); ny = c(cy * s); nz = c(cz * s)
        tx = c(zero - p1x); ty = c(zero - p1y); tz = c(zero - p1z)
        r0 = c(ty * e1z); r1 = c(e1y * tz); qx = c(r0 - r1)
        r2 = c(tz * e1x); r3 = c(e1z * tx); qy = c(r2 - r3)
        r4 = c(tx * e1y); r5 = c(e1x * ty); qz = c(r4 - r5)
    named = dict(x1=x1, y1=y1, z1=z1, w1=w1, x2=x2, y2=y2, z2=z2, w2=w2, x3=x3, y3=y3, z3=z3, w3=w3,
                 p1x=p1x, p1y=p1y, p1z=p1z, p2x=p2x, p2y=p2y, p2z=p2z, p3x=p3x, p3y=p3y, p3z=p3z,
                 e1x=e1x, e1y=e1y, e1z=e1z, e2x=e2x, e2y=e2y, e2z=e2z, ax=ax, ay=ay, az=az, bx=bx, by=by, bz=bz,
                 m0=m0, m1=m1, m2=m2, m3=m3, m4=m4, m5=m5, cx=cx, cy=cy, cz=cz, q0=q0, q1=q1, q2=q2, s0=s0, s1=s1, root=root, s=s,
                 nx=nx, ny=ny, nz=nz, tx=tx, ty=ty, tz=tz, r0=r0, r1=r1, r2=r2, r3=r3, r4=r4, r5=r5, qx=qx, qy=qy, qz=qz)
    tris = np.stack([p1x, p1y, p1z, e1x, e1y, e1z, e2x, e2y, e2z, nx, ny, nz], 1)
    tris_o = np.stack([tx, ty, tz, e1x, e1y, e1z, e2x, e2y, e2z, qx, qy, qz], 1)
    assert tris.dtype == dtype and tris_o.dtype == dtype
    return (tris, tris_o, named) if parts else (tris, tris_o)


# every difference of derive_ref: (result, minuend, subtrahend) -- where a row cancels, float32 and float64 part ways
DIFFERENCES = [(f"e{j}{a}", f"p{j + 1}{a}", f"p1{a}") for j in (1, 2) for a in "xyz"] + \
              [(f"{n}{a}", f"{a}{j}", f"{a}1") for n, j in (("a", 2), ("b", 3)) for a in "xyz"] + \
              [("cx", "m0", "m1"), ("cy", "m2", "m3"), ("cz", "m4", "m5"), ("qx", "r0", "r1"), ("qy", "r2", "r3"), ("qz", "r4", "r5")]


# ---- the bar of the device tests -----------------------------------------------------------------------------------------------------
def same_records_bits(got, want, what="", derived=None):
    """DeviceScene.records() of a refitted or posed scene against those of a scene created from edge_flat: every word of the node, wide
    and root records as uint32 (the box floats too: -0 is not +0), no box float a NaN; texel coordinates, normals and texture ids as
    bits; both triangle records the same bits, or NaN on both sides (a computed NaN's sign and payload are not part of the contract).
    derived: derive_ref's (tris, tris_o), compared with the device's under the same rule."""
    for k in ("nodes", "wide", "root_nodes"):
        bad = (got[k] != want[k]).any(1)
        assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {bad.size} records differ as bits, first {int(np.flatnonzero(bad)[0])}: " \
                              f"{got[k][bad][0]} against {want[k][bad][0]}"
        assert not np.isnan(pose_ref.split_boxes(got, k)[0]).any(), f"{what}: {k}: a NaN in a box"
    assert np.array_equal(got["tri_tex"], want["tri_tex"]), f"{what}: tri_tex"
    for k in ("tri_texcoord", "tri_normals"):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k}"
    for k, ref in (("tris", None if derived is None else derived[0]), ("tris_o", None if derived is None else derived[1])):
        g = got[k].view(np.float32)
        for name, w in (("the created scene", want[k].view(np.float32)), ("derive_ref", ref)):
            if w is None:
                continue
            bad = ~gf.same_f32(g, w)
            assert not bad.any(), f"{what}: {k} against {name}: {int(bad.any(1).sum())} records differ, first triangle " \
                                  f"{int(np.flatnonzero(bad.any(1))[0])}: {g[bad][0]!r} against {w[bad][0]!r}"


# ---- the trees -----------------------------------------------------------------------------------------------------------------------
TREES = ("sliced", "roots33", "h6", "h7")
_SIZES = (31, 17, 9, 24, 0, 25, 8, 16, 1, 31)
_TALL = {"h6": (24, 6, 16), "h7": (40, 7, 24)}            # name: (leaves, height, seed of the random shape that has exactly that height)


def _shape_height(t):
    return 0 if not isinstance(t, tuple) else 1 + max(_shape_height(t[0]), _shape_height(t[1]))


def tall_objects(name):
    """One object of exactly the height the name says (a random shape, leaves of 0 .. 31 triangles) and two small ones: more than 256
    triangles and no multiple of 256, so a refit's last workgroup is partial and family rows fall on both sides of triangle 255 / 256."""
    n_leaves, height, seed = _TALL[name]
    assert _shape_height(ts.shape_tree("random", n_leaves, seed)) == height
    rng = np.random.default_rng(700 + height)
    leaves = [_SIZES[k % len(_SIZES)] for k in range(n_leaves)]
    centres = ts.grid_centres(rng, n_leaves, 170.0, 230.0)[rng.permutation(n_leaves)]
    main = np.concatenate([ts.patch(rng, s, centres[k], (12.0, 12.0, 15.0), 14.0) for k, s in enumerate(leaves)])
    comb_l, comb_c = (6, 13, 4), ts.grid_centres(rng, 3, 120.0, 140.0, fill=0.6) + np.float32([-20.0, 12.0, 0.0])
    comb = np.concatenate([ts.patch(rng, s, comb_c[k], (8.0, 8.0, 5.0), 10.0) for k, s in enumerate(comb_l)])
    one = ts.patch(rng, 11, (22.0, -14.0, 130.0), (6.0, 6.0, 5.0), 8.0)
    return [dict(tris=main, leaves=leaves, shape="random", seed=seed, color=ts.COLORS[0], material=ts.MATERIALS[0], normals=ts.away_normals(main)),
            dict(tris=comb, leaves=comb_l, shape="right_comb", color=ts.COLORS[1], material=ts.MATERIALS[1], normals=ts.away_normals(comb)),
            dict(tris=one, leaves=(11,), shape="root_leaf", color=ts.COLORS[2], material=ts.MATERIALS[2], normals=ts.away_normals(one))]


@functools.lru_cache(maxsize=None)
def tree(name):
    """sliced, roots33: tree_shapes' own.  h6: no node above the bottom subtrees (k_pose_top returns at once).  h7: one node above
    them, the root, whose children both are roots of bottom subtrees.  records: leaf_vectors.record_points() in four objects."""
    if name in ("sliced", "roots33", "roots5"):
        return ts.family(name)
    if name in _TALL:
        flat = ts.flat_scene(tall_objects(name))
        h = node_height(flat)
        assert h[flat.obj_root[0]] == _TALL[name][1] and flat.n_tris > 256 and flat.n_tris % 256 != 0
        assert (h > POSE_SUB_HEIGHT).sum() == (name == "h7")
        return flat
    if name == "records":
        pts, _ = lv.record_points()
        objs, cut = [], np.linspace(0, pts.shape[0], 5).astype(np.int64)
        for k in range(4):
            n = int(cut[k + 1] - cut[k])
            leaves, left, j = [], n, 0
            while left:
                s = min(left, ts.LEAF_SIZES[(j + k) % len(ts.LEAF_SIZES)]); leaves.append(s); left -= s; j += 1
            objs.append(dict(tris=pts[cut[k]:cut[k + 1]], leaves=leaves, shape=("random", "zigzag", "random", "left_comb")[k] if len(leaves) < 250 else "random",
                             seed=90 + k, color=ts.COLORS[k], material=ts.MATERIALS[k % 3]))
        with np.errstate(all="ignore"):
            return ts.flat_scene(objs)
    raise KeyError(name)


def nonempty_leaves(flat):
    return np.flatnonzero((flat.node_left < 0) & (flat.node_count > 0))


def leaf_rows(flat, i):
    """The triangles of leaf i, in visit order."""
    return np.arange(int(flat.node_first[i]), int(flat.node_first[i]) + int(flat.node_count[i]))


def first_leaf_below(flat, i):
    """The first leaf with triangles below node i in visit order (-1: none)."""
    stack = [int(i)]
    while stack:
        j = stack.pop()
        if flat.node_left[j] < 0:
            if flat.node_count[j] > 0:
                return j
        else:
            stack.append(int(flat.node_right[j])); stack.append(int(flat.node_left[j]))
    return -1


# ---- the point families --------------------------------------------------------------------------------------------------------------
def screen_area(pts):
    """The area every triangle covers on the screen, up to a factor (0 where it is not finite)."""
    with np.errstate(all="ignore"):
        s = pts[..., :2].astype(np.float64) / pts[..., 2:3]
        a, b = s[:, 1] - s[:, 0], s[:, 2] - s[:, 0]
        area = np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
    return np.where(np.isfinite(area), area, 0.0)


def _spread(rng, pts, m):
    """m triangles, scattered, the larger on the screen the likelier (the frame must show what a family does); triangles 255 and 256
    among them where the tree has them."""
    n = pts.shape[0]
    area = screen_area(pts) + 1e-9
    pick = rng.choice(n, size=min(m, n), replace=False, p=area / area.sum())
    if n > 257:
        pick[:2] = (255, 256)
        pick = np.unique(pick)
    return np.sort(pick)


def _nan_bits(rng, shape):
    """NaN bit patterns: quiet and signalling in turn, either sign."""
    k = np.arange(int(np.prod(shape))).reshape(shape)
    u = np.where(k % 2 == 0, QUIET_NAN, SIGNALLING_NAN).astype(np.uint32)
    return u | np.where(rng.integers(0, 2, shape) == 1, SIGN_BIT, 0).astype(np.uint32)


def nan_some(rng, flat, pts):
    """One coordinate of one vertex NaN in a tenth to a sixth of the triangles (the smaller the tree, the larger the share: the frame
    must show it): point one, two, three and axis x, y, z in turn, quiet and
    signalling in turn, the sign in turns of two."""
    p = pts.copy(); u = p.view(np.uint32)
    pick = _spread(rng, pts, max(26, p.shape[0] // 10))
    tag = dict(tri=pick, vertex=np.arange(pick.size) % 3, axis=(np.arange(pick.size) // 3) % 3,
               signalling=np.arange(pick.size) % 2 == 1, negative=(np.arange(pick.size) // 2) % 2 == 1)
    val = np.where(tag["signalling"], SIGNALLING_NAN, QUIET_NAN).astype(np.uint32) | np.where(tag["negative"], SIGN_BIT, 0).astype(np.uint32)
    u[pick, tag["vertex"], tag["axis"]] = val
    assert np.isnan(p[pick, tag["vertex"], tag["axis"]]).all() and np.array_equal(u[pick, tag["vertex"], tag["axis"]], val)
    return p, tag


def nan_leaf(rng, flat, pts):
    """Every xyz of every triangle of some leaves NaN (both kinds): a left child, a right child and a leaf of 31 triangles (where all
    nodes are roots: three leaves, one of 31)."""
    p = pts.copy(); u = p.view(np.uint32)
    full = nonempty_leaves(flat)
    inner = flat.node_left >= 0
    lefts, rights = np.intersect1d(full, flat.node_left[inner]), np.intersect1d(full, flat.node_right[inner])
    big = full[flat.node_count[full] == 31]
    assert big.size, "a leaf of 31 triangles"
    chosen = [int(big[0])]
    for cand in ((lefts, rights) if inner.any() else (full[::2], full[1::2])):
        cand = cand[~np.isin(cand, chosen)]
        cand = cand[flat.node_count[cand] >= 9] if (flat.node_count[cand] >= 9).any() else cand
        chosen.append(int(cand[np.argmax([screen_area(pts[leaf_rows(flat, i)]).sum() for i in cand])]))
    for i in chosen:
        r = leaf_rows(flat, i)
        u[r, :, :3] = _nan_bits(rng, (r.size, 3, 3))
    return p, dict(leaves=np.array(chosen), big=chosen[0], left=chosen[1], right=chosen[2], has_children=bool(inner.any()))


def nan_object(rng, flat, pts):
    """One whole object NaN (xyz, both kinds) in a scene of at least three; of many one-node objects the three largest on the screen
    (one of them alone changes too little of the frame)."""
    assert flat.n_objects >= 3
    area = np.bincount(flat.tri_obj, screen_area(pts), flat.n_objects)
    objs = np.array([1]) if flat.n_objects < 10 else np.sort(np.argsort(area)[-3:])
    p = pts.copy(); u = p.view(np.uint32)
    r = np.flatnonzero(np.isin(flat.tri_obj, objs))
    assert r.size
    u[r, :, :3] = _nan_bits(rng, (r.size, 3, 3))
    return p, dict(objs=objs, tri=r)


def inf(rng, flat, pts):
    """+inf and -inf: single coordinates (every point, every axis), whole triangles of either, and a leaf whose only finite triangle
    lies between an all-+inf one and all-(-inf) ones."""
    p = pts.copy()
    n = p.shape[0]
    leaves = nonempty_leaves(flat)
    leaves = leaves[(flat.node_count[leaves] >= 3) & (flat.node_count[leaves] <= 12)]
    i = int(leaves[rng.integers(0, leaves.size)])
    r = leaf_rows(flat, i)
    pick = np.setdiff1d(_spread(rng, pts, max(12, n // 12)), r)
    tag = dict(tri=pick, vertex=np.arange(pick.size) % 3, axis=(np.arange(pick.size) // 3) % 3, negative=np.arange(pick.size) % 2 == 1)
    p[pick, tag["vertex"], tag["axis"]] = np.where(tag["negative"], -np.inf, np.inf).astype(np.float32)
    whole = rng.choice(np.setdiff1d(np.arange(n), np.concatenate([pick, r])), size=4, replace=False)
    p[whole[:2], :, :3] = np.inf; p[whole[2:], :, :3] = -np.inf
    p[r[0], :, :3] = np.inf; p[r[2:], :, :3] = -np.inf
    tag.update(plus=whole[:2], minus=whole[2:], sandwich=i)
    return p, tag


def fltmax(rng, flat, pts):
    """Coordinates of +-FLT_MAX exactly (a tie with the fold's start) and of the float next to it."""
    p = pts.copy()
    pick = _spread(rng, pts, max(20, p.shape[0] // 10))
    vals = np.array([FLT_MAX, -FLT_MAX, BELOW_MAX, -BELOW_MAX], np.float32)
    tag = dict(tri=pick, vertex=np.arange(pick.size) % 3, axis=(np.arange(pick.size) // 3) % 3, value=np.arange(pick.size) % 4)
    p[pick, tag["vertex"], tag["axis"]] = vals[tag["value"]]
    return p, tag


def _zero_run(flat):
    """The leaves of the zeros family: whole objects (all of a scene of one-node objects' even ones), so that inner nodes tie too."""
    objs = np.arange(0, flat.n_objects, 2) if flat.n_objects >= 10 else np.arange(max(1, flat.n_objects - 1))
    return objs, np.flatnonzero(np.isin(flat.tri_obj, objs))


def zeros(rng, flat, pts):
    """On the leaves of some objects: every z is one of {+0, -0, positive} (z is positive as it stands: two to four of a leaf's z become
    zeros of random sign), every x one of {+0, -0, negative} (x becomes -|x| - 1, then zeros likewise).  Every such leaf's minimum in z
    and maximum in x is a zero whose sign is that of the FIRST zero in visit order; every inner node above them ties.  Below the root of
    the first object the first zeros are set by hand: left +0 beside right -0 in z, the reverse in x."""
    p = pts.copy(); u = p.view(np.uint32)
    objs, tris = _zero_run(flat)
    assert (p[tris, :, 2] > 0).all()
    p[tris, :, 0] = -np.abs(p[tris, :, 0]) - np.float32(1.0)
    run = [int(i) for i in nonempty_leaves(flat) if flat.tri_obj[flat.node_first[i]] in objs]
    first = {}
    for i in run:
        r = leaf_rows(flat, i)
        for axis in (2, 0):
            slots = np.sort(rng.choice(3 * r.size, size=min(3 * r.size, int(rng.integers(2, 5))), replace=False))
            u[r[slots // 3], slots % 3, axis] = np.where(rng.integers(0, 2, slots.size) == 1, SIGN_BIT, 0).astype(np.uint32)
            first[(i, axis)] = (r[slots[0] // 3], slots[0] % 3)
    root = int(flat.obj_root[0])
    if flat.node_left[root] >= 0:
        a, b = first_leaf_below(flat, flat.node_left[root]), first_leaf_below(flat, flat.node_right[root])
        for axis, (sa, sb) in ((2, (0, SIGN_BIT)), (0, (SIGN_BIT, 0))):
            u[first[(a, axis)] + (axis,)] = sa; u[first[(b, axis)] + (axis,)] = sb
    return p, dict(leaves=np.array(run), tri=tris, objs=objs)


def _subnormal_bits(rng, n):
    """n subnormals of +-1.4e-45 .. +-1e-39 as bit patterns (a zero exponent field, the fraction log-uniform), either sign."""
    frac = np.exp(rng.uniform(0.0, np.log(713000.0), n)).astype(np.uint32)
    return np.maximum(frac, 1).astype(np.uint32) | np.where(rng.integers(0, 2, n) == 1, SIGN_BIT, 0).astype(np.uint32)


def is_subnormal(a):
    a = np.asarray(a, np.float32)
    return (bits(a) & 0x7F800000 == 0) & (bits(a) & 0x007FFFFF != 0)


def subnormal(rng, flat, pts):
    """Every third leaf, on one axis (x, y, z in turn): every coordinate a subnormal of either sign or an exact zero of either sign.
    A compare that flushed its operands would see ties everywhere and keep the first element."""
    p = pts.copy(); u = p.view(np.uint32)
    leaves = nonempty_leaves(flat)[::3]
    mask = np.zeros(p.shape[:2] + (3,), bool)
    for j, i in enumerate(leaves):
        r = leaf_rows(flat, int(i))
        n = 3 * r.size
        v = _subnormal_bits(rng, n)
        zero = rng.random(n) < 0.3
        v = np.where(zero, v & SIGN_BIT, v).astype(np.uint32)
        assert is_subnormal(from_bits(v))[~zero].all() and (from_bits(v)[zero] == 0).all(), "subnormals as drawn"
        u[r, :, j % 3] = v.reshape(r.size, 3)
        assert np.array_equal(bits(p[r, :, j % 3]).reshape(-1), v), "subnormals as stored"
        mask[r, :, j % 3] = ~zero.reshape(r.size, 3)
    assert is_subnormal(p[..., :3])[mask].all() and mask.sum() > 0, "subnormals in the family's array"
    return p, dict(leaves=leaves, mask=mask)


W_KINDS = ("generic", "negative", "huge_or_tiny", "zero", "minus_zero", "subnormal", "nan")


def w(rng, flat, pts):
    """xyzw points on a quarter of the triangles, one vertex each, every kind at every point position: w in [0.25, 4], negative, near
    1e+-30, +0, -0, subnormal, NaN.  The box ignores w; the records divide by it."""
    p = pts.copy(); u = p.view(np.uint32)
    pick = _spread(rng, pts, max(21, p.shape[0] // 4))
    k = np.arange(pick.size)
    tag = dict(tri=pick, kind=k % 7, vertex=(k // 7) % 3)
    g = rng.uniform(0.25, 4.0, pick.size)
    val = np.select([tag["kind"] == 0, tag["kind"] == 1, tag["kind"] == 2, tag["kind"] == 3, tag["kind"] == 4],
                    [g, -g, np.where(k % 2 == 0, 1e30, 1e-30) * rng.uniform(0.5, 2.0, pick.size), 0.0, -0.0], 1.0).astype(np.float32)
    vb = bits(val).copy()
    vb[tag["kind"] == 4] = SIGN_BIT
    vb[tag["kind"] == 5] = _subnormal_bits(rng, int((tag["kind"] == 5).sum()))
    vb[tag["kind"] == 6] = _nan_bits(rng, (int((tag["kind"] == 6).sum()),))
    u[pick, tag["vertex"], 3] = vb
    return p, tag


def records(rng, flat, pts):
    """leaf_vectors.record_points() as it stands (the `records` tree holds them): w != 1, slivers, zero area, cross products that
    overflow or underflow, subnormals."""
    return pts.copy(), {}


FAMILIES = dict(nan_some=nan_some, nan_leaf=nan_leaf, nan_object=nan_object, inf=inf, fltmax=fltmax, zeros=zeros, subnormal=subnormal, w=w)
UNTOUCHED_BOXES = ("w",)                      # families that leave every xyz as it was: the boxes are flat_scene's own, bit for bit
ALL_FINITE = ("fltmax", "zeros", "subnormal")  # every xyz finite: the boxes are numpy's min / max as values
WALK_MIX = ("nan_some", "nan_leaf", "nan_object", "inf", "w")
BUILD_MIX = ("nan_some", "inf", "w")


@functools.lru_cache(maxsize=None)
def points(names, tree_name):
    """(points, {family: tags}) of tree(tree_name) with the families `names` (a name or a tuple of names) applied in order.  Made once,
    shared, never changed."""
    names = (names,) if isinstance(names, str) else tuple(names)
    flat = tree(tree_name)
    p = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4).copy()
    tags = {}
    for nm in names:
        fn = records if nm == "records" else FAMILIES[nm]
        rng = np.random.default_rng([77, sorted(list(FAMILIES) + ["records"]).index(nm), sum(map(ord, tree_name))])
        p, tags[nm] = fn(rng, flat, p)
        assert p.dtype == np.float32 and p.shape == (flat.n_tris, 3, 4)
    p.setflags(write=False)
    return p, tags


@functools.lru_cache(maxsize=None)
def edge_scene(names, tree_name):
    """edge_flat of points(names, tree_name): made once, shared."""
    return edge_flat(tree(tree_name), points(names, tree_name)[0])


def edge_normals(rng, n_rows, width):
    """Normal rows that carry what a copy must not touch: NaN payloads of both kinds, -0, subnormals, among ordinary values."""
    nrm = rng.uniform(-1.0, 1.0, (n_rows, width)).astype(np.float32)
    u = nrm.view(np.uint32).reshape(-1)
    k = np.arange(u.size)
    u[k % 7 == 1] = QUIET_NAN | 0x1234 | np.where(k[k % 7 == 1] % 2 == 0, SIGN_BIT, 0).astype(np.uint32)
    u[k % 7 == 3] = SIGNALLING_NAN | 0x0ABC
    u[k % 7 == 4] = SIGN_BIT
    u[k % 7 == 6] = _subnormal_bits(rng, int((k % 7 == 6).sum()))
    return nrm


# ---- the matrices of a pose ------------------------------------------------------------------------------------------------------------
MATRIX_KINDS = ("inf_entry", "nan_entry", "scale_2p100", "turn_2p125", "scale_2m140", "zero", "proj_generic", "proj_zero", "mirror")


def turn(centre, axis, deg):
    """A rigid turn about a point, column-major."""
    a = np.radians(deg)
    v = np.asarray(axis, np.float64); v = v / np.linalg.norm(v)
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
    M = np.eye(4); M[:3, :3] = R; M[:3, 3] = np.asarray(centre, np.float64) - R @ np.asarray(centre, np.float64)
    return np.ascontiguousarray(M.T.reshape(16), np.float32)


def special_objects(flat):
    """The objects that take the family's matrix: every other object with triangles, at most half of all."""
    full = [k for k in range(flat.n_objects) if (flat.tri_obj == k).any()]
    return np.array(full[1::2][:flat.n_objects // 2])


def matrices(kind, flat):
    """n_objects x 16, column-major: a rigid turn about its own centre for every object, and the matrix of `kind` for special_objects."""
    assert kind in MATRIX_KINDS
    P = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)
    m = np.empty((flat.n_objects, 16), np.float32)
    centre = []
    for k in range(flat.n_objects):
        v = P[flat.tri_obj == k][..., :3].reshape(-1, 3)
        centre.append(v.mean(0) if len(v) else np.zeros(3))
        m[k] = turn(centre[k], (0.3 + 0.1 * (k % 5), 1.0, 0.2 * (k % 3)), 15.0 + 5.0 * (k % 7))
    for j, k in enumerate(special_objects(flat)):
        c = centre[k].astype(np.float64)
        M = np.eye(4)
        if kind in ("inf_entry", "nan_entry"):
            m[k, (5 * j + 1) % 16] = np.inf if kind == "inf_entry" else np.nan
            continue
        if kind == "scale_2p100":
            M[:3, :3] *= 2.0 ** 100
        elif kind == "turn_2p125":                                      # the points overflow; inf - inf appears in the sums
            M = m[k].reshape(4, 4).T.astype(np.float64); M[:3] *= 2.0 ** 125
        elif kind == "scale_2m140":
            M[:3, :3] *= 2.0 ** -140
        elif kind == "zero":
            M[:] = 0.0
        elif kind == "proj_generic":                                    # w' = 1 + a . (p - centre): inexact divides
            a = np.array([0.004, -0.003, 0.002])
            M[3, :3] = a; M[3, 3] = 1.0 - a @ c
        elif kind == "proj_zero":                                       # w' = x - x0, exactly 0 at the object's first point
            M[3] = (1.0, 0.0, 0.0, -float(P[flat.tri_obj == k][0, 0, 0]))
        elif kind == "mirror":
            M[0, 0] = -1.0; M[0, 3] = 2.0 * c[0]
        with np.errstate(over="ignore"):
            m[k] = np.ascontiguousarray(M.T.reshape(16), np.float32)
    return m
