"""The closest-point query at its edges (include/srt_points.h): one small flat scene and batches of (point, radius) that sit on
every decision of the definition, for tests/test_gpu_point_edges.py to compare with tests/point_ref.py bit for bit.

The scene (tests/tree_shapes.flat_scene, tight boxes):
  object 0   the axis triangle (2,1,3) (6,1,3) (2,5,3) and the tilted triangle (40,2,1) (43,6,1) (40,2,13) -- small dyadic coordinates: every
             d, v and w of a lattice point is exact, so a lattice point lies exactly ON a vertex, an edge, the face or a Voronoi boundary
             (d1 == 0, d3 == d4, vc == 0, ...) --, a zero-area triangle (three times one point) and two collinear ones;
  object 1   object 0's triangles again: every result is a tie across the two objects, and the lowest id wins;
  object 2   a tree with an EMPTY leaf, whose box is (+FLT_MAX, -FLT_MAX), beside a leaf of 31 (slices) and one of 9;
  object 3   one triangle with a NaN and one with an inf coordinate, and a finite one: a record with non-finite values."""
import functools

import numpy as np

import tree_shapes as ts

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
A, B, C = F([2, 1, 3]), F([6, 1, 3]), F([2, 5, 3])
TA, TB, TC = F([40, 2, 1]), F([43, 6, 1]), F([40, 2, 13])


def tri(*rows):
    t = np.ones((len(rows), 3, 4), F)
    t[..., :3] = np.asarray(rows, F)
    return t


@functools.lru_cache(maxsize=None)
def scene():
    base = tri((A, B, C), (TA, TB, TC), ((20, 20, 20),) * 3, ((10, -5, 0), (12, -5, 0), (16, -5, 0)), ((-8, 0, 0), (-8, 4, 4), (-8, 1, 1)))
    rng = np.random.default_rng(3)
    far = ts.patch(rng, 40, (-60.0, 70.0, -30.0), (8.0, 8.0, 8.0), 3.0)
    bad = tri(((100, 0, 0), (101, np.nan, 0), (100, 1, 0)), ((110, 0, 0), (111, 0, 0), (110, np.inf, 0)), ((120, 0, 0), (121, 0, 0), (120, 1, 0)))
    objs = [dict(tris=base, leaves=(2, 3), shape="right_comb"), dict(tris=base, leaves=(1, 4), shape="left_comb"),
            dict(tris=far, leaves=(31, 0, 9), shape="random", seed=4), dict(tris=bad, leaves=(3,), shape="root_leaf")]
    flat = ts.flat_scene(objs)
    empty = (flat.node_count == 0) & (flat.node_left < 0)
    assert empty.sum() == 1 and (flat.node_min[empty] == ts.FLT_MAX).all() and (flat.node_max[empty] == -ts.FLT_MAX).all()
    return flat


def ulp_steps(p):
    """p (m x 3) and its six neighbours one ulp away along each axis: 7m x 3."""
    out = [p]
    for a in range(3):
        for to in (-INF, INF):
            q = p.copy()
            q[:, a] = np.nextafter(p[:, a], to)
            out.append(q)
    return np.concatenate(out)


def lattice():
    """Points on and around the two dyadic triangles, with their one-ulp neighbours: every vertex, edge, face and Voronoi boundary exactly,
    and one ulp to either side of it."""
    g = np.arange(-2.0, 9.5, 0.5, dtype=F)
    x, y, z = np.meshgrid(g, g, F([3.0, 3.5, 1.0]), indexing="ij")
    axis = np.stack([x, y, z], -1).reshape(-1, 3)
    # the tilted triangle: TA + e1 * v + e2 * w + n * h with dyadic v, w, h (e1 = (3,4,0), e2 = (0,0,12), n = (4,-3,0) is orthogonal to both)
    k = F([-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.5])
    v, w, h = np.meshgrid(k, k, F([0.0, 0.5, -2.0]), indexing="ij")
    e1, e2, n = TB - TA, TC - TA, F([4, -3, 0])
    tilted = (TA + v[..., None] * e1 + w[..., None] * e2 + h[..., None] * n).reshape(-1, 3).astype(F)
    return ulp_steps(np.concatenate([axis, tilted]))


def batches():
    """name -> (points m x 3, radius m or None).  Every batch is a call of its own in the GPU test; `all` is their concatenation with the
    radii written out (None as +inf), in one call of several workgroups."""
    out = {}
    lat = lattice()
    out["lattice, no radius"] = (lat, None)
    # the radius at the winner's distance: above the axis triangle's face the distance is exactly h, and h * h is exact
    h = F([0.5, 1.0, 2.0, 3.0])
    above = np.stack([np.full(4, 3.0, F), np.full(4, 2.0, F), 3.0 + h], 1).astype(F)
    out["radius = distance (closed)"] = (above, h.copy())
    out["radius one ulp below the distance"] = (above, np.nextafter(h, F(0.0)))
    on = np.stack([A, B, C, (A + B) / 2, (B + C) / 2, (A + C) / 2, F([3, 2, 3]), TA, (TA + TC) / 2]).astype(F)
    out["radius 0 on the surface"] = (on, np.zeros(len(on), F))
    out["radius 0 off the surface"] = (on + F([0, 0, 1]), np.zeros(len(on), F))
    out["radius -0"] = (on, np.full(len(on), -0.0, F))
    some = lat[:: max(1, len(lat) // 67)][:67]
    out["radius -1"] = (some, np.full(len(some), -1.0, F))
    out["radius NaN"] = (some, np.full(len(some), NAN, F))
    out["radius +inf"] = (some, np.full(len(some), INF, F))
    out["radius -inf"] = (some, np.full(len(some), -INF, F))
    out["radius tiny"] = (some, np.full(len(some), 1e-30, F))      # r * r underflows to 0
    out["radius huge"] = (some, np.full(len(some), 1e30, F))       # r * r overflows to +inf
    out["radii mixed"] = (some, np.resize(F([0.25, 1.0, 4.0, 30.0, 200.0, INF, -1.0, NAN, 0.0]), len(some)))
    # points that are not finite, or so far away that dist2 overflows
    wild = np.array([[NAN, 0, 0], [0, NAN, 0], [NAN, NAN, NAN], [INF, 0, 0], [0, -INF, 0], [INF, INF, -INF], [1e19, 0, 0], [0, -1e19, 1e19], [3e38, 3e38, 3e38],
                     [-3e38, 0, 3], [1e-40, 1e-40, 1e-40], [3, 2, 1e19]], F)
    out["wild points, no radius"] = (wild, None)
    out["wild points, radius 1e19"] = (wild, np.full(len(wild), 1e19, F))
    out["wild points, radius 5"] = (wild, np.full(len(wild), 5.0, F))
    # the degenerate triangles and the non-finite records from near and far
    rng = np.random.default_rng(9)
    near = np.concatenate([F([20, 20, 20]) + rng.uniform(-2, 2, (40, 3)), F([13, -5, 0]) + rng.uniform(-4, 4, (40, 3)), F([-8, 2, 2]) + rng.uniform(-3, 3, (40, 3)),
                           F([105, 0.5, 0]) + rng.uniform(-12, 22, (60, 3)), F([[20, 20, 20], [11, -5, 0], [14, -5, 0], [17, -5, 0], [-8, 2, 2], [-8, 5, 5]])]).astype(F)
    out["degenerate and non-finite triangles, no radius"] = (near, None)
    out["degenerate and non-finite triangles, radius 3"] = (near, np.full(len(near), 3.0, F))
    pts = np.concatenate([p for p, _ in out.values()])
    rad = np.concatenate([np.full(len(p), INF, F) if r is None else r for p, r in out.values()])
    out["all"] = (pts, rad)
    return out
