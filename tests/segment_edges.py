"""The edge inputs of the segment query (include/srt_segments.h) for tests/test_gpu_segment_edges.py: one small scene and named segments
with their radii, all ordinary inputs -- nothing here may fault.

The scene, one object, leaves of 2, 0, 1 and 1 triangles (an EMPTY leaf among them, boxes (+FLT_MAX, -FLT_MAX)):
  0  (0,0,1) (1,0,1) (0,1,1)     the unit right triangle in the plane z = 1
  1  (1,0,1) (1,1,1) (0,1,1)     its neighbour across the diagonal: the two share edge 2-3 of triangle 0
  2  (4,0,1) (5,0,1) (6,0,1)     zero area
  3  (8,0,1) (inf,0,1) (8,1,NaN) not finite
cases(): (names, segments n x 6, radii n).  A case without a radius of its own appears twice, with r = 0.75 (box test 2 applies to the
sloped ones) and r = +inf (every triangle is a candidate, the zero-area and the non-finite one included)."""
import numpy as np

import tree_shapes as ts

F = np.float32
INF, NAN = F(np.inf), F(np.nan)


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


def scene():
    tris = np.zeros((4, 3, 4), F); tris[..., 3] = 1.0
    tris[0, :, :3] = [[0, 0, 1], [1, 0, 1], [0, 1, 1]]
    tris[1, :, :3] = [[1, 0, 1], [1, 1, 1], [0, 1, 1]]
    tris[2, :, :3] = [[4, 0, 1], [5, 0, 1], [6, 0, 1]]
    tris[3, :, :3] = [[8, 0, 1], [INF, 0, 1], [8, 1, NAN]]
    return ts.flat_scene([dict(tris=tris, leaves=[2, 0, 1, 1], shape="left_comb")])


def canonical(flat, x0):
    """The canonical id of the triangle whose first vertex has x == x0 and whose second has x == x0 + 1 (source triangles 0, 2, 3), or, for
    x0 == 1, the neighbour (source triangle 1)."""
    P = np.ascontiguousarray(flat.tri_points, F).reshape(-1, 3, 4)
    hit = np.flatnonzero((P[:, 0, 0] == F(x0)) & ((P[:, 1, 0] == F(x0 + 1)) | (P[:, 1, 0] == INF) | (x0 == 1)))
    assert hit.size == 1
    return int(hit[0])


def den_of(A, B):
    """den = a*e - b*b of the segment against edge 1-2 of triangle 0 (origin (0,0,1), dir (1,0,0)), in f32 as the definition has it."""
    d = (np.asarray(B, F) - np.asarray(A, F)).astype(F)
    a = F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    e, b = F(1.0), d[0]
    return F(F(a * e) - F(b * b))


def den_family():
    """Segments nearly parallel to edge 1-2: one with den exactly 0, the one with the smallest den > 0 and, if rounding gives one, one
    with den < 0, out of 4096 candidates from a fixed seed."""
    rng = np.random.default_rng(7)
    found = {}
    for _ in range(4096):
        A = np.array([rng.uniform(-0.5, 0.5), -0.5, 1.25], F)
        B = (A + np.array([rng.uniform(0.5, 1.5), rng.choice([0.0, 1.0]) * 2.0 ** -rng.integers(10, 14), 0.0], F)).astype(F)
        den = den_of(A, B)
        key = "den < 0" if den < 0 else "den == 0" if den == 0 else "den > 0"
        if key not in found or (key == "den > 0" and den < found[key][2]):
            found[key] = (A, B, den)
    return [(k, v[0], v[1], None) for k, v in sorted(found.items())]


def cases():
    rows = [
        # crossings at t = 0 and 1 and one ulp outside either
        ("crossing at t = 0", (0.25, 0.25, 1), (0.25, 0.25, 2), None),
        ("crossing, A one ulp above the plane", (0.25, 0.25, up(1)), (0.25, 0.25, 2), None),
        ("crossing, A one ulp below the plane", (0.25, 0.25, down(1)), (0.25, 0.25, 2), None),
        ("crossing at t = 1", (0.25, 0.25, 2), (0.25, 0.25, 1), None),
        ("crossing, B one ulp above the plane", (0.25, 0.25, 2), (0.25, 0.25, up(1)), None),
        ("crossing, B one ulp below the plane", (0.25, 0.25, 2), (0.25, 0.25, down(1)), None),
        ("crossing on the shared diagonal", (0.5, 0.5, 1.5), (0.5, 0.5, 0.5), None),
        ("crossing through a vertex", (1, 0, 1.5), (1, 0, 0.5), None),
        # in the plane, along an edge, at a vertex
        ("in the plane, through", (-0.5, 0.25, 1), (1.5, 0.25, 1), None),
        ("in the plane, outside", (-0.5, -0.25, 1), (1.5, -0.5, 1), None),
        ("collinear with edge 1-2, over it", (-1, 0, 1), (2, 0, 1), None),
        ("collinear with edge 1-2, beside it", (1.5, 0, 1), (3, 0, 1), None),
        ("collinear with the diagonal", (1.5, -0.5, 1), (-0.5, 1.5, 1), None),
        ("end A on a vertex", (0, 0, 1), (-1, -1, 2), None),
        ("end B on a vertex", (-1, -1, 2), (0, 0, 1), None),
        ("passing a vertex at a distance", (-0.5, 0.5, 1.25), (0.5, -0.5, 1.25), None),
        # u exactly 0 and 1 on edge 1-2
        ("u exactly 0", (0, -1, 1.5), (0, -0.5, 0.5), None),
        ("u exactly 1", (1, -1, 1.5), (1, -0.5, 0.5), None),
        # the radius, closed at the winner's own dist2 (0.5 above the plane: dist2 = 0.25 exactly)
        ("r * r == dist2", (0.25, 0.25, 1.5), (0.5, 0.125, 1.5), 0.5),
        ("r one ulp below", (0.25, 0.25, 1.5), (0.5, 0.125, 1.5), down(0.5)),
        ("r == 0 on a crossing", (0.25, 0.25, 2), (0.25, 0.25, 0), 0.0),
        ("r == -0 on a crossing", (0.25, 0.25, 2), (0.25, 0.25, 0), -0.0),
        ("r == 0 beside", (0.25, 0.25, 2), (0.25, 0.25, 1.5), 0.0),
        ("r negative", (0.25, 0.25, 2), (0.25, 0.25, 0), -1.0),
        ("r NaN", (0.25, 0.25, 2), (0.25, 0.25, 0), NAN),
        # end points
        ("A.x NaN", (NAN, 0.25, 2), (0.25, 0.25, 0), None),
        ("B.z NaN", (0.25, 0.25, 2), (0.25, 0.25, NAN), None),
        ("A NaN, a point", (NAN, NAN, NAN), (NAN, NAN, NAN), None),
        ("B.z -inf", (0.25, 0.25, 2), (0.25, 0.25, -INF), None),
        ("A.x +inf", (INF, 0.25, 2), (0.25, 0.25, 0), None),
        ("A = B = +inf", (INF, INF, INF), (INF, INF, INF), None),
        ("A 1e19", (1e19, 1e19, 1e19), (0.25, 0.25, 0), None),
        ("a point at 1e19", (1e19, 0.25, 2), (1e19, 0.25, 2), None),
        ("both ends 1e19", (1e19, 0.25, 2), (-1e19, 0.25, 0), None),
        # d with a zero, a subnormal and a 2^127 component, and their sloped neighbours
        ("d.x == 0", (0.25, 0.2, 2), (0.25, 0.3, 0.5), None),
        ("d.x subnormal", (0, 0.2, 2), (1e-40, 0.3, 0.5), None),
        ("d.x 2^-126", (0, 0.2, 2), (2.0 ** -126, 0.3, 0.5), None),
        ("d.x 2^-100", (0, 0.2, 2), (2.0 ** -100, 0.3, 0.5), None),
        ("d.x 2^127", (-2.0 ** 126, 0.2, 2), (2.0 ** 126, 0.3, 0.5), None),
        ("d.x 2^126", (-2.0 ** 125, 0.2, 2), (2.0 ** 125, 0.3, 0.5), None),
        ("d.x overflows", (-2.0 ** 127, 0.2, 2), (2.0 ** 127, 0.3, 0.5), None),
        ("sloped, a miss of every box", (3, 3, 3), (2, 2.5, 2), None),
        ("sloped, past the boxes its own box holds", (5, -1, 0.5), (-1, 5, 1.5), None),
        ("sloped, through the boxes", (-1, -0.5, 0.5), (9, 1.5, 1.5), None),
        # the other triangles
        ("across the zero-area triangle", (5, -1, 1), (5, 1, 1), None),
        ("beside the zero-area triangle", (4.5, 0.5, 1.5), (5.5, 0.25, 1.25), None),
        ("beside the triangle that is not finite", (8, 0.5, 1.5), (9, 0.25, 0.5), None),
    ] + den_family()
    names, seg, rad = [], [], []
    for name, A, B, r in rows:
        for rr in ((0.75, INF) if r is None else (r,)):
            names.append(name if r is None else name + " (its own radius)")
            seg.append(np.r_[np.asarray(A, F), np.asarray(B, F)]); rad.append(rr)
    return names, np.asarray(seg, F), np.asarray(rad, F)
