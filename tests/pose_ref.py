"""The pose tests' own restatement of srt_scene_pose (include/srt.h, POSE) in numpy float32: the transform with glm's association,
the box folds, and the flat scene the device records must equal -- same order, same tree, moved points, refitted boxes.

numpy evaluates a * b + c * d in float32 without contraction as long as every step is a separate float32 array operation; every
expression below is written that way."""
import dataclasses

import numpy as np

import scenes

FLT_MAX = np.float32(3.4028234663852886e38)


def transform(points, m16):
    """glm's mat4 * vec4 (type_mat4x4.inl:562-573) on points[..., 4]: per component i,
    (m[0][i] * x + m[1][i] * y) + (m[2][i] * z + m[3][i] * w), all four components; m16 = 16 floats, column-major."""
    p = np.ascontiguousarray(points, np.float32)
    m = np.ascontiguousarray(m16, np.float32).reshape(4, 4)              # m[c][i]
    x, y, z, w = p[..., 0], p[..., 1], p[..., 2], p[..., 3]
    out = np.empty_like(p)
    with np.errstate(all="ignore"):
        for i in range(4):
            a0 = m[0, i] * x
            a1 = m[1, i] * y
            a2 = m[2, i] * z
            a3 = m[3, i] * w
            s0 = a0 + a1
            s1 = a2 + a3
            out[..., i] = s0 + s1
    assert out.dtype == np.float32
    return out


def transform_objects(flat, matrices):
    """Every triangle's points by its object's matrix: matrices = n_objects x 16."""
    ms = np.ascontiguousarray(matrices, np.float32).reshape(flat.n_objects, 16)
    pts = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)
    out = pts.copy()
    for k in range(flat.n_objects):
        sel = flat.tri_obj == k
        out[sel] = transform(pts[sel], ms[k])
    return out


def _fold(v):
    """The reference's box fold over the rows of v (k x 3), from (+FLT_MAX, -FLT_MAX): `if (v < mn) mn = v; if (mx < v) mx = v;`.
    As a value: the smallest / largest element that compares at all -- a NaN never enters, +inf never lowers mn below FLT_MAX's
    start (inf < FLT_MAX is false), -inf does.  fmin / fmax with the start value as `initial` are exactly that for a quiet NaN.
    For a signalling one numpy's fmin / fmax return NaN, and a reduction over one loses elements: every NaN is made quiet first
    (tests/refit_edges.py, nan_some)."""
    v = np.where(np.isnan(v), np.float32(np.nan), np.asarray(v, np.float32))
    mn = np.fmin.reduce(v, axis=0, initial=FLT_MAX) if len(v) else np.full(3, FLT_MAX, np.float32)
    mx = np.fmax.reduce(v, axis=0, initial=-FLT_MAX) if len(v) else np.full(3, -FLT_MAX, np.float32)
    return mn.astype(np.float32), mx.astype(np.float32)


def boxes(flat, points):
    """node_min / node_max (n_nodes x 3) of flat's trees over `points` (n_tris x 3 x 4): a leaf folds its triangles in visit order,
    points one, two, three, raw xyz; an inner node is the fold over all triangles below it = combine(left, right), which keeps the
    left operand on ties (only the sign of a zero could tell, and box floats are compared with ==)."""
    xyz = np.ascontiguousarray(points, np.float32).reshape(-1, 3, 4)[..., :3]
    nN = flat.n_nodes
    mn = np.empty((nN, 3), np.float32); mx = np.empty((nN, 3), np.float32)
    done = np.zeros(nN, bool)
    for root in flat.obj_root:
        stack = [(int(root), False)]
        while stack:
            i, seen = stack.pop()
            l, r = int(flat.node_left[i]), int(flat.node_right[i])
            if l < 0:
                f, c = int(flat.node_first[i]), int(flat.node_count[i])
                mn[i], mx[i] = _fold(xyz[f:f + c].reshape(-1, 3) if c else xyz[:0].reshape(-1, 3))
                done[i] = True
            elif not seen:
                stack.append((i, True)); stack.append((r, False)); stack.append((l, False))
            else:
                mn[i] = np.where(mn[r] < mn[l], mn[r], mn[l])
                mx[i] = np.where(mx[l] < mx[r], mx[r], mx[l])
                done[i] = True
    assert done.all()
    return mn, mx


def pose_flat(flat, matrices, obj_color=None, obj_material=None):
    """The flat scene srt_scene_pose leaves on the device: flat's order and trees, moved points, refitted boxes."""
    pts = transform_objects(flat, matrices)
    mn, mx = boxes(flat, pts)
    kw = dict(tri_points=pts, node_min=mn, node_max=mx)
    if obj_color is not None:
        kw["obj_color"] = np.ascontiguousarray(obj_color, np.float32).reshape(-1, 3)
    if obj_material is not None:
        kw["obj_material"] = np.ascontiguousarray(obj_material, np.float32).reshape(-1, 3)
    return dataclasses.replace(flat, **kw)


ORBIT_ANGLES = (0.5, 3.0, -8.0)       # degrees the camera has turned against the pose the scene was created at


def orbit_matrix(T, angle_deg):
    """M_k = inverse(view_k) * view_0 of an orbit whose camera turns about the origin (scenes.orbit_view_matrix with radius 0), folded
    with the mirror's mat4 product and inverse: takes frame 0's view-space geometry to frame k's."""
    v0 = scenes.orbit_view_matrix(T, 0.0, 0.0, 0.0, 0.0)
    vk = scenes.orbit_view_matrix(T, 0.0, angle_deg, 0.0, 0.0)
    return T.mul(T.inverse(vk), v0)


def split_boxes(rec, key):
    """The box floats and the other words of a device record array (DeviceScene.records()): (boxes as float32, rest as uint32).
    nodes / root_nodes: 8 words = 6 box floats, skip, leaf; wide: 16 words = 12 box floats, linfo, rinfo, node, rnode."""
    a = rec[key]
    nb = 12 if key == "wide" else 6
    return np.ascontiguousarray(a[:, :nb]).view(np.float32), a[:, nb:]


def one_triangle_scene():
    """A one-triangle object (the reference's builder leaves it an EMPTY left leaf, boxes (+FLT_MAX, -FLT_MAX)) over a slab, through
    the host mirror."""
    import golden_util as gu
    from simple_raytracer_amd import build, host
    build.build_host()
    T = host.Transformation
    om = host.ObjectManager()
    om.add_object("one", np.array([[[-30, -30, 200, 1], [30, -30, 200, 1], [0, 40, 210, 1]]], np.float32)); om.setColor("one", (0.9, 0.4, 0.1))
    om.createBoundingHierarchy("one")
    om.add_object("slab", gu.load_mesh("cube")); om.setColor("slab", (0.2, 0.6, 0.8))
    om.transformTriangles("slab", T.scaleObj(80.0, 4.0, 80.0)); om.transformTriangles("slab", T.changeObjPosition(0.0, 40.0, 220.0))
    om.createBoundingHierarchy("slab")
    flat = om.flatten()
    assert (flat.node_count[flat.node_left < 0] == 0).any(), "the one-triangle object has an empty leaf"
    return flat
