"""The refit tests' own restatement of srt_scene_refit_device (include/srt.h, REFIT) in numpy: a welded vertex buffer and its index
buffer, the points a refit gathers from them, and the flat scene the device records must equal afterwards -- flat's order and trees,
the new points, the boxes of pose's fold over them (tests/pose_ref.py: it is reused, not restated), the new normals.  No arithmetic
touches a point or a normal here either: they are copied."""
import dataclasses

import numpy as np

import pose_ref


def weld(flat):
    """(verts, tri_vertex): the distinct points of flat.tri_points, told apart by their bit patterns (n_verts x 4 float32), and per
    triangle the three vertex numbers in point order one, two, three (n_tris x 3 uint32, the scene's visit order)."""
    p = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 4)
    u, inv = np.unique(p.view(np.uint32), axis=0, return_inverse=True)
    return np.ascontiguousarray(u).view(np.float32), np.ascontiguousarray(inv.reshape(-1, 3), np.uint32)


def expand(verts, tri_vertex, stride):
    """The points an indexed refit gathers: n_tris x 3 x 4 from verts (n_verts x stride) through tri_vertex; a stride of 3 means
    w = 1.0f exactly."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, stride)
    tv = np.ascontiguousarray(tri_vertex, np.uint32).reshape(-1, 3)
    out = np.ones((tv.shape[0], 3, 4), np.float32)
    out[..., :stride] = v[tv]
    return out


def direct(points, stride):
    """The points a direct refit reads: n_tris x 3 x 4 from a buffer of n_tris x 3 points of `stride` floats."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3, stride)
    out = np.ones((p.shape[0], 3, 4), np.float32)
    out[..., :stride] = p
    return out


def expand_normals(vertex_normals, tri_vertex):
    """The normal rows an indexed refit writes: n_tris x 9, the three gathered n_verts x 3 rows in point order."""
    n = np.ascontiguousarray(vertex_normals, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(n[np.ascontiguousarray(tri_vertex, np.uint32).reshape(-1, 3)].reshape(-1, 9))


def refit_flat(flat, points, normals=None):
    """The flat scene srt_scene_refit_device leaves on the device: flat's order and trees, `points` (n_tris x 3 x 4), refitted boxes,
    and `normals` (n_tris x 9) where given."""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3, 4)
    assert pts.shape[0] == flat.n_tris
    mn, mx = pose_ref.boxes(flat, pts)
    kw = dict(tri_points=pts, node_min=mn, node_max=mx)
    if normals is not None:
        kw["tri_normals"] = np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
    return dataclasses.replace(flat, **kw)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_records(got, want, what=""):
    """DeviceScene.records() of a refitted scene against those of a scene created from refit_flat: both triangle records, texel
    coordinates, normals, texture ids and the words beside the boxes of the node records byte for byte; the box floats equal as floats
    (under the fold's rule only -0 against +0 can differ from numpy's fmin / fmax, and no compare of the slab test tells them apart)."""
    for k in ("tris", "tris_o", "tri_tex"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}: {int((got[k] != want[k]).any(-1).sum() if got[k].ndim > 1 else (got[k] != want[k]).sum())} records differ"
    for k in ("tri_texcoord", "tri_normals"):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k}"
    for k in ("nodes", "wide", "root_nodes"):
        gb, gr = pose_ref.split_boxes(got, k); wb, wr = pose_ref.split_boxes(want, k)
        assert np.array_equal(gr, wr), f"{what}: {k}, words beside the boxes"
        assert np.array_equal(gb, wb), f"{what}: {k}, {int((gb != wb).sum())} box floats differ"


def same_bytes(a, b, what=""):
    """Two DeviceScene.records() dicts, byte for byte."""
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k}"
