"""CPU-only: the pose extension's ABI surface (srt_scene_set_pose_source, srt_scene_pose) and the test's own restatement of its
arithmetic (tests/pose_ref.py), pinned to the host mirror -- which the goldens pin to the reference -- and to the reference's own
boxes.  No device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_util as gu
import pose_ref
from simple_raytracer_amd import abi, build, host, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f32p = C.POINTER(C.c_float)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def L():
    build.build_all()
    return lib.load()


def test_header_declares_and_library_exports_the_pose_entry_points(L):
    hdr = open(os.path.join(ROOT, "include", "srt.h")).read()
    declared = set(re.findall(r"^int\s+(srt_[a-z_0-9]+)\s*\(", hdr, re.M))
    for name in ("srt_scene_set_pose_source", "srt_scene_pose"):
        assert name in declared, name
        assert name in lib.ABI_SYMBOLS, name
        assert hasattr(L, name), name
    assert re.search(r"#define\s+SRT_ABI_VERSION\s+3\b", hdr) and L.srt_abi_version() == 3      # additive only
    assert hasattr(lib.DeviceScene, "set_pose_source") and hasattr(lib.DeviceScene, "pose")


def test_null_arguments_are_refused_without_device_work(L):
    pts = np.ones((1, 3, 4), np.float32)
    m = np.eye(4, dtype=np.float32).reshape(16)
    assert L.srt_scene_set_pose_source(None, None) == abi.SRT_ERR_ARG
    assert L.srt_scene_set_pose_source(None, pts.ctypes.data_as(_f32p)) == abi.SRT_ERR_ARG
    assert L.srt_scene_pose(None, 1, None, None, None, None) == abi.SRT_ERR_ARG
    assert L.srt_scene_pose(None, 1, m.ctypes.data_as(_f32p), None, None, None) == abi.SRT_ERR_ARG


@pytest.mark.parametrize("mesh", ["cube", "sphere", "bunny"])
def test_transform_restatement_is_the_mirrors_transformTriangles(mesh):
    """pose_ref.transform == ObjectManager::transformTriangles (glm's mat4 * vec4 association, w included) bit for bit, for the orbit
    matrices of the GPU tests and a non-rigid one, on points that have been through a placement first (so that no coordinate is a
    round number)."""
    build.build_host()
    T = host.Transformation
    om = host.ObjectManager()
    om.add_object("o", gu.load_mesh(mesh))
    om.transformTriangles("o", T.scaleObj(150.0, 137.0, 161.0)); om.transformTriangles("o", T.rotateObjX(T.radians(181.0)))
    om.transformTriangles("o", T.changeObjPosition(20.0, 170.0, 300.0))
    mats = [pose_ref.orbit_matrix(T, a) for a in pose_ref.ORBIT_ANGLES]
    mats.append(T.mul(T.shearObj(0.25, 0.0, -0.125, 0.0, 0.0, 0.375), T.scaleObj(1.25, 0.75, 1.5)))
    persp = np.eye(4, dtype=np.float32); persp[2, 3] = 0.001; persp[3, 3] = 0.9      # m[2][3], m[3][3]: w changes too
    mats.append(persp.reshape(16))
    for m in mats:
        base = om.points("o")
        want_in = base.copy()
        om.transformTriangles("o", m)
        got = pose_ref.transform(want_in, m)
        assert np.array_equal(bits(got), bits(om.points("o")))
    assert not np.array_equal(om.points("o")[..., 3], np.ones_like(base[..., 3]))      # the last matrix moved w


@pytest.mark.parametrize("name", ["cubes4_a0", "ground_bunny", "one_triangle"])
def test_box_restatement_gives_the_scenes_own_boxes_at_the_identity_pose(name):
    """The boxes of a golden scene are the reference's own (Object.cpp:205-221): the restated fold over the same points must give the
    same floats for every node, the (+FLT_MAX, -FLT_MAX) box of an empty leaf included."""
    flat = pose_ref.one_triangle_scene() if name == "one_triangle" else gu.GoldenScene(name).flat
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1))
    moved = pose_ref.transform_objects(flat, eye)
    assert np.array_equal(bits(moved), bits(flat.tri_points))
    mn, mx = pose_ref.boxes(flat, moved)
    assert np.array_equal(mn, flat.node_min.reshape(-1, 3)) and np.array_equal(mx, flat.node_max.reshape(-1, 3))
    posed = pose_ref.pose_flat(flat, eye)
    assert posed.n_nodes == flat.n_nodes and np.array_equal(posed.node_left, flat.node_left) and np.array_equal(posed.tri_obj, flat.tri_obj)
