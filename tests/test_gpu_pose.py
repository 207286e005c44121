"""GPU (-m gpu): srt_scene_pose -- objects moved by matrix, the hierarchy refitted on the device (include/srt.h, POSE).

Every case creates the scene, sets the pose source, poses it, and compares with a SECOND scene made by srt_scene_create from the
test's own restatement (tests/pose_ref.py: same order, same tree, moved points, refitted boxes):
  * records: both triangle records, texel coordinates, normals, texture ids and the non-box words of the 32 B, 64 B and root node
    records byte for byte; the box floats inside those records equal as floats (only -0 against +0 can differ under that rule, and
    no compare of the slab test can tell them apart);
  * frames against the oracle run with the device's pow on pose_ref's flat scene, at the bar of gpu_frames.compare_exact."""
import ctypes as C

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import pose_ref
import scenes
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def T():
    from simple_raytracer_amd import build, host
    build.build_host()
    return host.Transformation


def same_records(got, want, what=""):
    for k in ("tris", "tris_o", "tri_tex"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k}"
    for k in ("tri_texcoord", "tri_normals"):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{what}: {k}"
    for k in ("nodes", "wide", "root_nodes"):
        gb, gr = pose_ref.split_boxes(got, k); wb, wr = pose_ref.split_boxes(want, k)
        assert np.array_equal(gr, wr), f"{what}: {k}, words beside the boxes"
        assert np.array_equal(gb, wb), f"{what}: {k}, {int((gb != wb).sum())} box floats differ"


def check_pose(srt, oracle, ds, flat0, mats, params, col=None, mat=None, what=""):
    """pose(mats) on ds (created from flat0, pose source set) against pose_ref's flat scene: records, then every frame of `params`.
    Returns the pipelines the frames took."""
    ds.pose(mats, col, mat)
    want = pose_ref.pose_flat(flat0, mats, col, mat)
    fresh = srt.DeviceScene(want)
    same_records(ds.records(), fresh.records(), what)
    pipes = []
    for p in params:
        o = ds.render(p)
        c = oracle.render(want, p, pow="device")
        gf.compare_exact(srt, o, c, gf.owned(p), want, p, f"{what} L={p.n_lights}")
        if p.flags & abi.SRT_FLAG_COUNT_WORK:
            assert o["stats"]["node_tests"] == c["stats"]["node_tests"] and o["stats"]["tri_tests"] == c["stats"]["tri_tests"], what
        pipes.append(ds.pipeline)
    fresh.close()
    return pipes


def about(T, centre, m):
    """m applied about a point: translate(centre) * m * translate(-centre)."""
    return T.mul(T.changeObjPosition(*centre), T.mul(m, T.changeObjPosition(*[-x for x in centre])))


def test_four_cubes_orbit_every_key_a_tie(srt, oracle, T):
    """four_cubes: every sort key of the build is a tie, three clones have zero material.  Light-sample counts 1, 8 and 16 are the
    counts at which the library switches shadow pipelines; the work counters are compared once."""
    g = gu.GoldenScene("cubes4_a0")
    ds = srt.DeviceScene(g.flat); ds.set_pose_source()
    pipes = []
    for k, a in enumerate(pose_ref.ORBIT_ANGLES):
        mats = np.tile(pose_ref.orbit_matrix(T, a), (g.flat.n_objects, 1))
        ps = [g.params(128, 96, L, flags=abi.SRT_FLAG_COUNT_WORK if (k == 0 and L == 8) else 0) for L in ((1, 8, 16) if k == 0 else (2,))]
        pipes += check_pose(srt, oracle, ds, g.flat, mats, ps, what=f"four cubes {a} deg")
    assert len(set(pipes)) > 1, pipes


def test_ground_bunny_orbit_and_determinism(srt, oracle, T):
    """K3 scene over three orbit angles, light-sample counts 1, 8, 16; two pose calls with the same matrices leave bitwise identical
    records (the reduction has a fixed order)."""
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    pipes = []
    for k, a in enumerate(pose_ref.ORBIT_ANGLES):
        mats = np.tile(pose_ref.orbit_matrix(T, a), (flat.n_objects, 1))
        ps = [g.params(192, 108, L, flags=abi.SRT_FLAG_COUNT_WORK if (k == 0 and L == 1) else 0) for L in ((1, 8, 16) if k == 0 else (1,))]
        pipes += check_pose(srt, oracle, ds, flat, mats, ps, what=f"ground bunny {a} deg")
    assert len(set(pipes)) > 1, pipes
    r1 = ds.records()
    ds.pose(mats)
    r2 = ds.records()
    for k in r1:
        assert np.array_equal(r1[k].view(np.uint8), r2[k].view(np.uint8)), k


def test_one_object_turns_while_the_others_stay(srt, oracle, T):
    """What camera mode cannot do: the bunny turns about its own centre, the slab and the light stay."""
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    kb = flat.names.index("./obj/stanford-bunny.obj")
    c = flat.tri_points[flat.tri_obj == kb][..., :3].reshape(-1, 3).mean(0)
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    for deg in (25.0, -140.0):
        mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1))
        mats[kb] = about(T, [float(x) for x in c], T.rotateObjY(T.radians(deg)))
        check_pose(srt, oracle, ds, flat, mats, [g.params(192, 108, 2)], what=f"bunny alone {deg} deg")
    # the slab's records are the created scene's own, bit for bit (identity matrix)
    ks = 1 - kb
    sel = flat.tri_obj == ks
    assert np.array_equal(ds.records()["tris"][sel], srt.DeviceScene(flat).records()["tris"][sel])


def test_non_rigid_matrices(srt, oracle, T):
    """Scale + shear, another matrix per object, new colours and materials with them (one shininess no longer an integer: the
    integer-shininess kernels must not be taken for this frame)."""
    g = gu.GoldenScene("cubes4_a0")
    flat = g.flat
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = []
    for k in range(flat.n_objects):
        c = [float(x) for x in flat.tri_points[flat.tri_obj == k][..., :3].reshape(-1, 3).mean(0)]
        mats.append(about(T, c, T.mul(T.shearObj(0.25 * k, 0.0, -0.125, 0.0, 0.0, 0.375), T.scaleObj(1.25, 0.75 + 0.1 * k, 1.5))))
    col = np.array([[0.9, 0.1, 0.1], [0.1, 0.9, 0.1], [0.1, 0.1, 0.9], [0.8, 0.8, 0.2]], np.float32)[:flat.n_objects]
    mat = np.tile(np.array([0.2, 0.5, 15.0], np.float32), (flat.n_objects, 1)); mat[0, 2] = 12.5
    check_pose(srt, oracle, ds, flat, np.array(mats), [g.params(128, 96, 1), g.params(128, 96, 8)], col, mat, "shear + scale")
    # ... and back to integer exponents, colours untouched
    mat[0, 2] = 9.0
    check_pose(srt, oracle, ds, dataclass_with(flat, obj_color=col), np.array(mats), [g.params(128, 96, 1)], None, mat, "shear + scale, integer shininess")


def dataclass_with(flat, **kw):
    import dataclasses
    return dataclasses.replace(flat, **kw)


def test_textured_scene_with_smooth_normals(srt, oracle, T):
    """scene_texquad with vertex normals: texel coordinates, texture ids and normals stay where they are (the reference's
    transformTriangles moves points only), the textured frame follows the pose."""
    g = gu.GoldenScene("texquad")
    P = g.flat.tri_points[..., :3]
    nrm = P - P.reshape(-1, 3).mean(0) + np.array([0.0, 0.0, -40.0], np.float32)
    nrm = nrm / np.linalg.norm(nrm, axis=2, keepdims=True)
    flat = dataclass_with(g.flat, tri_normals=np.ascontiguousarray(nrm.reshape(-1, 9), np.float32))
    assert flat.n_textures >= 1 and (flat.tri_tex >= 0).any()
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    W, H, L = g.renders[0]
    for a in (3.0, -8.0):
        mats = np.tile(pose_ref.orbit_matrix(T, a), (flat.n_objects, 1))
        check_pose(srt, oracle, ds, flat, mats, [g.params(W, H, L, flags=abi.SRT_FLAG_SMOOTH_NORMALS), g.params(W, H, 1)], what=f"texquad {a} deg")


def test_soup_of_100k_triangles_in_four_objects(srt, oracle, T):
    """Four interleaved objects of 25 000 triangles each: deep trees, many bottom subtrees per object, boxes that overlap heavily."""
    from simple_raytracer_amd import host
    recipe, meshes = scenes.soup(100000)
    flat = host.build_flat_scene(recipe, meshes)
    assert flat.n_objects == 4 and flat.n_tris == 100000
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = [about(T, [0.0, 0.0, 1000.0], T.rotateObjZ(T.radians(15.0 * k))) for k in range(4)]
    mats[3] = T.mul(T.changeObjPosition(40.0, -25.0, 60.0), mats[3])
    p = abi.make_params(160, 90, abi.light_staircase(recipe.light, 2), flags=abi.SRT_FLAG_COUNT_WORK)
    check_pose(srt, oracle, ds, flat, np.array(mats), [p], what="soup")


def test_one_triangle_object_keeps_its_empty_leaf(srt, oracle, T):
    flat = pose_ref.one_triangle_scene()
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (2, 1))
    mats[flat.names.index("one")] = about(T, [0.0, 0.0, 205.0], T.rotateObjZ(T.radians(30.0)))
    p = abi.make_params(240, 160, abi.light_staircase((120.0, -260.0, -40.0), 2), flags=abi.SRT_FLAG_COUNT_WORK)
    check_pose(srt, oracle, ds, flat, mats, [p], what="one triangle")
    nodes, _ = pose_ref.split_boxes(ds.records(), "nodes")
    assert (nodes[:, 0] == pose_ref.FLT_MAX).any() and (nodes[:, 3] == -pose_ref.FLT_MAX).any()


def test_pose_render_pose_render_on_one_stream_without_a_host_wait(srt, oracle, T):
    """pose -> render -> pose -> render enqueued on the scene's own stream, one wait at the end: each frame is the frame of its pose."""
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    L_ = srt.load()
    ds = srt.DeviceScene(flat); ds.set_pose_source()
    p = g.params(192, 108, 2)
    ma, mb = [np.tile(pose_ref.orbit_matrix(T, a), (flat.n_objects, 1)) for a in (3.0, -8.0)]
    ds.pose(ma); ds.render(p)                                   # warm: workspace, lights and staging are allocated
    fa, fb = gf.PinnedFrame(L_, 108, 192), gf.PinnedFrame(L_, 108, 192)
    try:
        ds.pose(ma)
        assert L_.srt_render_async(ds.h, C.byref(p), *fa.ptrs) == 0
        ds.pose(mb)
        assert L_.srt_render_async(ds.h, C.byref(p), *fb.ptrs) == 0
        ds.sync()
        oa, ob = fa.out(), fb.out()
    finally:
        fa.free(); fb.free()
    assert not np.array_equal(oa["hit_id"], ob["hit_id"])
    for m, o, nme in ((ma, oa, "first"), (mb, ob, "second")):
        want = pose_ref.pose_flat(flat, m)
        c = oracle.render(want, p, pow="device")
        o["stats"] = c["stats"]                                  # (srt_sync reports the last frame only; the pixels are what is checked here)
        gf.compare_exact(srt, o, c, gf.owned(p), want, p, f"{nme} frame of the stream")


def test_shared_handle_update_and_argument_errors(srt, oracle, T):
    g = gu.GoldenScene("cubes4_a0")
    flat = g.flat
    ds = srt.DeviceScene(flat)
    mats = np.tile(pose_ref.orbit_matrix(T, 3.0), (flat.n_objects, 1))
    with pytest.raises(srt.SrtError) as e:                       # no pose source yet
        ds.pose(mats)
    assert e.value.code == abi.SRT_ERR_ARG
    ds.set_pose_source()
    with pytest.raises(srt.SrtError) as e:                       # another object count
        ds.pose(mats[:-1])
    assert e.value.code == abi.SRT_ERR_LAYOUT
    # a pose through a shared handle rewrites the records every handle reads; the pose source belongs to the records
    sh = ds.share()
    sh.pose(mats)
    want = pose_ref.pose_flat(flat, mats)
    fresh = srt.DeviceScene(want)
    same_records(sh.records(), fresh.records(), "shared handle")          # (records() waits for the device)
    p = g.params(128, 96, 2)
    for h in (ds, sh):
        gf.compare_exact(srt, h.render(p), oracle.render(want, p, pow="device"), gf.owned(p), want, p, "shared handle")
    sh.close()
    # srt_scene_update discards the pose source ...
    ds.update(want); ds.sync()
    with pytest.raises(srt.SrtError) as e:
        ds.pose(mats)
    assert e.value.code == abi.SRT_ERR_ARG
    same_records(ds.records(), fresh.records(), "a refused pose changes nothing")
    # ... and with a new one the poses apply to the updated scene's points
    ds.set_pose_source()
    check_pose(srt, oracle, ds, want, mats, [p], what="pose after update")


def test_renderer_pose_path_of_the_host_mirror(srt, oracle, T):
    """srt_host::Renderer::renderPosed: the scene uploaded once, one mat4 per object per frame, every frame the oracle's frame of
    pose_ref's flat scene; render() in between rebuilds as ever and the next posed frame uploads again."""
    from simple_raytracer_amd import host
    rec = scenes.four_cubes(T, 0.0)
    om = host.ObjectManager(); rec.replay(om, {"cube": gu.load_mesh("cube")})
    flat = om.flatten()
    W, H = 160, 120
    light = list(rec.light) + [1.0]
    def expect(f):
        p = abi.make_params(W, H, abi.light_staircase(rec.light, 2))
        p.background[0] = p.background[1] = p.background[2] = 0
        return oracle.render(f, p)["rgb8"].astype(np.float32)
    r = host.Renderer(0)
    for k, a in enumerate((3.0, -8.0, 0.5)):
        mats = np.tile(pose_ref.orbit_matrix(T, a), (flat.n_objects, 1))
        mats[1] = T.mul(T.changeObjPosition(0.0, 2.0 * k, 0.0), mats[1])              # one object on a path of its own
        if k == 2:
            r.render(om, W, H, light, light_amount=2)                                  # the drop-in path in between: rebuilds, discards the pose source
        img, n = r.render_posed(om, W, H, light, mats, light_amount=2)
        d = np.abs(img - expect(pose_ref.pose_flat(flat, mats)))
        assert d.max() <= 1.0 and (d.max(-1) > 0).sum() <= 2 and n > 1500, a
    with pytest.raises(host.HostError):
        r.render_posed(om, W, H, light, mats[:-1], light_amount=2)
