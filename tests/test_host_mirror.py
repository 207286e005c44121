"""CPU-only: the host-side C++ mirror (ObjectManager / Transformation / hierarchy builder / flattener)
reproduces, bit for bit, what the reference's host code produced (golden vectors exported from the
reference's own Node* trees and glm matrices)."""
import os

import numpy as np
import pytest

import golden_util as gu
import scenes
from mutants import mutate_bytes
from simple_raytracer_amd import abi, build


@pytest.fixture(scope="module")
def host():
    build.build_all()
    from simple_raytracer_amd import host
    host.load()
    return host


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_transformation_factories_match_reference(host):
    k = gu.load_kat(); T = host.Transformation
    rad = np.array([T.radians(float(a)) for a in k["tf_deg"]], np.float32)
    assert np.array_equal(bits(rad), bits(k["tf_rad"]))
    for name, fn in (("tf_rotx", T.rotateObjX), ("tf_roty", T.rotateObjY), ("tf_rotz", T.rotateObjZ)):
        got = np.stack([fn(float(r)) for r in k["tf_rad"]])
        assert np.array_equal(bits(got), bits(k[name])), name
    assert np.array_equal(bits(np.stack([T.scaleObj(*map(float, v)) for v in k["tf_scale_in"]])), bits(k["tf_scale"]))
    assert np.array_equal(bits(np.stack([T.changeObjPosition(*map(float, v)) for v in k["tf_scale_in"]])), bits(k["tf_translate"]))
    assert np.array_equal(bits(np.stack([T.mirrorObj(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)])), bits(k["tf_mirror"]))
    assert np.array_equal(bits(np.stack([T.shearObj(*map(float, v)) for v in k["tf_shear_in"]])), bits(k["tf_shear"]))
    view = np.stack([T.createViewMatrix(k["tf_view_pos"][i], k["tf_view_rot"][i]) for i in range(10)])
    assert np.array_equal(bits(view), bits(k["tf_view"]))
    assert np.array_equal(bits(np.stack([T.inverse(m) for m in k["tf_view"]])), bits(k["tf_view_inv"]))
    assert np.array_equal(bits(np.stack([T.mul(k["tf_view"][i], k["tf_view"][(i + 1) % 10]) for i in range(10)])), bits(k["tf_mul"]))
    assert np.array_equal(bits(np.stack([T.mul_vec4(k["tf_view_inv"][i], k["tf_vec"][i]) for i in range(10)])), bits(k["tf_mulvec"]))


def test_builder_reproduces_reference_main_scene(host):
    """The scene of the reference's checked-in main() (minus the cats): 177 k triangles in 5 objects, three of them textured
    clones.  Stored as sha256 of every array of the reference's export; GoldenScene.flat rebuilds it with the mirror and
    asserts the hashes (object order, trees, leaf order, transformed points, texel coordinates, texture bytes)."""
    g = gu.GoldenScene("main_nocats")
    f = g.flat
    assert (f.n_objects, f.n_nodes, f.n_tris, f.n_textures) == tuple(int(x) for x in g.z["scene_counts"])
    assert f.n_tris == 177463 and f.n_textures == 1 and (f.tri_tex >= 0).sum() == 3 * 36000


@pytest.mark.parametrize("name", [s for s in gu.SCENES if s not in ("texquad", "main_nocats")])
def test_builder_reproduces_reference_flat_scene(host, name):
    """Replay the scene recipe (same transforms, same createBoundingHierarchy calls) on the host mirror:
    object order, tree topology, boxes, leaf order and transformed points equal the reference's."""
    g = gu.GoldenScene(name)
    meshes = {k: gu.load_mesh(k) for k in g.recipe.meshes}
    flat = host.build_flat_scene(g.recipe, meshes)
    assert flat.names == g.flat.names, "unordered_map iteration order differs from the reference's"
    for k in ("obj_root", "node_left", "node_right", "node_first", "node_count", "tri_obj", "tri_tex"):
        assert np.array_equal(getattr(flat, k), getattr(g.flat, k)), k
    for k in ("node_min", "node_max", "tri_points", "obj_color", "obj_material", "tri_texcoord"):
        assert np.array_equal(bits(getattr(flat, k)), bits(getattr(g.flat, k))), k


def test_scene_scripts_with_host_transformation_equal_recipes(host):
    """The scene scripts evaluated with the host Transformation give the matrices the reference gave."""
    T = host.Transformation
    for name, fn in (("cube", lambda: scenes.one_cube(T, 0.0)), ("cubes4_a40", lambda: scenes.four_cubes(T, 40.0)),
                     ("ground_bunny", lambda: scenes.ground_bunny(T)), ("spheres6", lambda: scenes.six_spheres(T))):
        g = gu.GoldenScene(name)
        assert fn().to_json() == g.recipe.to_json(), name


def test_error_behaviour_mirrors_reference(host):
    om = host.ObjectManager()
    with pytest.raises(KeyError):                 # getTriangles -> objTriangles.at() throws (Object.cpp:174)
        om.num_tris("nope.obj")
    om.loadObjFile("/nonexistent/thing.obj")      # prints to stderr and carries on with an empty object (:35-39)
    assert om.num_tris("/nonexistent/thing.obj") == 0
    om.add_object("a", gu.load_mesh("cube"))
    with pytest.raises(host.HostError):           # no hierarchy: the reference null-derefs (:422); here an error
        om.flatten()


def test_one_triangle_object_has_empty_left_leaf(host):
    """Object.cpp:254-259 on a 1-triangle object: left half empty with the (+FLT_MAX, -FLT_MAX) box."""
    om = host.ObjectManager()
    om.add_object("t", gu.load_mesh("cube")[:1]); om.build_bvh("t")
    f = om.flatten()
    assert f.n_nodes == 3 and list(f.node_count) == [0, 0, 1]
    assert np.all(f.node_min[1] == np.float32(3.4028235e38)) and np.all(f.node_max[1] == np.float32(-3.4028235e38))


def test_hierarchy_keeps_the_geometry_of_build_time(host, oracle):
    """The reference's Node holds its triangles by value (Object.h:46-57): what is rendered is the object as it was when
    createBoundingHierarchy ran, whatever transformTriangles does afterwards.  Same here (and, where the compiled
    reference is present, the same flat scene as its Node trees give)."""
    T = host.Transformation
    om = host.ObjectManager()
    om.add_object("c", gu.load_mesh("cube")); om.transformTriangles("c", T.scaleObj(3.0, 4.0, 5.0)); om.build_bvh("c")
    before = om.flatten()
    om.transformTriangles("c", T.changeObjPosition(100.0, 0.0, 0.0))        # after the build: not rendered
    after = om.flatten()
    assert np.array_equal(bits(before.tri_points), bits(after.tri_points)) and np.array_equal(bits(before.node_min), bits(after.node_min))
    om.build_bvh("c")
    rebuilt = om.flatten()
    assert not np.array_equal(bits(before.tri_points), bits(rebuilt.tri_points))
    if oracle.ref_available():
        r = oracle.RefScene()
        r.add_object("c", gu.load_mesh("cube")); r.transform("c", T.scaleObj(3.0, 4.0, 5.0)); r.build_bvh("c")
        r.transform("c", T.changeObjPosition(100.0, 0.0, 0.0))
        rf = r.export()
        assert np.array_equal(bits(rf.tri_points), bits(after.tri_points)) and np.array_equal(bits(rf.node_max), bits(after.node_max))


def test_obj_loader_own_asset(host, tmp_path):
    """OBJ parsing: triangles, quads (shorter-diagonal split like tinyobjloader), negative indices, vt/vn."""
    p = tmp_path / "m.obj"
    p.write_text("v 0 0 0\nv 2 0 0\nv 2 1 0\nv 0 1 0\nv 0 0 5\nvt 0 0\nvn 0 0 1\n"
                 "f 1 2 3 4\nf 1/1/1 2/1/1 5/1/1\nf -1 -2 -3\n")
    om = host.ObjectManager(); om.loadObjFile(str(p))
    pts = om.points(str(p))
    assert pts.shape == (4, 3, 4) and np.all(pts[..., 3] == 1.0)
    # quad 0-1-2-3: |02|^2 = 5 == |13|^2 = 5 -> not '<' -> [0,1,3],[1,2,3]
    assert np.array_equal(pts[0, :, :3], [[0, 0, 0], [2, 0, 0], [0, 1, 0]])
    assert np.array_equal(pts[1, :, :3], [[2, 0, 0], [2, 1, 0], [0, 1, 0]])
    assert np.array_equal(pts[3, :, :3], [[0, 0, 5], [0, 1, 0], [2, 1, 0]])
    tc, col, ht, nrm = om.tri_attrs(str(p))
    assert np.array_equal(nrm[2, :3], [0, 0, 1]) and ht.sum() == 0


def test_parallel_sort_is_std_sort_to_the_element(host):
    """The hierarchy builder sorts big nodes with its own introsort whose partitions run in parallel; the order it leaves
    EQUAL keys in must be std::sort's (that order is the reference's leaf order, Object.cpp:193-247).  Arrays full of ties,
    sorted, reversed, organ-pipe, sizes around the thresholds: same permutation as std::sort."""
    rng = np.random.default_rng(1)
    sizes = [1, 2, 15, 16, 17, 33, 100, 127, 128, 129, 145, 146, 147, 255, 256, 257, 300, 1000, 4095, 4096, 4097, 5000, 16384, 20000, 69451, 131072]
    for trial, n in enumerate(sizes * 3):        # (sizes around 2 x 64 + 17: where the partition's branch-free block phase starts and stops)
        kind = trial % 6
        if kind == 0: k = rng.normal(size=n)
        elif kind == 1: k = rng.integers(0, max(2, n // 6), n)              # every key shared by ~6 elements, like first vertices
        elif kind == 2: k = np.sort(rng.integers(0, 50, n))
        elif kind == 3: k = np.sort(rng.normal(size=n))[::-1]
        elif kind == 4: k = np.where(rng.random(n) < 0.9, 1.0, rng.normal(size=n))
        else: k = np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]])
        a, b = host.sort_keys_both_ways(np.asarray(k, np.float32))
        assert np.array_equal(a, b), (n, kind)


def test_parsed_assets_are_cached_until_the_file_changes(host, tmp_path):
    """loadObjFile keeps a parsed OBJ per process (the reference's main() loads every asset again for every frame): a
    second load gives the same triangles, a rewritten file is parsed again."""
    p = tmp_path / "a.obj"
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    a = host.ObjectManager(); a.loadObjFile(str(p))
    b = host.ObjectManager(); b.loadObjFile(str(p))
    assert np.array_equal(bits(a.points(str(p))), bits(b.points(str(p)))) and a.num_tris(str(p)) == 1
    b.transformTriangles(str(p), host.Transformation.scaleObj(2.0, 2.0, 2.0))       # a loaded copy is the caller's own
    c = host.ObjectManager(); c.loadObjFile(str(p))
    assert np.array_equal(bits(a.points(str(p))), bits(c.points(str(p))))
    p.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 0 0 5\nf 1 2 3\nf 1 2 4\n")          # size (and time) change: parsed again
    d = host.ObjectManager(); d.loadObjFile(str(p))
    assert d.num_tris(str(p)) == 2


def test_polygon_faces_are_cut_like_tinyobj_earcut(host, tmp_path):
    """Faces with more than four corners: the reference's loader is tinyobjloader built with mapbox earcut
    (simple_raytracer.cpp:15-16).  tests/golden/polygons.npz: 29 faces of 5..120 corners (concave, both windings,
    collinear / duplicate corners, self-intersecting, degenerate, non-planar) and the 898 triangles the compiled reference
    made of them: same triangles, same order, same corner rotation."""
    z = np.load(os.path.join(gu.GOLDEN, "polygons.npz"))
    p = tmp_path / "polys.obj"
    p.write_bytes(z["obj"].tobytes())
    om = host.ObjectManager(); om.loadObjFile(str(p))
    got = om.points(str(p))
    assert got.shape == z["points"].shape
    assert np.array_equal(bits(got), bits(z["points"]))


def test_obj_loader_matches_reference_loader(host, oracle):
    """Where the reference and its assets are present: same triangles as tinyobjloader + Object.cpp:70-167."""
    if not (oracle.ref_available() and os.path.exists("/root/reference/obj/stanford-bunny.obj")):
        pytest.skip("reference assets not present")
    for name in ("cube.obj", "sphere.obj", "./obj/stanford-bunny.obj"):
        r = oracle.RefScene(); r.load_obj(name)
        om = host.ObjectManager()
        om.loadObjFile(os.path.join("/root/reference", name))
        assert np.array_equal(bits(om.points(os.path.join("/root/reference", name))), bits(r.points(name))), name
    # textured assets (JPEG / PNG diffuse maps with cwd-relative paths, house.obj has 5..32-corner faces): triangles,
    # per-vertex integer texel coordinates (Object.cpp:113-119, from the decoded image's size), normals, texture bytes
    old = os.getcwd()
    os.chdir("/root/reference")
    try:
        for name in ("./obj/tree/tree.obj", "./obj/horse/horse.obj", "./obj/grass/grass.obj", "./obj/bird/bird.obj", "./obj/house/house.obj"):
            r = oracle.RefScene(); r.load_obj(name)
            om = host.ObjectManager(); om.loadObjFile(name)
            assert np.array_equal(bits(om.points(name)), bits(r.points(name))), name
            for a, b in zip(om.tri_attrs(name), r.tri_attrs(name)):
                assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b), name
    finally:
        os.chdir(old)


def test_texture_decoders_and_textured_loader(host, tmp_path, oracle):
    """PNG decode + per-vertex texel coordinates (Object.cpp:113-119) against the reference's loader."""
    from PIL import Image
    rng = np.random.default_rng(3)
    tex = rng.integers(0, 256, (20, 32, 3), dtype=np.uint8)
    Image.fromarray(tex).save(tmp_path / "t.png")
    (tmp_path / "q.mtl").write_text(f"newmtl m\nmap_Kd {tmp_path}/t.png\n")
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nusemtl m\nv 0 0 1\nv 1 0 1\nv 1 1 1\nv 0 1 1\n"
                                    "vt 0.1 0.2\nvt 0.9 0.25\nvt 0.85 0.97\nvt 0.05 0.6\nf 1/1 2/2 3/3\nf 1/1 3/3 4/4\n")
    name = str(tmp_path / "q.obj")
    om = host.ObjectManager(); om.loadObjFile(name); om.build_bvh(name)
    tc, col, ht, _ = om.tri_attrs(name)
    assert ht.all()
    f = om.flatten()
    assert f.n_textures == 1 and np.array_equal(f.tex_rgb.reshape(20, 32, 3), tex) and np.all(f.tri_tex == 0)
    u = np.floor(np.float32(0.9) * 32) % 32; v = np.floor((np.float32(1.0) - np.float32(0.25)) * 20) % 20
    assert tc[0, 2] == u and tc[0, 3] == v
    if oracle.ref_available():
        r = oracle.RefScene(); r.load_obj(name, cwd=str(tmp_path))
        rtc, rcol, rht, _ = r.tri_attrs(name)
        assert np.array_equal(bits(tc), bits(rtc)) and np.array_equal(bits(col), bits(rcol)) and np.array_equal(ht, rht)


def test_jpeg_decoder_gives_the_reference_loaders_bytes(host, tmp_path, oracle):
    """The reference decodes textures with stbi_load(path, ..., 3) (Object.cpp:57) and most of its assets are JPEGs.
    tests/golden/jpeg.npz: 18 small JPEG files (baseline / progressive, 4:4:4 / 4:2:2 / 4:2:0 / grey / CMYK, restart
    intervals, one-pixel edges) with the bytes the compiled reference decoded them to: the loader's decoder must give
    exactly those.  Where the reference's assets are present, its seven 1024x1024 textures too (sha256 + live)."""
    import hashlib
    z = np.load(os.path.join(gu.GOLDEN, "jpeg.npz"))
    for name in z["names"]:
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(z[f"{name}_file"].tobytes())
        got = host.decode_image(str(p))
        assert got is not None, name
        assert got.shape == z[f"{name}_rgb"].shape and np.array_equal(got, z[f"{name}_rgb"]), name
    (tmp_path / "bad.jpg").write_bytes(z["base444_file"].tobytes()[:100])
    assert host.decode_image(str(tmp_path / "bad.jpg")) is None
    if os.path.exists("/root/reference/obj/tree/10445_Oak_Tree_v1_diffuse.jpg"):
        for a, want in zip(z["asset_names"], z["asset_sha"]):
            got = host.decode_image(os.path.join("/root/reference", str(a)))
            assert hashlib.sha256(got.tobytes()).hexdigest() == str(want), a
            if oracle.ref_available():
                assert np.array_equal(got, oracle.ref_stbi_load(os.path.join("/root/reference", str(a)))), a


def test_decoders_survive_corrupt_files(host, tmp_path):
    """Texture files are user input: byte flips, truncation and stray markers must end in "does not decode" or an image of
    the declared size, never in a crash.  (tools/host_sanitize.py runs the same mutants, and such of PNG / BMP / PPM and OBJ files, through an
    AddressSanitizer / UBSan build of the loaders.)"""
    z = np.load(os.path.join(gu.GOLDEN, "jpeg.npz"))
    rng = np.random.default_rng(5)
    seen_ok = seen_bad = 0
    for name in ("base420", "prog420", "rst444", "cmyk", "grey_prog"):
        base = z[f"{name}_file"].tobytes()
        for it in range(60):
            f = tmp_path / "m.jpg"; f.write_bytes(mutate_bytes(rng, base))
            got = host.decode_image(str(f))
            if got is None: seen_bad += 1
            else:
                seen_ok += 1
                assert got.ndim == 3 and got.shape[2] == 3 and got.size > 0
    assert seen_ok > 20 and seen_bad > 20


def test_integration_adapter_compiles_against_the_reference(tmp_path):
    """INTEGRATION.md option A: the adapter a reference maintainer adds (their ObjectManager / Node / Triangle types ->
    srt_scene_desc -> srt_render) compiles against the reference's own headers.  Build container only."""
    import re
    import subprocess
    ref = "/root/reference"
    if not os.path.exists(os.path.join(ref, "Object.h")):
        pytest.skip("reference sources not present")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    md = open(os.path.join(root, "INTEGRATION.md")).read()
    code = re.search(r"```cpp\n(// srt_adapter\.cpp.*?)```", md, re.S).group(1)
    built = open(os.path.join(root, "oracle", "srt_adapter.cpp")).read()
    assert code in built, "oracle/srt_adapter.cpp (what the GPU tests run) and the block in INTEGRATION.md differ"
    src = tmp_path / "srt_adapter.cpp"
    src.write_text(code)
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-w", "-I" + ref, "-I" + ref + "/library/glm-master/glm", "-I" + ref + "/library/tinyobjloader",
           "-I" + os.path.join(root, "include"), str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]


def test_camera_mode_definition_against_the_exact_frame(oracle):
    """Camera mode (srt_params.ray_matrix, an EXTENSION: the reference always moves the scene, never the camera): the scene of
    main()'s 4-cube script left in world space, rays taken there by the viewMatrix, must show what the reference's frame shows --
    same geometry, different rounding and a different hierarchy (built from world-space keys), so the comparison is geometric:
    t to 1e-4 relative and the 8-bit image within 2 LSB on all but a sliver of silhouette pixels."""
    import scenes
    from simple_raytracer_amd import abi, host
    T = host.Transformation
    cube = gu.load_mesh("cube")
    for angle in (0.0, 40.0):
        exact = scenes.four_cubes(T, angle)
        inv = scenes._orbit_view(T, 100.0, angle, 0.0, 0.0)
        view = scenes.orbit_view_matrix(T, 100.0, angle, 0.0, 0.0)
        world = scenes.in_world_space(exact, inv)
        f_exact = host.build_flat_scene(exact, {"cube": cube})
        f_world = host.build_flat_scene(world, {"cube": cube})
        W, H, L = 160, 120, 3
        a = oracle.render(f_exact, abi.make_params(W, H, abi.light_staircase(exact.light, L)))
        b = oracle.render(f_world, abi.make_params(W, H, abi.light_staircase(world.light, L), ray_matrix=view))
        hit_a, hit_b = a["hit_id"] >= 0, b["hit_id"] >= 0
        assert (hit_a != hit_b).mean() < 2e-3 and hit_a.sum() > 2000
        both = hit_a & hit_b
        assert np.abs(a["t"][both] - b["t"][both]).max() < 1e-4 * a["t"][both].max()
        d8 = np.abs(a["rgb8"].astype(int) - b["rgb8"].astype(int)).max(-1)
        assert (d8[both] > 2).mean() < 5e-3
