"""Pins the CPU restatement (oracle/srt_oracle.c) to the golden vectors produced by the compiled
reference (tests/golden/make_golden.py).  CPU only.  Bit-exact everywhere: the restatement and the
reference run the same IEEE ops and the same libm on the same host class."""
import numpy as np
import pytest

import golden_util as gu
import tonemap_ref as tr
from simple_raytracer_amd import abi


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def kat():
    return gu.load_kat()


def test_kat_ray_triangle(oracle, kat):
    for pre in ("rt", "rt2"):
        t = oracle.ray_triangle(kat[pre + "_ray"], kat[pre + "_tri"])
        assert np.array_equal(bits(t), bits(kat[pre + "_t"]))
    # the vectors really cover hits, misses, t == 0 and NaN
    t = kat["rt_t"]
    assert (t == -np.inf).sum() > 100 and (t > 0).sum() > 100 and np.isnan(t).sum() >= 1 and (t == 0).sum() >= 1


def test_kat_ray_aabb(oracle, kat):
    h = oracle.ray_aabb(kat["ab_ray"], kat["ab_box"])
    assert np.array_equal(h, kat["ab_hit"])
    assert 200 < h.sum() < h.size - 200
    # intersectRayAabb (origin-0 form, :204-248) == NoOrigin form whenever the origin is 0
    o0 = np.all(kat["ab_ray"][:, :3] == 0, axis=1)
    assert np.array_equal(kat["ab_hit"][o0], kat["ab_hit_origin0"][o0])


def test_kat_phong(oracle, kat):
    assert np.array_equal(bits(oracle.phong(kat["ph_in"])), bits(kat["ph_rgb"]))


def test_kat_barycentric(oracle, kat):
    assert np.array_equal(bits(oracle.barycentric(kat["bc_in"])), bits(kat["bc_uvw"]))


def test_kat_interp_normal(oracle, kat):
    assert np.array_equal(bits(oracle.interp_normal(kat["in_in"])), bits(kat["in_out"]))
    assert np.isnan(kat["in_out"][:8]).all()          # missing normals (0,0,0): 0 * (1/sqrt(0)) = NaN, as the reference


def test_kat_tonemap(oracle, kat):
    tone, q = oracle.tonemap(kat["tm_lin"])
    assert np.array_equal(bits(tone), bits(kat["tm_tone"]))
    assert np.array_equal(q, kat["tm_q"])


@pytest.mark.parametrize("reinhard", tr.REINHARD)
@pytest.mark.parametrize("gamma", tr.GAMMA)
def test_tonemap_against_float64(oracle, reinhard, gamma):
    """The oracle's tone map with non-default literals (glibc powf) against the float64 restatement: within 1 ulp everywhere,
    bitwise on all but 2e-3 of the inputs (glibc's powf is not correctly rounded on ~0.1 %), incl. zeros, denormals, the pow
    cut-offs, inf, NaN and negative colours; q is exactly the quantiser of its own tone."""
    lin = tr.inputs(reinhard, gamma)
    tone, q = oracle.tonemap(lin, reinhard, gamma)
    ref = tr.tone_ref(lin, reinhard, gamma)
    d = tr.ulp_diff(tone, ref)
    assert d.max() <= 1, f"{int((d > 1).sum())} tones differ by more than 1 ulp, e.g. lin {lin.reshape(-1)[np.argmax(d.reshape(-1))]}"
    assert (d > 0).mean() < 2e-3, int((d > 0).sum())
    assert np.array_equal(q, tr.quant_ref(tone))
    assert np.isnan(ref).any() and (ref == 0).any() and (q == 255).any() and ((q > 0) & (q < 255)).any()


def test_light_staircase(oracle, kat):
    tab = oracle.light_staircase(kat["ls_base"], 64)
    assert np.array_equal(bits(tab), bits(kat["ls_table"]))
    assert np.array_equal(bits(abi.light_staircase(kat["ls_base"], 64)), bits(kat["ls_table"]))
    # sample i differs from sample i-1 on axis (i-1)%3 only
    d = np.diff(tab, axis=0)
    for i in range(63):
        assert d[i, i % 3] > 0 and np.all(np.delete(d[i], i % 3) == 0)


@pytest.mark.parametrize("name,W,H,L", gu.all_renders())
def test_scene_matches_reference(oracle, name, W, H, L):
    g = gu.GoldenScene(name)
    o = oracle.render(g.flat, g.params(W, H, L))
    assert np.array_equal(o["hit_id"], g.out(W, H, L, "hit_id")), "closest-hit ids differ from the reference"
    assert np.array_equal(o["rgb8"], g.out(W, H, L, "rgb8")), "8-bit image differs from the reference"
    assert gu.sha(o["t"]) == str(g.out(W, H, L, "sha_t"))
    assert gu.sha(o["rgb_linear"]) == str(g.out(W, H, L, "sha_lin"))
    assert gu.sha(o["rgb_tone"]) == str(g.out(W, H, L, "sha_tone"))
    if g.out(W, H, L, "t") is not None:
        assert np.array_equal(bits(o["t"]), bits(g.out(W, H, L, "t")))
        assert np.array_equal(bits(o["rgb_linear"]), bits(g.out(W, H, L, "lin")))
    st = o["stats"]
    assert st["hit_rays"] == int((g.out(W, H, L, "hit_id") >= 0).sum())
    assert st["shadow_rays"] == st["hit_rays"] * L and st["primary_rays"] == W * H


def test_k4_bands_at_full_size_match_reference(oracle):
    """BASELINE configs[3] at its own shape (3840x2160, 64 light samples, composite scene with horse and house): two bands of
    scanlines the compiled reference rendered (a whole frame would be hours of reference time)."""
    g = gu.GoldenScene("k4")
    assert g.flat.n_objects == 7 and g.flat.n_tris == 223855 and g.flat.n_textures == 8
    assert len(g.bands) == 2
    for (W, H, L, y0, y1) in g.bands:
        assert (W, H, L) == (3840, 2160, 64)
        o = oracle.render(g.flat, g.band_params(W, H, L, y0, y1))
        assert np.array_equal(o["hit_id"], g.band_out(W, H, L, y0, y1, "hit_id"))
        assert np.array_equal(o["rgb8"], g.band_out(W, H, L, y0, y1, "rgb8"))
        assert gu.sha(o["t"]) == str(g.band_out(W, H, L, y0, y1, "sha_t")) and gu.sha(o["rgb_linear"]) == str(g.band_out(W, H, L, y0, y1, "sha_lin"))
        assert (o["hit_id"] >= 0).sum() > 3000


def test_scanline_blocks_tile_the_frame(oracle):
    """Block-cyclic scanline ownership (multi-GPU tiling): any split reassembles to the whole frame."""
    g = gu.GoldenScene("cubes4_a0")
    W, H, L = 128, 96, 8
    whole = oracle.render(g.flat, g.params(W, H, L))
    for world, rows in [(2, 8), (3, 5), (4, 16), (8, 7)]:
        hit = np.full((H, W), -9, np.int32); rgb8 = np.zeros((H, W, 3), np.uint8); lin = np.zeros((H, W, 3), np.float32)
        for rank in range(world):
            o = oracle.render(g.flat, g.params(W, H, L, block_rows=rows, block_first=rank, block_stride=world))
            ys = abi.rows_owned(H, rows, rank, world)
            assert o["hit_id"].shape[0] == len(ys)
            hit[ys] = o["hit_id"]; rgb8[ys] = o["rgb8"]; lin[ys] = o["rgb_linear"]
        assert np.array_equal(hit, whole["hit_id"]) and np.array_equal(rgb8, whole["rgb8"])
        assert np.array_equal(bits(lin), bits(whole["rgb_linear"]))


def test_oracle_vs_live_reference_random_scenes(oracle):
    """Where the compiled reference is present (this container), fuzz beyond the fixtures."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not built (no /root/reference here)")
    import scenes
    rng = np.random.default_rng(11)
    for trial in range(3):
        s = oracle.RefScene()
        n_obj = 3
        for k in range(n_obj):
            n = int(rng.integers(1, 60))
            c = rng.uniform(-60, 60, (n, 1, 3)).astype(np.float32); c[..., 2] += 260
            pts = np.ones((n, 3, 4), np.float32); pts[..., :3] = c + rng.uniform(-30, 30, (n, 3, 3)).astype(np.float32)
            s.add_object(f"o{k}", pts); s.set_color(f"o{k}", rng.uniform(0, 1, 3)); s.build_bvh(f"o{k}")
        flat = s.export()
        light = rng.uniform(-400, 400, 3).astype(np.float32)
        W, H, L = 96, 64, 1 + trial
        hit, t, tone, lin = s.trace(W, H, light, L)
        o = oracle.render(flat, abi.make_params(W, H, abi.light_staircase(light, L)))
        assert np.array_equal(o["hit_id"], hit)
        assert np.array_equal(bits(o["t"]), bits(t)) and np.array_equal(bits(o["rgb_linear"]), bits(lin))
        assert np.array_equal(bits(o["rgb_tone"]), bits(tone))


def test_supersampling_extension_definition(oracle):
    """spp = n x n (extension): sub-sample 0 of a 2x2 grid is the frame rendered with a -0.25 px offset; the
    pixel is the tone-mapped mean of the four sub-frames' pre-tone-map sums."""
    g = gu.GoldenScene("cubes4_a0")
    W, H, L = 64, 48, 2
    o4 = oracle.render(g.flat, g.params(W, H, L, spp=4))
    assert o4["stats"]["primary_rays"] == W * H * 4 and o4["stats"]["shadow_rays"] == o4["stats"]["hit_rays"] * L
    o1 = oracle.render(g.flat, g.params(W, H, L))
    assert np.array_equal(o1["hit_id"], oracle.render(g.flat, g.params(W, H, L, spp=1))["hit_id"])
    # an interior pixel of a flat face has the same hit in all four sub-samples -> nearly the 1-spp value
    same = (o4["hit_id"] == o1["hit_id"]) & (o1["hit_id"] >= 0)
    assert same.mean() > 0.05
    assert np.median(np.abs(o4["rgb_linear"][same] - o1["rgb_linear"][same])) < 1e-3
    with pytest.raises(RuntimeError):
        oracle.render(g.flat, g.params(W, H, L, spp=2))


def test_emitted_pixel_counts_of_the_survey(oracle):
    """SURVEY.md s8(c) lists, for renders made with the compiled reference during the survey, how many pixels
    sendRaysAndIntersectPointsColors emitted (non-black pixels, :518): an independent pin of the scene scripts, camera
    conventions and the hit / shading path.  (Its FNV hashes of the pixel stream are not reproduced here: the survey does
    not pin down the byte layout that was hashed; the pixel goldens of tests/golden/ play that role.)"""
    for name, W, H, want in (("cube", 256, 256, 41606), ("sphere", 256, 256, 3651),
                             ("ground_bunny", 600, 400, 118548), ("ground_bunny", 1920, 1080, 785274)):
        g = gu.GoldenScene(name)
        p = g.params(W, H, 1)
        p.background[0] = p.background[1] = p.background[2] = 0          # black = "not emitted"
        o = oracle.render(g.flat, p)
        assert int((o["rgb8"].reshape(-1, 3).max(1) > 0).sum()) == want, (name, W, H)


# ---- the device-pow mode (pow="device"): the kernels' pow in place of glibc powf, nothing else ----------------------------------
def test_device_pow_mode_of_the_leaf_functions(oracle, kat):
    """oracle.phong / oracle.tonemap with pow="device" differ from the default only on inputs where glibc powf and the device's pow
    (tonemap_ref.pow_device_ref) return different floats for what phong / tone1 hand to pow; the device-mode tone map is that pow
    of c / (c + r) bit for bit, at every test literal."""
    inp = kat["ph_in"]
    host, dev = oracle.phong(inp), oracle.phong(inp, pow="device")
    assert np.array_equal(bits(host), bits(kat["ph_rgb"]))                 # the default is still the reference's
    import gpu_frames as gf
    sx, sh = gf.phong_pow_inputs(inp)
    with np.errstate(all="ignore"):
        glibc = np.power(sx, sh)                                            # float32 power: the C library's powf
    differs = ~gf.same_f32(glibc, tr.pow_device_ref(sx, sh))
    changed = np.any(~gf.same_f32(host, dev), axis=1)
    assert not (changed & ~differs).any(), np.flatnonzero(changed & ~differs)[:5]
    for reinhard in tr.REINHARD:
        for gamma in tr.GAMMA:
            lin = tr.inputs(reinhard, gamma, n_random=6000)
            tone, q = oracle.tonemap(lin, reinhard, gamma, pow="device")
            want = tr.pow_device_ref(gf.tone_inputs(lin, reinhard), np.float32(gamma))
            assert np.array_equal(bits(tone)[~np.isnan(want)], bits(want)[~np.isnan(want)]) and np.isnan(tone[np.isnan(want)]).all(), (reinhard, gamma)
            assert np.array_equal(q, tr.quant_ref(tone))
    with pytest.raises(ValueError):
        oracle.tonemap(kat["tm_lin"], pow="glibc")


def _pixel_phong_rows(flat, p, y, x, hit, t, lights):
    """The 28-float phong input of every light at one pixel of a 1-spp frame without camera (o = 0, the reference's ray), the colour
    from the object or its texel as softShadow reads it (simple_raytracer.cpp:350-361)."""
    W, H = p.width, p.height
    d = np.array([np.float32(int(-W / 2) + x), np.float32(int(-H / 2) + y), np.float32(p.focal)], np.float32)
    obj = int(flat.tri_obj[hit])
    color = np.asarray(flat.obj_color, np.float32).reshape(-1, 3)[obj]
    tex = int(flat.tri_tex[hit]) if flat.tri_tex is not None else -1
    pts = np.asarray(flat.tri_points, np.float32).reshape(-1, 12)[hit]
    if tex >= 0:
        P = d * np.float32(t)
        bc_in = np.concatenate([pts, P]).astype(np.float32)[None]
        bc = oracle_bary(bc_in)[0]
        tc = np.asarray(flat.tri_texcoord, np.float32).reshape(-1, 6)[hit]
        tx = (bc[0] * tc[0] + bc[1] * tc[2]) + bc[2] * tc[4]
        ty = (bc[0] * tc[1] + bc[1] * tc[3]) + bc[2] * tc[5]
        w, h = int(flat.tex_w[tex]), int(flat.tex_h[tex])
        i = min(max((int(ty) * w + int(tx)) * 3, 0), w * h * 3 - 3)
        td = flat.tex_rgb[int(flat.tex_off[tex]) + i:][:3]
        color = td.astype(np.float32) / np.float32(255.0)
    mat = np.asarray(flat.obj_material, np.float32).reshape(-1, 3)[obj]
    rows = np.zeros((len(lights), 28), np.float32)
    rows[:, 3:6] = d; rows[:, 6:18] = pts; rows[:, 18:21] = lights; rows[:, 21:24] = color; rows[:, 24:27] = mat; rows[:, 27] = t
    return rows


def oracle_bary(inp):
    from oracle import pyoracle
    return pyoracle.barycentric(inp)


@pytest.mark.parametrize("name", gu.SCENES)
def test_device_pow_mode_changes_colours_only_through_pow(oracle, name):
    """pow="device" on every golden scene (its smallest render): hit ids, t and the ray counts are the default mode's bit for bit;
    an rgb_linear element changes only where the specular pow of one of the pixel's lights returns another float under the two
    functions (the pixel's phong inputs rebuilt and run through oracle.phong in both modes); rgb_tone is tone1 of the device pow on the
    frame's own rgb_linear."""
    g = gu.GoldenScene(name)
    W, H, L = min(g.renders, key=lambda r: (r[0] * r[1] * r[2], r))
    p = g.params(W, H, L)
    a, b = oracle.render(g.flat, p), oracle.render(g.flat, p, pow="device")
    assert np.array_equal(a["hit_id"], b["hit_id"]) and np.array_equal(bits(a["t"]), bits(b["t"]))
    for k in ("primary_rays", "hit_rays", "shadow_rays", "node_tests_primary", "node_tests_shadow", "tri_tests_primary", "tri_tests_shadow"):
        assert a["stats"][k] == b["stats"][k], k
    lights = abi.light_staircase(g.light, L)
    changed = np.argwhere(~np.all(bits(a["rgb_linear"]) == bits(b["rgb_linear"]), axis=-1))
    assert len(changed) <= max(2, int(1e-3 * W * H)), len(changed)
    for y, x in changed:
        rows = _pixel_phong_rows(g.flat, p, int(y), int(x), int(a["hit_id"][y, x]), a["t"][y, x], lights)
        by_light = ~np.all(bits(oracle.phong(rows)) == bits(oracle.phong(rows, pow="device")), axis=0)
        ch = bits(a["rgb_linear"][y, x]) != bits(b["rgb_linear"][y, x])
        assert not (ch & ~by_light).any(), (name, int(y), int(x))
    tone, q = oracle.tonemap(b["rgb_linear"], p.reinhard, p.gamma, pow="device")
    assert np.array_equal(bits(tone.reshape(b["rgb_tone"].shape)), bits(b["rgb_tone"]))
    assert np.array_equal(bits(oracle.tonemap(a["rgb_linear"], p.reinhard, p.gamma)[0].reshape(a["rgb_tone"].shape)), bits(a["rgb_tone"]))


# ---- the leaf functions beyond scene-scale inputs (tests/leaf_vectors.py) ------------------------------------------------------------
import os

import leaf_vectors as lv


def same(a, b):
    """the same bits, or NaN on both sides"""
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def leaf():
    return {"box": lv.box_families(), "tri": lv.tri_families(), "kat": np.load(os.path.join(gu.GOLDEN, "leaf_kat.npz"))}


def test_leaf_families_are_real_tests(oracle, leaf):
    """Every family holds at least 5 % passes and 5 % misses by the oracle, or is named "always pass" / "always miss" in the generator
    and is.  (A triangle family's "miss": no positive distance, see leaf_vectors._tri_always.)  Every scale and every family of the
    issue is there; arrays are finite unless the family says otherwise."""
    names = {f.name for f in leaf["box"]} | {f.name for f in leaf["tri"]}
    for base in ("primary", "shadow", "camera", "corner", "zero_dir", "hole1_x", "flat", "behind", "kat_rt", "kat_rt2", "w_pos", "w_neg",
                 "degenerate", "origin_on"):
        for e in lv.SCALES:
            assert f"{base}@2^{e}" in names, (base, e)
    for one in ("empty@2^0", "special_dir@2^0", "inf_box@2^0", "dir_sweep@2^0", "w_extreme@2^0"):
        assert one in names
    for f in leaf["box"]:
        assert f.nonfinite or f.tags["empty"] or (np.isfinite(f.ray).all() and np.isfinite(f.box).all()), f.name
        h = oracle.ray_aabb(f.ray, f.box).astype(bool)
        if f.always:
            assert f.always.startswith("pass:") and h.all(), (f.name, f.always, float(h.mean()))
        else:
            assert 0.05 <= h.mean() <= 0.95, (f.name, float(h.mean()))
    for f in leaf["tri"]:
        assert np.isfinite(f.ray).all() and np.isfinite(f.tri).all(), f.name
        t = oracle.ray_triangle(f.ray, f.tri)
        if f.always:
            assert f.always.startswith("miss:") and not (t > 0).any(), (f.name, f.always, int((t > 0).sum()))
        else:
            assert 0.05 <= (t >= 0).mean() <= 0.95, (f.name, float((t >= 0).mean()))
    # the special inputs are where they are meant to be
    d = {f.name: f for f in leaf["box"]}
    sp = d["special_dir@2^0"].ray[:, 3:]
    assert np.isnan(sp).any() and np.isinf(sp).any() and ((sp != 0) & (np.abs(sp) < 2.0 ** -126)).any()
    assert np.isinf(d["inf_box@2^0"].box).any()
    sw = np.abs(d["dir_sweep@2^0"].ray[:, 3:])
    assert ((sw > 0) & (sw < 2.0 ** -126)).any() and (sw > 2.0 ** 126).any() and np.isfinite(sw).all()
    z = d["zero_dir@2^0"]
    zero = z.ray[:, 3:] == 0
    both = zero & (z.box[:, :3] == z.ray[:, :3]) & (z.box[:, 3:] == z.ray[:, :3])
    assert np.signbit(z.ray[:, 3:][zero]).any() and (~np.signbit(z.ray[:, 3:][zero])).any()
    assert both[:, 0].any() and both[:, 1].any() and both[:, 2].any() and (zero.sum(1) == 3).any() and (z.ray[:, :3] != 0).any()
    for base in ("shadow", "camera", "corner"):
        assert (d[f"{base}@2^0"].ray[:, :3] != 0).any(), base


def test_leaf_hole1_family_has_boxes_the_other_axes_would_reject(oracle, leaf):
    """d.x = 0 and a box flat on x at the origin's x: the oracle passes every such box (NaN against everything is false), also where
    the y and z intervals alone -- what a min / max that drops NaN is left with -- are disjoint.  Those rows are the ones a filter
    that does not notice the NaN pair decides wrongly."""
    for f in leaf["box"]:
        if not f.name.startswith("hole1_x"):
            continue
        o, d = f.ray[:, :3].astype(np.float64), f.ray[:, 3:].astype(np.float64)
        assert np.all(d[:, 0] == 0) and np.all(f.box[:, 0] == f.ray[:, 0]) and np.all(f.box[:, 3] == f.ray[:, 0])
        with np.errstate(all="ignore"):
            q0, q1 = (f.box[:, 1:3] - o[:, 1:]) / d[:, 1:], (f.box[:, 4:6] - o[:, 1:]) / d[:, 1:]
        lo, hi = np.minimum(q0, q1), np.maximum(q0, q1)
        disjoint = (lo.max(1) > hi.min(1) * (1 + 1e-9)) & np.isfinite(lo).all(1) & np.isfinite(hi).all(1)
        assert disjoint.mean() > 0.2, (f.name, float(disjoint.mean()))
        assert oracle.ray_aabb(f.ray, f.box)[disjoint].all(), f.name


def test_leaf_ordinary_families_show_both_outcomes_under_emulation(oracle, leaf):
    """The families the device test requires decided AND ambiguous rows of (primary-, shadow-, camera-like and corner rays at scales
    2^-60 .. 2^60) have both when the filter is emulated in numpy with the reciprocal shifted by -1, 0 and +1 ulp, and the emulated
    filter is sound on them -- the reasoning behind that requirement, checked where no device is."""
    n = 0
    for f in leaf["box"]:
        if not f.ordinary:
            continue
        n += 1
        h = oracle.ray_aabb(f.ray, f.box).astype(bool)
        for ulp in (-1, 0, 1):
            p, amb = lv.filter_emulated(f.ray, f.box, ulp=ulp)
            assert amb.any() and (~amb).any(), (f.name, ulp)
            assert np.array_equal(p[~amb], h[~amb]), (f.name, ulp)
    assert n == 4 * len(lv.ORDINARY_SCALES)


def test_leaf_origin_rows_hit(oracle, leaf):
    """the rows of the origin-form test: all from the origin, with hits at finite t among them"""
    dirs, tris, _ = lv.origin0_rows(leaf["tri"])
    ray = np.zeros((dirs.shape[0], 6), np.float32); ray[:, 3:] = dirs
    t = oracle.ray_triangle(ray, tris)
    assert (np.isfinite(t) & (t > 0)).sum() > 2000 and (t == -np.inf).sum() > 2000 and np.isnan(t).any()


def _sub(fams):
    return [lv.Family(f.name, "tri", f.ray[lv.subsample(f.ray.shape[0])], tri=f.tri[lv.subsample(f.ray.shape[0])]) for f in fams]


def test_leaf_oracle_matches_recorded_reference(oracle, leaf):
    """Without the live reference: the oracle on the subsample of every family that tests/golden/leaf_kat.npz records from the compiled
    reference (make_golden.make_leaf_kat), bit for bit.  The inputs are recorded too: the generators must still draw them."""
    k = leaf["kat"]
    ray, box, names, rows = lv.recorded_rows(leaf["box"])
    assert np.array_equal(names, k["box_family"]) and np.array_equal(rows, k["box_row"])
    assert same(ray, k["box_ray"]).all() and same(box, k["box_box"]).all(), "the generators no longer draw the recorded inputs"
    want = np.unpackbits(k["box_hit_bits"])[: ray.shape[0]]
    got = oracle.ray_aabb(k["box_ray"], k["box_box"])
    assert np.array_equal(got, want), [str(x) for x in np.unique(names[got != want])]
    ray, tri, names, rows = lv.recorded_rows(leaf["tri"])
    assert np.array_equal(names, k["tri_family"]) and np.array_equal(rows, k["tri_row"])
    assert same(ray, k["tri_ray"]).all() and same(tri, k["tri_tri"]).all(), "the generators no longer draw the recorded inputs"
    bad = ~same(oracle.ray_triangle(k["tri_ray"], k["tri_tri"]), k["tri_t"])
    assert not bad.any(), [str(x) for x in np.unique(names[bad])]
    sub = _sub(leaf["tri"])
    assert same(oracle.barycentric(lv.bary_inputs(sub)), k["bc_uvw"]).all()
    assert same(oracle.interp_normal(lv.interp_inputs(sub)), k["in_out"]).all()
    assert os.path.getsize(os.path.join(gu.GOLDEN, "leaf_kat.npz")) < (1 << 20)


def test_leaf_oracle_matches_live_reference_on_every_family(oracle, leaf):
    """Where the compiled reference is present: ray_aabb, ray_triangle, barycentric and interp_normal of the oracle against the
    reference's own functions on EVERY row of every family, bit for bit (NaN equals NaN) -- the pin of the oracle over the range the
    device tests rely on."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not built (no reference sources here)")
    for f in leaf["box"]:
        assert np.array_equal(oracle.ray_aabb(f.ray, f.box), oracle.ref_kat_ray_aabb(f.ray, f.box)[0]), f.name
    for f in leaf["tri"]:
        assert same(oracle.ray_triangle(f.ray, f.tri), oracle.ref_kat_ray_triangle(f.ray, f.tri)).all(), f.name
        b = lv.bary_inputs([f])
        assert same(oracle.barycentric(b), oracle.ref_kat_barycentric(b)).all(), f.name
        q = lv.interp_inputs([f])
        assert same(oracle.interp_normal(q), oracle.ref_kat_interp_normal(q)).all(), f.name
    pts, _ = lv.record_points()
    b = np.concatenate([pts.reshape(-1, 12), pts[:, 0, :3] + np.float32(1.0)], 1)
    assert same(oracle.barycentric(b), oracle.ref_kat_barycentric(b)).all()
