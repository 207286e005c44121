"""Every shipped kernel chain against the oracle where two features meet (-m gpu): the pipeline the dispatcher picks (light-count
bucket, overlap estimate, camera mode, XCD row deal, no lights) crossed pairwise with the frame layout (whole, scanline share, tile
deal), supersampling, smooth normals, the in-flight hint and non-default render literals; frames at the edges of the 8 x 8 tile;
the light counts where the pipeline or the shadow-word count changes; batch calls that split into several launches; the tone map
against float64.

Frames go through srt_render_device into pinned host buffers filled with sentinels and carrying one guard row: after every render
the padding of a tile deal (include/srt.h: "not written") and the guard row must still hold the sentinels.
Bars as in tests/test_gpu_parity.py: hit id and t bit for bit, pre-tone-map RGB within TOL_LINEAR (relative to the frame's
maximum), rgb8 <= 1 LSB on at most 1e-3 of the pixels, primary / hit / shadow ray counts equal.  Next to that every frame meets the
strict bar of tests/gpu_frames.compare_exact against the oracle run with the device's pow: colours bit for bit up to the residual of
the device pow's general branch, which srt_kat_pow explains."""
import copy

import numpy as np
import pytest

import golden_util as gu
import gpu_frames as gf
import tonemap_ref as tr
from simple_raytracer_amd import abi

pytestmark = pytest.mark.gpu

FUSED = "k_trace_nq+k_shade_tile"
NQ_NQ = "k_closest_hit_nq+k_shadow_nq+k_shade_tile"
NQ_PK = "k_closest_hit_nq+k_shadow_pk+k_shade_tile"
PK_NQ = "k_closest_hit_pk+k_shadow_nq+k_shade_tile"
PK_PK = "k_closest_hit_pk+k_shadow_pk+k_shade_tile"
NQ_DARK = "k_closest_hit_nq+k_shade_tile"
PK_DARK = "k_closest_hit_pk+k_shade_tile"
SHIPPED = {FUSED, NQ_NQ, NQ_PK, PK_NQ, PK_PK, NQ_DARK, PK_DARK}

# chain: (scene, light samples, camera mode, kernel variant, the pipeline srt_hip.hip's dispatcher must pick)
CHAINS = {
    "fused": ("ground_bunny", 3, False, 0, FUSED),
    "nq+nq": ("ground_bunny", 9, False, 0, NQ_NQ),            # 8..15 samples, overlap estimate < 14: samples cut over blockIdx.z
    "nq+pk mid": ("main_nocats", 9, False, 0, NQ_PK),         # 8..15 samples on a scene whose estimate is >= 14
    "nq+pk": ("ground_bunny", 16, False, 0, NQ_PK),           # 16+ samples
    "pk+nq": ("soup", 1, False, 0, PK_NQ),                    # overlap estimate > 150: packet closest hit
    "pk+pk": ("soup", 9, False, 0, PK_PK),
    "camera nq": ("ground_bunny", 3, True, 0, FUSED),         # camera build of the fused node-queue kernel
    "camera pk": ("ground_bunny", 9, True, 0, PK_PK),         # camera mode on the packet closest-hit kernel
    "xcd fused": ("ground_bunny", 3, False, 18, FUSED),       # whole tile rows per XCD (variant 18 forces it; otherwise only records over 32 MiB)
    "nq dark": ("ground_bunny", 0, False, 0, NQ_DARK),
    "pk dark": ("soup", 0, False, 0, PK_DARK),
    "camera dark": ("ground_bunny", 0, True, 0, PK_DARK),
}

LITERALS = (
    {},                                                                                   # the reference's
    dict(focal=150.0, shadow_div=1.0, reinhard=0.2, gamma=2.0, background=(0, 0, 0)),    # gamma 2: pow's square-and-multiply branch
    dict(focal=1000.0, shadow_div=2.5, reinhard=4.0, gamma=0.4545, background=(255, 0, 7)),
    dict(focal=37.0, gamma=1.0),
)
LAYOUTS = (
    ("whole", {}),
    ("share", dict(block_rows=8, block_first=1, block_stride=3)),
    ("tile", dict(block_rows=8, block_cols=16, block_stride=3, block_first=2)),     # on widths that are no multiple of 16
)
# (literals, layout, spp > 1, smooth normals, in-flight hint): every pair of values of any two factors occurs in some row
PAIRWISE = ((0, 0, 0, 0, 0), (0, 1, 1, 1, 0), (0, 2, 0, 0, 1), (1, 0, 1, 0, 0), (1, 1, 0, 1, 0), (1, 2, 1, 0, 1),
            (2, 0, 0, 1, 0), (2, 1, 1, 0, 0), (2, 2, 0, 1, 1), (3, 0, 1, 1, 1), (3, 1, 0, 0, 1), (3, 2, 1, 1, 0))
MATRIX = [(ch, i, (lit, lay, 4 if s else 1, sm, fl)) for ch in CHAINS for i, (lit, lay, s, sm, fl) in enumerate(PAIRWISE)]
MATRIX.append(("nq+pk", len(PAIRWISE), (2, 2, 9, 1, 0)))      # 3 x 3 sub-frames: the heavy-quadrant lists carry over nine times

REACHED = {}           # pipeline string -> chains of the matrix that reached it


def camera_matrix():
    """Yaw of 4 degrees, origin (3, -2, 10): column-major like glm::mat4."""
    a = np.radians(4.0)
    c, s = np.cos(a), np.sin(a)
    return np.array([c, 0, -s, 0, 0, 1, 0, 0, s, 0, c, 0, 3.0, -2.0, 10.0, 1.0], np.float32)


def with_normals(flat):
    """Vertex normals pointing away from each object's centroid (as test_smooth_normal_mode)."""
    f = copy.copy(flat)
    P = f.tri_points[..., :3]
    centre = np.zeros_like(P)
    for obj in range(f.n_objects):
        m = f.tri_obj == obj
        if m.any():
            centre[m] = P[m].reshape(-1, 3).mean(0)
    nrm = P - centre
    nrm /= np.maximum(np.linalg.norm(nrm, axis=2, keepdims=True), 1e-6)
    f.tri_normals = np.ascontiguousarray(nrm.reshape(-1, 9), np.float32)
    return f


def shifted(flat, dx):
    """The scene moved along x (points and boxes in float32: rounding is monotonic, so every box still holds its triangles)."""
    f = copy.copy(flat)
    o = np.array([dx, 0.0, 0.0], np.float32)
    f.node_min = flat.node_min + o
    f.node_max = flat.node_max + o
    tp = flat.tri_points.copy()
    tp[..., :3] += o
    f.tri_points = tp
    return f


class World:
    """Device scenes and oracle results, built once per module."""

    def __init__(self, srt):
        self.srt, self.flats, self.scenes, self.oracle_cache = srt, {}, {}, {}

    def flat(self, name):
        if name not in self.flats:
            if name == "soup":
                import scenes
                from simple_raytracer_amd import build, host
                build.build_host()
                recipe, meshes = scenes.soup(200000)
                # moved 12 units so that the central ray meets a triangle (1 x 1 and single-row frames hit geometry)
                self.flats[name] = (with_normals(shifted(host.build_flat_scene(recipe, meshes), -12.0)), np.array(recipe.light[:3], np.float32))
            else:
                g = gu.GoldenScene(name)
                self.flats[name] = (with_normals(g.flat), g.light)
        return self.flats[name]

    def ds(self, name):
        if name not in self.scenes:
            self.scenes[name] = self.srt.DeviceScene(self.flat(name)[0])
        return self.scenes[name]

    def params(self, name, W, H, L, camera=False, flags=0, **kw):
        return abi.make_params(W, H, abi.light_staircase(self.flat(name)[1], L), ray_matrix=camera_matrix() if camera else None, flags=flags, **kw)

    def oracle(self, oracle, name, p, pow="host"):
        """The oracle's frame; cached by everything the oracle reads (the hint and the variant bits are not among it)."""
        key = (name, pow, tuple(getattr(p, k) for k in ("width", "height", "block_rows", "block_first", "block_stride", "block_cols", "focal",
                                                    "n_lights", "shadow_div", "reinhard", "gamma", "spp")),
               bytes(p.background), p.flags & abi.SRT_FLAG_SMOOTH_NORMALS, p._lights.tobytes(), getattr(p, "_ray_matrix", np.zeros(0)).tobytes())
        if key not in self.oracle_cache:
            self.oracle_cache[key] = oracle.render(self.flat(name)[0], p, pow=pow)
        return self.oracle_cache[key]

    def check(self, srt, oracle, name, o, p, what):
        """Both bars: compare against the oracle as the reference computes pow, compare_exact against the device-mode oracle."""
        own = gf.owned(p)
        c = self.oracle(oracle, name, p)
        gf.compare(o, c, own, what)
        gf.compare_exact(srt, o, self.oracle(oracle, name, p, pow="device"), own, self.flat(name)[0], p, what)
        return c


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


@pytest.fixture(scope="module")
def world(srt):
    w = World(srt)
    yield w
    for ds in w.scenes.values():
        ds.close()


def chain_params(world, chain, W, H, flags=0, **kw):
    scene, L, cam, variant, _ = CHAINS[chain]
    return world.params(scene, W, H, L, camera=cam, flags=flags | (variant << 8), **kw)


def render_check(srt, oracle, world, chain, p, what):
    scene, _, _, _, want = CHAINS[chain]
    o, pipe = gf.render_pinned(srt, world.ds(scene), p)
    assert pipe == want, (what, pipe)
    c = world.check(srt, oracle, scene, o, p, what)
    return o, c


# ---- 1. pipeline x mode matrix -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain,i,row", MATRIX, ids=[f"{ch}-{i}" for ch, i, _ in MATRIX])
def test_mode_matrix(srt, oracle, world, chain, i, row):
    lit, lay, spp, smooth, in_flight = row
    W, H = (62, 46) if CHAINS[chain][0] == "soup" else (90, 60)
    flags = (abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0) | (abi.SRT_FLAG_FRAMES_IN_FLIGHT if in_flight else 0)
    p = chain_params(world, chain, W, H, flags=flags, spp=spp, **LITERALS[lit], **LAYOUTS[lay][1])
    what = f"{chain} literals {lit} {LAYOUTS[lay][0]} spp {spp} smooth {smooth} in-flight {in_flight}"
    o, c = render_check(srt, oracle, world, chain, p, what)
    REACHED.setdefault(CHAINS[chain][4], set()).add(chain)
    assert (c["hit_id"] >= 0).sum() > 10, what


# ---- 2. frame edges ------------------------------------------------------------------------------------------------------------
EDGE_SIZES = ((1, 1), (1, 40), (40, 1), (3, 2), (7, 9), (8, 8), (9, 7), (16, 17), (65, 3))
EDGE_CHAINS = ("fused", "nq+nq", "nq+pk", "pk+nq", "camera nq", "camera pk")


def edge_layouts(W, H):
    out = [{}, dict(block_rows=8, block_cols=16, block_stride=3, block_first=2), dict(block_rows=8, block_cols=8, block_stride=2, block_first=1)]
    if H >= 2:
        out.append(dict(block_rows=1, block_first=1, block_stride=2))      # every other row
    if H > 8:
        out.append(dict(block_rows=8, block_first=1, block_stride=3))
    return out


@pytest.mark.parametrize("chain", EDGE_CHAINS)
@pytest.mark.parametrize("W,H", EDGE_SIZES)
def test_frame_edges(srt, oracle, world, chain, W, H):
    """Frames narrower or shorter than one 8 x 8 tile, single rows and columns, tile deals in which a call owns only padding in some
    rows (widths below block_cols x stride), supersampled tile deals."""
    for kw in edge_layouts(W, H):
        for spp in ((1, 4) if kw.get("block_cols") else (1,)):
            p = chain_params(world, chain, W, H, spp=spp, **kw)
            o, c = render_check(srt, oracle, world, chain, p, f"{chain} {W}x{H} {kw} spp {spp}")
            if not kw and (W == 1 or H == 1):
                assert (c["hit_id"] >= 0).any(), f"{chain} {W}x{H}: the frame should hit geometry"


@pytest.mark.parametrize("chain", ("fused", "nq+pk", "pk+nq", "camera pk"))
def test_call_that_owns_no_rows(srt, oracle, world, chain):
    """A scanline share that owns no block of the frame: SRT_OK, nothing written; srt_sync then reports zero rays on an idle handle,
    and the statistics of earlier pending work are kept."""
    scene = CHAINS[chain][0]
    ds = world.ds(scene)
    L = srt.load()
    p0 = chain_params(world, chain, 33, 9, block_rows=8, block_first=2, block_stride=3)
    assert ds.rows(p0) == 0
    ds.sync()
    empty = gf.PinnedFrame(L, 0, ds.cols(p0))
    frame = None
    try:
        ds.render_device(p0, 0, *empty.ptrs)
        st = ds.sync()
        empty.check_untouched(gf.owned(p0), "no rows")
        for k in ("primary_rays", "hit_rays", "shadow_rays", "rows"):
            assert st[k] == 0, (k, st)
        o = ds.render(p0)                                              # srt_render too
        assert o["hit_id"].shape == (0, 33) and o["stats"]["primary_rays"] == 0
        # pending work: its statistics survive a call that owns no rows
        p = chain_params(world, chain, 48, 32)
        frame = gf.PinnedFrame(L, ds.rows(p), ds.cols(p))
        ds.render_device(p, 0, *frame.ptrs)
        ds.render_device(p0, 0, *empty.ptrs)
        st = ds.sync()
        frame.check_untouched(gf.owned(p), "pending frame")
        empty.check_untouched(gf.owned(p0), "no rows behind a pending frame")
        out = frame.out()
        out["stats"] = st
        world.check(srt, oracle, scene, out, p, f"{chain}: pending frame")
        assert st["hit_rays"] > 0
    finally:
        empty.free()
        if frame is not None:
            frame.free()


# ---- 3. light-count boundaries -------------------------------------------------------------------------------------------------
BOUNDARY_L = (0, 1, 7, 8, 15, 16, 63, 64, 65, 128, 129)


def bucket_pipeline(L, overlap):
    """srt_hip.hip's dispatcher for the shipped pipeline, no camera, scenes without the packet preference."""
    if L == 0:
        return NQ_DARK
    if L < 8:
        return FUSED
    if L < 16 and overlap < 14.0:
        return NQ_NQ
    return NQ_PK


@pytest.mark.parametrize("name", ("ground_bunny", "cubes4_a0"))
@pytest.mark.parametrize("L", BOUNDARY_L)
def test_light_count_boundaries(srt, oracle, world, name, L):
    """The light counts where the pipeline changes (7/8, 15/16) and where a pixel's shadow bits take another 64-bit word (64/65,
    128/129), whole frames and a tile deal."""
    ds = world.ds(name)
    assert ds.overlap_estimate < 150.0
    for kw in ({}, dict(block_rows=8, block_cols=16, block_stride=3, block_first=1)):
        p = world.params(name, 64, 48, L, **kw)
        o, pipe = gf.render_pinned(srt, ds, p)
        assert pipe == bucket_pipeline(L, ds.overlap_estimate), (L, pipe)
        c = world.check(srt, oracle, name, o, p, f"{name} L {L} {kw}")
        assert (c["hit_id"] >= 0).sum() > 100


# ---- 4. batch calls that split into several launches ---------------------------------------------------------------------------
def batch_frames(world, n_fused, n_pk, extras):
    """(scene, params, pipeline) per frame: 48 x 32 frames of two scenes, every frame with its own light."""
    frames = []
    for k in range(n_fused):
        name = ("ground_bunny", "texquad")[k % 2]
        light = world.flat(name)[1].copy(); light[0] += 9.0 * k
        frames.append((name, abi.make_params(48, 32, abi.light_staircase(light, 1 + k % 7)), FUSED + " (batched)"))
    for k in range(n_pk):
        name = ("ground_bunny", "texquad")[k % 2]
        light = world.flat(name)[1].copy(); light[1] -= 7.0 * k
        frames.append((name, abi.make_params(48, 32, abi.light_staircase(light, 16 + k % 5)), NQ_PK + " (batched)"))
    if extras:
        # tile deals of a 140-pixel-wide frame: 48 local columns x 32 rows, the shape of the whole frames -- they join the held
        # groups, with block_first 0, 1, 2 in one launch; the last tile column is partly padding
        for first in range(3):
            for L, pipe in ((2, FUSED), (16, NQ_PK)):
                light = world.flat("ground_bunny")[1].copy(); light[2] += 5.0 * first + L
                p = abi.make_params(140, 32, abi.light_staircase(light, L), block_rows=8, block_cols=16, block_stride=3, block_first=first)
                frames.append(("ground_bunny", p, pipe + " (batched)"))
        frames.append(("texquad", abi.make_params(48, 32, abi.light_staircase(world.flat("texquad")[1], 2), spp=4), FUSED))
        frames.append(("ground_bunny", world.params("ground_bunny", 48, 32, 2, camera=True), FUSED))
    return frames


@pytest.mark.parametrize("n_fused,n_pk,extras", [(36, 0, False), (37, 37, False), (70, 0, True)], ids=["36", "37+37", "73+extras"])
def test_batch_splits_into_launches(srt, world, n_fused, n_pk, extras):
    """srt_render_device_batch launches the held frames FRAME_TAB_MAX (36) at a time: 36, 37 and 73 frames of the fused group, 37 of
    the 8+-sample group, tile deals with different block_first in the same launch, a supersampled and a camera frame launched on
    their own.  Every frame is its single render bit for bit, with its own statistics; padding and guard rows keep the sentinels."""
    frames = batch_frames(world, n_fused, n_pk, extras)
    if extras:
        assert sum(1 for f in frames if f[2] == FUSED + " (batched)") == 73
    L = srt.load()
    solo = {name: world.ds(name) for name in ("ground_bunny", "texquad")}
    first = {name: srt.DeviceScene(world.flat(name)[0]) for name in solo}
    handles = [first[name].share() for name, _, _ in frames]
    for h in first.values():
        h.close()
    bufs = [gf.PinnedFrame(L, h.rows(p), h.cols(p)) for h, (_, p, _) in zip(handles, frames)]
    try:
        fb = srt.FrameBatch(handles, [p for _, p, _ in frames], *[[b.ptrs[k] for b in bufs] for k in range(4)])
        fb.render()
        stats = [h.sync() for h in handles]
        for k, ((name, p, pipe), h, b, st) in enumerate(zip(frames, handles, bufs, stats)):
            assert h.pipeline == pipe, (k, h.pipeline)
            own = gf.owned(p)
            b.check_untouched(own, f"frame {k}")
            got = b.out()
            want = solo[name].render(p)
            live = own >= 0
            assert np.array_equal(got["hit_id"][live], want["hit_id"][live]), k
            assert np.array_equal(gf.bits(got["t"][live]), gf.bits(want["t"][live])), k
            assert np.array_equal(gf.bits(got["rgb_linear"][live]), gf.bits(want["rgb_linear"][live])), k
            assert np.array_equal(got["rgb8"][live], want["rgb8"][live]), k
            for key in ("primary_rays", "hit_rays", "shadow_rays", "rows"):
                assert st[key] == want["stats"][key], (k, key)
            assert st["hit_rays"] > 0, k
    finally:
        for h in handles:
            h.close()
        for b in bufs:
            b.free()


# ---- 5. tone map against float64 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reinhard", tr.REINHARD)
@pytest.mark.parametrize("gamma", tr.GAMMA)
def test_device_tonemap_against_float64(srt, reinhard, gamma):
    """srt_kat_tonemap (tone1 / quant1 on the device) with non-default literals against the float64 restatement: bitwise on all but
    1e-5 of the inputs and within 1 ulp on the rest; q is exactly the quantiser of the device's own tone."""
    lin = tr.inputs(reinhard, gamma)
    tone, q = srt.kat_tonemap(lin, reinhard, gamma)
    ref = tr.tone_ref(lin, reinhard, gamma)
    d = tr.ulp_diff(tone, ref)
    assert d.max() <= 1, f"{int((d > 1).sum())} tones differ by more than 1 ulp, e.g. lin {lin.reshape(-1)[np.argmax(d.reshape(-1))]}"
    assert (d > 0).sum() <= int(1e-5 * d.size), int((d > 0).sum())
    assert np.array_equal(q, tr.quant_ref(tone))


def test_device_pow_at_its_cutoffs(srt):
    """pow_like_host on either side of the bounds of its fast path (x = 1e-30 and 1e30, |y| = 1e4) against float64: the library call
    and the fast path meet without a seam."""
    steps = np.arange(-40, 41, dtype=np.int32)
    xs = [(np.full(steps.size, v, np.float32).view(np.int32) + steps).view(np.float32) for v in (1e-30, 1e30, 1e-4, 0.5)]
    x = np.concatenate(xs)
    ys = np.array(list(tr.GAMMA) + [0.5, 3.0, 9999.0, 1e4, -9999.0, -1e4, -1.1, -2.0], np.float32)
    X = np.repeat(x, ys.size)
    Y = np.tile(ys, x.size)
    fast, _ = srt.kat_pow(X, Y)
    with np.errstate(all="ignore"):
        ref = np.power(X.astype(np.float64), Y.astype(np.float64)).astype(np.float32)
    d = tr.ulp_diff(fast, ref)
    assert d.max() <= 1, (X[np.argmax(d)], Y[np.argmax(d)], fast[np.argmax(d)], ref[np.argmax(d)])
    assert (d > 0).sum() <= max(1, int(1e-5 * d.size))


# ---- 6. the shading arithmetic, bit for bit ---------------------------------------------------------------------------------------
# Materials, colours, shadow divisors, light counts and supersampling that move the colours and nothing else, each through every
# shipped chain and checked with compare_exact only: a reordered sum, a reciprocal for a divide or a contracted multiply-add in the
# shading path changes a few ulp, which the 1e-4 bar of compare cannot see.
SHADING = {
    **{f"shininess {s:g}": dict(material=(0.2, 0.5, s)) for s in (1.0, 2.0, 15.0, 63.0, 64.0, 65.0, 64.5, 0.5, 0.0)},   # integer path edges; pow(0, 0)
    **{f"shadow_div {d:g}": dict(shadow_div=d) for d in (2.0, 3.0, 0.7)},
    "ka ks 0": dict(material=(0.0, 0.0, 15.0)),
    "ka ks 1": dict(material=(1.0, 1.0, 15.0)),
    "ka ks above 1": dict(material=(2.5, 3.75, 7.0)),
    "ka 0 ks above 1 shininess 64.5": dict(material=(0.0, 1.7, 64.5)),
    "colour 0": dict(color=(0.0, 0.0, 0.0)),
    "colour above 1": dict(color=(1.75, 0.0, 3.2), material=(1.3, 0.25, 33.0)),
    **{f"lights {n}": dict(lights=n) for n in (63, 64, 65, 128, 129)},      # where a kernel could split the light sum into groups
    "spp 4": dict(spp=4, material=(0.2, 0.5, 2.5)),
    "spp 4 smooth": dict(spp=4, smooth=True),
    "spp 16 smooth": dict(spp=16, smooth=True, material=(0.4, 1.5, 64.5)),
}


def shaded_flat(flat, case):
    """The chain's scene with every object's colour and / or material replaced (textured triangles keep their texels)."""
    f = copy.copy(flat)
    if "material" in case:
        f.obj_material = np.ascontiguousarray(np.tile(np.asarray(case["material"], np.float32), (f.n_objects, 1)))
    if "color" in case:
        f.obj_color = np.ascontiguousarray(np.tile(np.asarray(case["color"], np.float32), (f.n_objects, 1)))
    return f


@pytest.mark.parametrize("case", list(SHADING))
def test_shading_arithmetic_bitwise(srt, oracle, world, case):
    """One shading case through all twelve chains (camera mode, the XCD row deal and the unlit kernels included), 64 x 48 frames (the
    light-count cases move the chain to the pipeline of that count).  Every frame is the device-mode oracle's, bit for bit up to the
    residual of pow's general branch."""
    kw = SHADING[case]
    flats, scenes = {}, {}
    try:
        for chain, (scene, L, cam, variant, want) in CHAINS.items():
            if scene not in scenes:
                flats[scene] = shaded_flat(world.flat(scene)[0], kw)
                scenes[scene] = srt.DeviceScene(flats[scene])
            n = kw.get("lights", L)
            p = world.params(scene, 64, 48, n, camera=cam, flags=(variant << 8) | (abi.SRT_FLAG_SMOOTH_NORMALS if kw.get("smooth") else 0),
                             spp=kw.get("spp", 1), shadow_div=kw.get("shadow_div", 5.0))
            what = f"{case}: {chain}"
            o, pipe = gf.render_pinned(srt, scenes[scene], p)
            assert pipe == want or "lights" in kw, (what, pipe)
            c = oracle.render(flats[scene], p, pow="device")
            gf.compare_exact(srt, o, c, gf.owned(p), flats[scene], p, what)
            assert (c["hit_id"] >= 0).sum() > 10, what
    finally:
        for ds in scenes.values():
            ds.close()


# ---- 7. limits -----------------------------------------------------------------------------------------------------------------
def test_supersampled_frame_beyond_the_accumulation_index_is_refused(srt, world):
    """spp > 1 accumulates 3 floats per pixel under a 32-bit index: 40000 x 40000 at spp = 4 is refused with SRT_ERR_LIMIT before
    anything is allocated or launched, by srt_render, srt_render_device and the batch call."""
    ds = world.ds("cubes4_a0")
    p = world.params("cubes4_a0", 40000, 40000, 1, spp=4)
    for call in (lambda: ds.render(p), lambda: ds.render_device(p), lambda: srt.FrameBatch([ds], [p]).render()):
        with pytest.raises(srt.SrtError) as e:
            call()
        assert e.value.code == abi.SRT_ERR_LIMIT


# ---- the matrix reached every chain (keep this test last in the module) ---------------------------------------------------------
def test_matrix_reached_every_chain(srt, oracle, world):
    for chain, (_, _, _, _, want) in CHAINS.items():
        if chain not in REACHED.get(want, set()):         # (a run that selected only some matrix cases)
            W, H = (62, 46) if CHAINS[chain][0] == "soup" else (90, 60)
            render_check(srt, oracle, world, chain, chain_params(world, chain, W, H), chain)
            REACHED.setdefault(want, set()).add(chain)
    assert set(REACHED) >= SHIPPED, sorted(SHIPPED - set(REACHED))
    assert all(ch in REACHED[want] for ch, (_, _, _, _, want) in CHAINS.items())
