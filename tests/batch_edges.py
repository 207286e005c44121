"""What tests/test_batch_edges_ref.py (CPU) and tests/test_gpu_batch_edges.py share: the calls that put srt_render_device_batch -- the
kernels no single render runs (k_trace_nq_batch's ROW_Z build, k_closest_hit_nq_batch, k_shadow_pk_batch, k_shade_tile_batch) and the
host rules around them (plan_frame's hold rule, BatchCollector, render_device_batch_impl in srt_hip.hip) -- on the frame edges and
light-count boundaries every single-frame chain is pinned at.  No GPU is needed to build any of this.

A call is a list of Frame(scene, params, pipeline, cls): the scene's name in test_gpu_modes.World, the frame's srt_params, the string
srt_scene_pipeline must give after the call and the class the batch holds the frame in (FUSED_CLASS, PK_CLASS or None = launched as it
comes).  The expectations are written down by hand in the builders below; hold_rule() restates plan_frame's decision from a frame's
facts, predict() walks a call with it, and tests/test_batch_edges_ref.py shows that the two agree on every frame of every table.

The bunny of ground_bunny fills every frame up to 65 pixels wide at the reference's focal length, and a hit's own object never shadows
it: with the scene's own light no shadow ray of such a frame is blocked.  BUNNY_LIGHTS therefore has two lights BELOW the ground slab
(y grows downwards: the slab is y = 120 .. 140 under x = -400 .. 400): from the second every shadow ray of the bunny's front crosses the
slab, from the third only the rays of points below the line where the ray to the light leaves the slab's edge at x = 400."""
import collections
import copy

import numpy as np

import gpu_frames as gf
import test_gpu_modes as tm
from simple_raytracer_amd import abi

Frame = collections.namedtuple("Frame", "scene params pipeline cls")
FUSED_CLASS, PK_CLASS = "fused", "pk"
FUSED_HELD, PK_HELD = tm.FUSED + " (batched)", tm.NQ_PK + " (batched)"
NOT_RENDERED = ""                   # srt_scene_pipeline of a fresh handle: a frame that owns no rows launches nothing and leaves it
SMOOTH, IN_FLIGHT, COUNT = abi.SRT_FLAG_SMOOTH_NORMALS, abi.SRT_FLAG_FRAMES_IN_FLIGHT, abi.SRT_FLAG_COUNT_WORK
V_FULL_GRID = 64                    # "0 in everything (batch hold-back ... included) but the tile spans": the rule holds such a frame
FRAME_TAB_MAX = 36                  # srt_kernels.h: frames per launch
XCD_BYTES = 32 << 20                # plan_frame: records beyond this get the XCD row deal
PACKET_OVERLAP = 150.0              # srt_hip.hip PACKET_OVERLAP_THRESHOLD
MID_OVERLAP = 14.0                  # plan_frame's few_nodes_mid

BUNNY = "ground_bunny"
SHINY = "ground_bunny shininess 64.5"
BIG = "main_nocats"                 # with vertex normals (World.flat): records over 32 MiB, overlap estimate 17
SOUP = "soup"
BUNNY_LIGHTS = ((300.0, -600.0, -100.0), (600.0, 400.0, 240.0), (1000.0, 300.0, 239.0))

# ---- sizes --------------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = tm.EDGE_SIZES
BOUNDARY_SIZES = ((64, 48), (9, 7))
BOUNDARY_L = tm.BOUNDARY_L
BIG_SIZES = ((90, 60), (9, 7))
BIG_L = (3, 8, 15, 16, 65)
BETWEEN_SIZE = (40, 24)
NO_ROWS = dict(width=33, height=9, block_rows=8, block_first=2, block_stride=3)
TABLE_SIZE = (9, 7)
TABLE_CALLS = {"36 fused": (36, 2), "37 fused": (37, 2), "1 fused": (1, 2), "37 pk": (37, 16)}      # name -> (frames, light samples)
NULLS_SIZE = (17, 9)
NULLS_L = (2, 16)


# ---- the scenes' facts, restated ----------------------------------------------------------------------------------------------------
def _area(a, b):
    d = b - a
    return np.where((d < 0).any(-1), 0.0, d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0])


def overlap_estimate(flat):
    """srt_hip.hip's overlap_estimate in float64: the objects, plus twice the area of every inner node's box over the area of the union
    of the root boxes.  (The library sums in the records' order: the two agree to rounding.)"""
    mn, mx = flat.node_min.reshape(-1, 3).astype(np.float64), flat.node_max.reshape(-1, 3).astype(np.float64)
    r = np.asarray(flat.obj_root).astype(np.int64)
    keep = _area(mn[r], mx[r]) > 0
    total = float(_area(mn[r][keep].min(0), mx[r][keep].max(0))) if keep.any() else 0.0
    if not total > 0:
        return 0.0
    inner = (np.asarray(flat.node_left) >= 0) | (np.asarray(flat.node_right) >= 0)
    return flat.n_objects + float((2.0 * _area(mn[inner], mx[inner])).sum()) / total


def record_bytes(flat):
    """srt_scene_device_bytes of a fresh handle: srt_hip.hip's record_list, row by row (an array of no elements is one element)."""
    nN, nT, nO = flat.n_nodes, flat.n_tris, flat.n_objects
    tex = flat.tri_tex is not None and bool((np.asarray(flat.tri_tex) >= 0).any())
    nX = 0 if flat.tex_w is None else len(flat.tex_w)
    rows = [(32, nN), (64, (nN - nO) // 2), (4, nO), (32, nO), (4, 8), (48, nT), (48, nT), (4, nT), (8, nO), (4, nO + 1), (4, nO * 3), (4, nO * 3),
            (4 if flat.tri_normals is not None and nT else 0, nT * 9), (4, nN)]
    if tex:
        size = np.asarray(flat.tex_w, np.uint64) * np.asarray(flat.tex_h, np.uint64) * np.uint64(3)
        rows += [(4, nT), (4, nT * 6), (1, int((np.asarray(flat.tex_off, np.uint64) + size).max())), (8, nX), (8, nX), (4, nX), (4, nX)]
    return sum(e * max(n, 1) for e, n in rows if e)


Facts = collections.namedtuple("Facts", "overlap bytes normals")


def scene_facts(flat):
    return Facts(overlap_estimate(flat), record_bytes(flat), flat.tri_normals is not None)


# ---- the hold rule, restated ---------------------------------------------------------------------------------------------------------
def local_size(p):
    """(cols, rows) of the buffers a call with these params writes."""
    rows, cols = gf.owned(p).shape
    return cols, rows


def variant(p):
    return (p.flags >> 8) & 0xff


def frame_ok(facts, p):
    """check_frame's preconditions (srt_hip.hip), for the shipped choice and the variants that map to it."""
    n = int(round(np.sqrt(p.spp)))
    return bool(p.width and p.height and p.block_rows and p.block_stride and (variant(p) == 0 or variant(p) == V_FULL_GRID) and
                (not p.n_lights or p.light_pos) and
                not (p.block_cols and (p.block_cols & 7 or p.block_rows & 7 or p.block_first >= p.block_stride)) and
                1 <= p.spp <= 4096 and n * n == p.spp and p.width * p.height < 1 << 31 and p.width * p.height * max(p.n_lights, 1) < 1 << 32 and
                (p.spp == 1 or 3 * local_size(p)[0] * local_size(p)[1] < 1 << 32) and (facts.normals or not p.flags & SMOOTH))


def hold_rule(overlap, nbytes, normals, L, camera, spp, count, size, held_size):
    """plan_frame for variant 0 (and 64, which is 0 to the rule): (class, pipeline) of a frame of a batch call from its facts -- the scene's
    overlap estimate, record bytes and whether it has vertex normals (frame_ok's business: the rule does not read it), the frame's light
    samples, camera mode, spp, counting flag and local size, and the size the call's held frames have so far (None: none held yet)."""
    del normals
    xcd_rows = nbytes > XCD_BYTES
    prefer_packet = overlap > PACKET_OVERLAP
    cam_nq = camera and not count and not prefer_packet and 1 <= L < 8 and not xcd_rows
    pk_closest = (camera and not cam_nq) or prefer_packet
    few_nodes_mid = not count and not camera and 8 <= L < 16 and overlap < MID_OVERLAP and not prefer_packet
    pk_shadow = L >= 8 and not few_nodes_mid
    fused = L >= 1 and not few_nodes_mid and not pk_shadow and not pk_closest
    fits = held_size is None or tuple(size) == tuple(held_size)
    holdable = fits and not count and spp == 1 and not pk_closest
    if holdable and ((not xcd_rows and not camera) if fused else pk_shadow):
        return (FUSED_CLASS, FUSED_HELD) if fused else (PK_CLASS, PK_HELD)
    first = "k_trace_nq" if fused else "k_closest_hit_pk" if pk_closest else "k_closest_hit_nq"
    return None, first + ("" if fused or not L else "+k_shadow_pk" if pk_shadow else "+k_shadow_nq") + "+k_shade_tile"


def predict(call, facts_of):
    """(class, pipeline) of every frame of a call in order, as BatchCollector sees them: the first held frame fixes the size, a frame that
    owns no rows never reaches the rule."""
    out, held_size = [], None
    for f in call:
        p, size = f.params, local_size(f.params)
        if size[1] == 0:
            out.append((None, NOT_RENDERED))
            continue
        fa = facts_of(f.scene)
        cls, pipe = hold_rule(fa.overlap, fa.bytes, fa.normals, p.n_lights, bool(p.ray_matrix), p.spp, bool(p.flags & COUNT), size, held_size)
        if cls and held_size is None:
            held_size = size
        out.append((cls, pipe))
    return out


def launches(call):
    """{class: [held, ...]}: the frames per launch of each held class, FRAME_TAB_MAX at a time."""
    out = {}
    for cls in (FUSED_CLASS, PK_CLASS):
        n = sum(1 for f in call if f.cls == cls)
        out[cls] = [min(FRAME_TAB_MAX, n - k) for k in range(0, n, FRAME_TAB_MAX)]
    return out


# ---- frames --------------------------------------------------------------------------------------------------------------------------
def shiny_flat(flat):
    """ground_bunny with every object's shininess 64.5: pow's general branch, so the library's int_shin is false for the scene."""
    f = copy.copy(flat)
    m = np.array(flat.obj_material, np.float32).reshape(-1, 3).copy()
    m[:, 2] = 64.5
    f.obj_material = np.ascontiguousarray(m.reshape(np.asarray(flat.obj_material).shape))
    return f


def prepare(world):
    """The scenes of the calls that tests/test_gpu_modes.World does not know by name."""
    if SHINY not in world.flats:
        flat, light = world.flat(BUNNY)
        world.flats[SHINY] = (shiny_flat(flat), light)
    return world


def own_light(world, scene, k, which=None):
    """Frame k's light: for the bunny scenes BUNNY_LIGHTS in turn (or the one named), for the others the scene's own; every frame a little
    off its base."""
    base = BUNNY_LIGHTS[k % 3 if which is None else which] if scene in (BUNNY, SHINY) else world.flat(scene)[1][:3]
    return np.asarray(base, np.float32) + np.array([2.0 * k, 0.0, -1.5 * k], np.float32)


def frame(world, scene, W, H, L, k, pipeline, cls, camera=False, flags=0, which=None, **kw):
    p = abi.make_params(W, H, abi.light_staircase(own_light(world, scene, k, which), L), ray_matrix=tm.camera_matrix() if camera else None, flags=flags, **kw)
    return Frame(scene, p, pipeline, cls)


def view_focal(W, H):
    """Calls 2 and 4 to 7 look at ground_bunny with the frame's longer side as the focal length (never below 8): the bunny, the slab under it
    with the bunny's shadow, and background."""
    return float(max(W, H, 8))


# ---- call 1: frame edges, both held classes --------------------------------------------------------------------------------------------
def edge_layouts(W, H):
    """tm.edge_layouts(W, H) that give a share with rows and columns."""
    out = []
    for kw in tm.edge_layouts(W, H):
        cols, rows = local_size(abi.make_params(W, H, np.zeros((0, 3), np.float32), **kw))
        if cols and rows:
            out.append(kw)
    return out


def other_size_layout(W, H, kw):
    """A share of the same frame whose local size differs from layout kw's.  The local size of a tile deal does not depend on
    block_first (every call writes all rows, ceil(ceil(W / block_cols) / stride) column blocks wide), so only a scanline share has
    another block_first of another size; elsewhere the frame is dealt another way."""
    held = local_size(abi.make_params(W, H, np.zeros((0, 3), np.float32), **kw))
    firsts = [dict(kw, block_first=b) for b in range(kw.get("block_stride", 1)) if not kw.get("block_cols")]
    for alt in firsts + [dict(block_rows=1, block_first=0, block_stride=2), dict(block_rows=8, block_cols=16, block_stride=3, block_first=0), {}]:
        size = local_size(abi.make_params(W, H, np.zeros((0, 3), np.float32), **alt))
        if size != held and size[0] and size[1]:
            return alt
    raise AssertionError((W, H, kw))


EDGE_LITERALS = (0, 3, 1, 0, 2, 1, 3)      # frame -> row of tm.LITERALS: rows 0, 1, 2 in the fused launch, 3, 0, 1 in the packet one, 3 for the frame of another size

# frame -> BUNNY_LIGHTS: the second frame of each class is lit from under the slab.  In a tile deal of a frame inside one block only ONE
# block_first owns pixels -- the second frame's, with the block_first values the deals of tm.edge_layouts start from
EDGE_LIGHTS = (0, 2, 1, 1, 2, 0, 0)


def edge_call(world, W, H, kw):
    """Three frames of L = 2 and three of L = 16 in turn, every frame with its own light and row of LITERALS; the second of each class with
    smooth normals, the third with the in-flight hint; a tile deal's frames take block_first, block_first + 1, ... (one local size);
    between them a frame of L = 2 of another local size."""
    def one(k, L, pipeline, cls, layout, flags):
        return frame(world, BUNNY, W, H, L, k, pipeline, cls, flags=flags, which=EDGE_LIGHTS[k], **tm.LITERALS[EDGE_LITERALS[k]], **layout)
    call = []
    for k in range(6):
        j, pk = k // 2, k % 2
        layout = dict(kw, block_first=(kw["block_first"] + j) % kw["block_stride"]) if kw.get("block_cols") else kw
        call.append(one(k, 16 if pk else 2, PK_HELD if pk else FUSED_HELD, PK_CLASS if pk else FUSED_CLASS, layout, (0, SMOOTH, IN_FLIGHT)[j]))
        if k == 2:
            call.append(one(6, 2, tm.FUSED, None, other_size_layout(W, H, kw), 0))
    return call


def edge_calls(world, W, H):
    return {str(kw): edge_call(world, W, H, kw) for kw in edge_layouts(W, H)}


# ---- call 2: light-count boundaries in one launch --------------------------------------------------------------------------------------
def boundary_expect(L):
    """ground_bunny's overlap estimate is below 14."""
    if L == 0:
        return tm.NQ_DARK, None
    if L < 8:
        return FUSED_HELD, FUSED_CLASS
    if L < 16:
        return tm.NQ_NQ, None
    return PK_HELD, PK_CLASS


def boundary_calls(world, W, H):
    fwd = [frame(world, BUNNY, W, H, L, k, *boundary_expect(L), focal=view_focal(W, H)) for k, L in enumerate(BOUNDARY_L)]
    return {"forward": fwd, "reversed": fwd[::-1]}


# ---- call 3: the held packet class below 16 samples, a scene over 32 MiB -----------------------------------------------------------------
def big_focal(W, H):
    """main_nocats is a room 70 wide whose near face is 25 away: 0.7 of the width shows the trees, the bunny and the walls beside them."""
    return 0.7 * W


def big_call(world, W, H):
    return [frame(world, BIG, W, H, L, k, *((tm.FUSED, None) if L < 8 else (PK_HELD, PK_CLASS)), focal=big_focal(W, H), flags=SMOOTH if k >= len(BIG_L) else 0)
            for k, L in enumerate(BIG_L + BIG_L)]


# ---- call 4: frames a batch must not hold, between frames it holds ----------------------------------------------------------------------
def between_calls(world):
    W, H = BETWEEN_SIZE
    kw = dict(focal=view_focal(W, H))
    call = [
        frame(world, BUNNY, W, H, 2, 0, FUSED_HELD, FUSED_CLASS, **kw),
        frame(world, BUNNY, W, H, 2, 1, tm.FUSED, None, camera=True, **kw),               # the camera build of the fused kernel
        frame(world, BUNNY, W, H, 2, 2, FUSED_HELD, FUSED_CLASS, **kw),
        frame(world, BUNNY, W, H, 2, 3, tm.FUSED, None, spp=4, **kw),
        frame(world, BUNNY, W, H, 2, 4, tm.FUSED, None, flags=COUNT, **kw),
        frame(world, SOUP, W, H, 2, 5, tm.PK_NQ, None),                                   # packet closest hit
        frame(world, BUNNY, W, H, 16, 6, PK_HELD, PK_CLASS, **kw),
        # variant 64 is variant 0 to plan_frame (variant_or_shipped) and only turns the tile spans off, which a batch never uses: the rule
        # holds the frame.  At 16 samples, so that the packet class of this call has a second member
        frame(world, BUNNY, W, H, 16, 7, PK_HELD, PK_CLASS, flags=V_FULL_GRID << 8, **kw),
        frame(world, BUNNY, NO_ROWS["width"], NO_ROWS["height"], 2, 8, NOT_RENDERED, None, **{k: v for k, v in NO_ROWS.items() if k.startswith("block")}),
        frame(world, BUNNY, W, H, 2, 9, FUSED_HELD, FUSED_CLASS, **kw),
    ]
    rest = call[:8] + call[9:]
    return {"in place": call, "first": [call[8]] + rest, "last": rest + [call[8]]}


# ---- call 5: table lengths at a ragged size ----------------------------------------------------------------------------------------------
def table_call(world, name):
    n, L = TABLE_CALLS[name]
    W, H = TABLE_SIZE
    return [frame(world, BUNNY, W, H, L, k, *boundary_expect(L), focal=view_focal(W, H)) for k in range(n)]


# ---- call 6: mixed shading kernel and NULL outputs ----------------------------------------------------------------------------------------
HIT, T, LIN, RGB8 = range(4)      # the output tables in srt_render_device_batch's order


def nulls_calls(world, L):
    """name -> (call, {frame: outputs passed as NULL}, tables passed as NULL).  Golden and shininess-64.5 handles in turn: the batch takes
    the general shading kernel for all of them."""
    W, H = NULLS_SIZE
    call = [frame(world, (BUNNY, SHINY)[k % 2], W, H, L, k, *boundary_expect(L), focal=view_focal(W, H)) for k in range(4)]
    return {"entries": (call, {1: (HIT, T), 2: (LIN,)}, ()), "t table": (call, {0: (LIN,), 3: (HIT,)}, (T,))}
