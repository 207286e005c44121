"""What tests/test_edge_frames_ref.py (CPU), tests/test_gpu_trace_edges.py and tests/trace_edges_graph_case.py share: the frame shapes, views
and scenes that put the trace kernels of frames in flight (k_trace_nq_whole8_spans, k_trace_nq_wave8_spans, k_trace_nq_half8_spans,
srt_kernels.h) on the edges of their index arithmetic.  No GPU is needed to build any of this.

A workgroup of the one-wave kernels is one wave that owns 8 x 4 pixels; its grid row is padded to groups of eight tiles and doubled
(blocks 16g .. 16g + 7 are the upper halves of tiles 8g .. 8g + 7, the next eight their lower halves), a lower half with no live row leaves
before it touches anything (by * 8 + wave * 4 >= rows), and a wave tests its own roots while the scene has at most 32 objects, six objects
at a time (384 queue entries / (2 * 32 rays)).  SHAPES cuts the frame at every place that arithmetic names; object_grid(n) puts the object
count on each side of every bound it names; offset_scene() starts a span at a tile that is no multiple of eight and carries it over a
group boundary."""
import types

import numpy as np

import golden_util as gu
import scenes
import wave8_scenes as w8
from simple_raytracer_amd import abi

IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
LIGHTS = (1, 4, 5, 7)      # 1 and 4: the one-wave workgroups (the whole-frame kernels under variant 0); 5 and 7: variant 0 keeps two waves a tile

SHAPES = [
    # smaller than a half tile or a tile: 15 of the 16 workgroups of a padded grid row leave, and so does the lower half where rows <= 4
    (1, 1),        # one pixel
    (1, 40),       # one column: five tile rows of one live pixel column
    (40, 1),       # one row: five tiles, every lower half dead, the upper halves one row deep
    (3, 2),        # less than a half tile both ways
    (7, 3),        # one pixel short of a tile's width, inside the upper half
    (8, 4),        # exactly one half tile: rows == 4, the lower half's first row is the first dead one
    (8, 5),        # one row into the lower half
    # the last tile row cut at every remainder: one tile row ...
    (9, 1),        # H % 8 == 1, two tiles across (the second one pixel wide)
    (9, 2),        # H % 8 == 2
    (9, 3),        # H % 8 == 3
    (9, 7),        # H % 8 == 7: the lower half is cut one row short
    # ... and several (24 = three whole tiles across)
    (24, 33),      # H % 8 == 1 under four whole tile rows: the upper wave partly live, the lower wave dead
    (24, 34),      # H % 8 == 2
    (24, 35),      # H % 8 == 3
    (24, 39),      # H % 8 == 7
    # widths at the group of eight tiles, and the right-hand remainders not yet seen
    (63, 9),       # 8 tiles exactly (one group, no padding), W % 8 == 7
    (65, 3),       # 9 tiles: a second group that is one live tile and seven of padding
    (65, 12),      # 9 tiles, two tile rows, H % 8 == 4
    (121, 10),     # 16 tiles: two full groups, W % 8 == 1
    (129, 9),      # 17 tiles: three groups, the third nearly all padding
    (131, 11),     # W % 8 == 3
    (134, 6),      # W % 8 == 6
]
GOLDEN = ("cube_ground", "cubes4_a40")
# cubes4_a40 is four cubes around the z axis that leave the slab |y| < 5 free.  A frame of one row has j0 = int(-0.5) = 0: every ray
# lies in the plane y = 0, whatever the focal length, and hits nothing.  These frames are rendered all the same -- no ray passes a root
# box, the table keeps its one tile -- and tests/test_edge_frames_ref.py asserts that they are the only views without a hit.
NO_HIT_POSSIBLE = {("cubes4_a40", (1, 1)), ("cubes4_a40", (40, 1)), ("cubes4_a40", (9, 1))}


def edge_focal(name, W, H):
    """The focal length (in pixels) of the view of a golden scene at an edge shape: the frame's longer side, so that it spans +-0.5 in
    i / focal and the scenes -- cube_ground's cube at i / focal in -0.48 .. 0.16 over a ground slab, the four cubes within +-0.34 -- have
    background beside them; never below 8, where a frame of two or three rows would look past the cubes.  The four cubes leave |y| < 5
    free at z = 76 .. 124: a wide frame of few rows looks into that gap unless j / focal reaches 5 / 76, so there the focal length is at
    most six times the frame's half height."""
    f = max(W, H, 8)
    if name == "cubes4_a40":
        f = max(8, min(f, 6 * (H // 2)))
    return float(f)


def edge_view(name, W, H):
    """params(L, flags=0) of golden scene `name` at W x H."""
    g = gu.GoldenScene(name)
    focal = edge_focal(name, W, H)
    return lambda L, flags=0: g.params(W, H, L, focal=focal, flags=flags)


# ---- off-centre spans ---------------------------------------------------------------------------------------------------------------
OFFSET_FOCAL = 100.0
OFFSET_LIGHT = (20.0, -3.0, 0.0)
OFFSET_SHAPES = [(121, 10), (129, 9), (131, 11), (134, 6)]      # the shapes of 16 tiles or more
# (x0, n) of tile row 0's span.  The wall is x = -14.5 .. 34.5 at z = focal, so a unit is a pixel: columns x - i0, i0 = int(-W / 2) =
# -60, -64, -65, -67.  Hits on columns -14 - i0 .. 34 - i0 = 46..94, 50..98, 51..99, 53..101, and the table's pixel of margin stays in
# the same tiles: 5..11, 6..12, 6..12, 6..12.
OFFSET_SPANS = {(121, 10): (5, 7), (129, 9): (6, 7), (131, 11): (6, 7), (134, 6): (6, 7)}


def offset_scene():
    """(flat scene, light): a wall in the plane z = 100 and a chip in front of it that shadows it, both well inside the wall's columns."""
    from simple_raytracer_amd import host
    r = scenes.Recipe()
    meshes = {"wall": w8.rect(100.0, -14.5, -2.5, 34.5, 4.5), "chip": w8.rect(80.0, 0.0, -1.5, 10.0, 2.0, 3)}
    for k, name in enumerate(meshes):
        r.load(f"{name}.obj", name)
        r.color(f"{name}.obj", scenes.SOUP_PALETTE[k])
        r.bvh(f"{name}.obj")
    r.light = OFFSET_LIGHT
    flat = host.build_flat_scene(r, meshes)
    assert flat.n_objects == 2
    return flat, r.light


def offset_view(W, H):
    assert (W, H) in OFFSET_SPANS
    return lambda L, flags=0: abi.make_params(W, H, abi.light_staircase(OFFSET_LIGHT, L), focal=OFFSET_FOCAL, flags=flags)


# ---- object counts ------------------------------------------------------------------------------------------------------------------
# 6 | 7 and 12 | 13: a last root group of one object; 31 | 32 | 33: the last count whose roots a wave tests itself, bit 31 of the root masks
# of the two- and four-wave forms, and the first count on the queue path.  1: a group of one that is also the first.
OBJECT_COUNTS = (1, 6, 7, 12, 13, 31, 32, 33)
GRID_SHAPES = [(64, 40), (24, 35)]
GRID_COLS = 8
GRID_PITCH, GRID_SIDE = 60.0, 90.0      # one and a half pitches wide: neighbours overlap by half a pitch, more than a pixel even where 24 pixels show eight columns
GRID_RIM = (GRID_SIDE - GRID_PITCH) / 2
GRID_LIGHT = (450.0, 300.0, -400.0)     # right of, below and behind the camera: a nearer rectangle shadows its farther neighbours to the left and above
GRID_AWAY = 1.0e6                       # without_last: the last object this far to the right, beyond the frame and the light
GRID_Z_LAST = 350.0                     # the last object stands in front of all the others (400 .. 475)


def grid_depth(n, k):
    """Staggered: neighbours in a row are 25 or 75 apart, neighbours in a column 50; the shadow of a rectangle lands (450 - x, 300 - y) *
    dz / (z + 400) to its left and above, a few units to a pitch -- on its neighbour, a pitch of 60 away."""
    i, j = k % GRID_COLS, k // GRID_COLS
    return GRID_Z_LAST if k == n - 1 else 400.0 + 25.0 * ((3 * i + 2 * j) % 4)


def grid_extent(n):
    cols, rows = min(n, GRID_COLS), (n + GRID_COLS - 1) // GRID_COLS
    return cols, rows


def _grid_recipe(n, slot_of, last_away):
    """The recipe and meshes of the grid with mesh r<m> in grid slot slot_of[m]; slot k is column k % 8 of row k // 8."""
    cols, rows = grid_extent(n)
    r = scenes.Recipe()
    meshes = {}
    for m in range(n):
        k = slot_of[m]
        i, j = k % GRID_COLS, k // GRID_COLS
        z = grid_depth(n, k)
        s = z / 400.0      # pitch and side are those of the plane z = 400: on screen every rectangle overlaps its neighbours by half the pitch, whatever their depths
        x0, y0 = ((i - cols / 2.0) * GRID_PITCH - GRID_RIM) * s, ((j - rows / 2.0) * GRID_PITCH - GRID_RIM) * s
        if last_away and k == n - 1:
            x0 += GRID_AWAY
        meshes[f"r{m:02d}"] = w8.rect(z, x0, y0, x0 + GRID_SIDE * s, y0 + GRID_SIDE * s, 1 + k % 2)
        r.load(f"r{m:02d}.obj", f"r{m:02d}")
        r.color(f"r{m:02d}.obj", scenes.SOUP_PALETTE[k % len(scenes.SOUP_PALETTE)])
        r.bvh(f"r{m:02d}.obj")
    r.light = GRID_LIGHT
    return r, meshes


def object_grid(n, last_away=False):
    """(flat scene, light): n rectangles of alternately 2 and 4 triangles, eight to a row, centred on the z axis, at staggered depths
    (grid_depth).  Object k of the flat scene stands in slot k -- the builder orders objects by a hash of their names, so the scene is
    built once to learn that order and once more with every mesh in its object's slot.  The last object (index n - 1) is the nearest:
    nothing hides it, and it shadows a neighbour to its left or above it.  last_away: the same scene with that object far beside the
    frame and the light (without_last)."""
    from simple_raytracer_amd import host
    names = host.build_flat_scene(*_grid_recipe(n, list(range(n)), False)).names
    slot_of = [names.index(f"r{m:02d}.obj") for m in range(n)]
    r, meshes = _grid_recipe(n, slot_of, last_away)
    flat = host.build_flat_scene(r, meshes)
    assert flat.n_objects == n and flat.names == names
    z = flat.node_min.reshape(-1, 3)[np.asarray(flat.obj_root).astype(np.int64), 2]
    assert all(float(z[k]) == grid_depth(n, k) for k in range(n)), "object k stands in slot k"
    return flat, r.light


def grid_focal(n, W, H):
    """The whole grid (as it stands in the plane z = 400) with a rim of background: inside 0.9 of the frame both ways."""
    cols, rows = grid_extent(n)
    return float(0.9 * 400.0 * min(W / (cols * GRID_PITCH + 2 * GRID_RIM), H / (rows * GRID_PITCH + 2 * GRID_RIM)))


def grid_view(n, W, H):
    focal = grid_focal(n, W, H)
    return lambda L, flags=0: abi.make_params(W, H, abi.light_staircase(GRID_LIGHT, L), focal=focal, flags=flags)


def without_last(n):
    """object_grid(n) with its last object moved out of every ray's way: the others keep their triangles' indices.  A pixel that shows
    the same triangle in both scenes and another colour has a shadow ray that the last object stops (and no other object does: the
    colour would not change)."""
    assert n >= 2
    return object_grid(n, last_away=True)[0]


def shadowed_by_last(oracle, n, W, H, plain):
    """(H, W) bool at one light sample: the pixels of the oracle's frame `plain` of object_grid(n) (rendered with pow="device") whose
    shadow ray the last object stops."""
    rest = oracle.render(without_last(n), grid_view(n, W, H)(1), pow="device")
    same = (np.asarray(plain["hit_id"]) == rest["hit_id"]) & (rest["hit_id"] >= 0)
    return same & (bits(plain["rgb_linear"]) != bits(rest["rgb_linear"])).any(-1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def root_passes_by_object(ts, flat, W, H, focal):
    """(n_objects, H, W) bool: wave8_scenes.root_passes for one root box at a time (ts: tests/test_tile_spans.py, its judge)."""
    out = []
    for k in range(flat.n_objects):
        one = types.SimpleNamespace(obj_root=np.asarray(flat.obj_root)[k:k + 1], node_min=flat.node_min, node_max=flat.node_max)
        out.append(w8.root_passes(ts, one, W, H, focal))
    return np.stack(out)


def moved(flat):
    """Every object a little to the side, up and AWAY, at the scene's own scale (trace_half_eight_graph_case.moved_scene moves in x and
    y only, which leaves a rectangle in a plane z = const the same t and the same colour on every pixel it keeps): every hit pixel
    gets another t."""
    import pose_ref
    from simple_raytracer_amd import host
    r = np.asarray(flat.obj_root).astype(np.int64)
    mn, mx = flat.node_min.reshape(-1, 3)[r], flat.node_max.reshape(-1, 3)[r]
    span = float((mx - mn)[:, :2].max())
    mats = np.tile(np.asarray(host.Transformation.changeObjPosition(0.02 * span, -0.015 * span, 0.05 * span), np.float32).reshape(1, 16), (flat.n_objects, 1))
    return pose_ref.pose_flat(flat, mats)
