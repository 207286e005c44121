"""What tests/test_gpu_trace_wave8.py and tests/trace_wave8_graph_case.py share: the scenes and shapes of the one-wave trace workgroups
(k_trace_nq_wave8_spans, srt_kernels.h), the "ledge" view, and the CPU-side count of the half tiles that take the wave-level miss path.

The kernel's workgroup is one wave that owns half an 8x8 tile (rows 4h .. 4h + 3) and tests the roots of its own 32 rays.  A wave inside
the tile spans none of whose rays passes a root box writes its 32 misses through the closest-hit phase's write-out; the two-wave form never
does that (there wave 0 decides for the whole tile).  The golden scenes reach that path only by accident, so the LEDGE puts it on a whole
strip: a wide square whose lower edge projects onto the middle of a tile row, and a small one in front of it that shadows it.  In the
64 x 40 frame at focal 100 the big square (x -100 .. 100, y -60 .. 30, z 400) covers columns 7 .. 57 and rows 5 .. 27 (j0 = -20: the edge
y = 30 is row 30 * 100 / 400 + 20 = 27.5), so in tile row 3 (rows 24 .. 31) the upper halves hold hits and the lower halves -- inside
the spans, which are whole tiles -- hold none, over tiles 0 .. 7."""
import numpy as np

import scenes
from simple_raytracer_amd import abi

IN_FLIGHT = abi.SRT_FLAG_FRAMES_IN_FLIGHT
V_WAVE_8 = 31         # the eight-wave build and, over tile spans, its one-wave workgroups, without the in-flight hint
V_ADJACENT = 32      # the one-wave workgroups in the other dispatch order: a tile's halves next to each other (shipped: eight apart, on one XCD)
V_FOUR_WAVES = 59     # four waves of 4x4 pixels per tile on the full grid
V_TWO_WAVES = 67      # the shipped choice with the two-wave workgroups kept (k_trace_nq_half8_spans)
# 37 x 29: tiles cut on both edges; 64 x 40: whole tiles; 40 x 36: rows % 8 == 4 -- the last tile row's lower halves have no live pixel
SHAPES = [(37, 29), (64, 40), (40, 36)]
LIGHTS = [1, 4]

LEDGE_W, LEDGE_H, LEDGE_FOCAL = 64, 40, 100.0
LEDGE_LIGHT = (120.0, -60.0, 0.0)


def rect(z, x0, y0, x1, y1, segments=6):
    """A rectangle in the plane z = const as a fan of 2 * segments triangles from (x0, y0) (half_eight_scenes.fan is the square form)."""
    a = [x0, y0, z, 1.0]
    rim = [(x1, y) for y in np.linspace(y0, y1, segments + 1)] + [(x, y1) for x in np.linspace(x0, x1, segments + 1)[::-1][1:]]
    return np.array([[a, [p[0], p[1], z, 1.0], [q[0], q[1], z, 1.0]] for p, q in zip(rim[:-1], rim[1:])], np.float32)


def ledge_scene():
    """(flat scene, light)"""
    from simple_raytracer_amd import host
    r = scenes.Recipe()
    meshes = {"wall": rect(400.0, -100.0, -60.0, 100.0, 30.0), "chip": rect(300.0, 10.0, -40.0, 50.0, -5.0, 3)}
    for k, name in enumerate(meshes):
        r.load(f"{name}.obj", name)
        r.color(f"{name}.obj", scenes.SOUP_PALETTE[k])
        r.bvh(f"{name}.obj")
    r.light = LEDGE_LIGHT
    flat = host.build_flat_scene(r, meshes)
    assert flat.n_objects == 2
    return flat, r.light


def ledge_params(W, H, L, flags=0):
    assert (W, H) == (LEDGE_W, LEDGE_H)
    return abi.make_params(W, H, abi.light_staircase(LEDGE_LIGHT, L), focal=LEDGE_FOCAL, flags=flags)


def half_tiles(mask):
    """(H, W) bool -> (tile rows, 2, tile columns) bool: does the half tile hold a pixel of the mask."""
    H, W = mask.shape
    pad = np.zeros(((H + 7) // 8 * 8, (W + 7) // 8 * 8), bool)
    pad[:H, :W] = mask
    return pad.reshape(pad.shape[0] // 8, 2, 4, pad.shape[1] // 8, 8).any(axis=(2, 4))


def root_passes(ts, flat, W, H, focal):
    """(H, W) bool: the pixel's ray passes some root box under the reference's comparisons (ts: tests/test_tile_spans.py, its judge)."""
    mn, mx = ts.root_boxes(flat)
    i0, j0 = int(-np.float32(W) / 2), int(-np.float32(H) / 2)
    d = np.empty((H, W, 3), np.float32)
    d[..., 0] = (i0 + np.arange(W)).astype(np.float32)[None, :]
    d[..., 1] = (j0 + np.arange(H)).astype(np.float32)[:, None]
    d[..., 2] = np.float32(focal)
    out = np.zeros((H, W), bool)
    for k in range(mn.shape[0]):
        out |= ts.ray_aabb_f32(np.zeros(3, np.float32), d, mn[k], mx[k])
    return out


def miss_path_half_tiles(ts, flat, kept, hit_id, W, H, focal):
    """(tile rows, 2, tile columns) bool: half tiles INSIDE the spans (kept: the table's tiles) with live pixels, none of whose rays passes
    a root box -- the wave writes 32 misses itself -- while the tile's other half has hit pixels in the oracle's frame."""
    passes, hits, live = half_tiles(root_passes(ts, flat, W, H, focal)), half_tiles(np.asarray(hit_id) >= 0), half_tiles(np.ones((H, W), bool))
    assert not (hits & ~passes).any(), "a hit pixel's ray passes its object's root box"
    return kept[:, None, :] & live & ~passes & hits[:, ::-1, :]
