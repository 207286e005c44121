"""The scene that overflows a 384-entry node queue in the half-tile trace kernel's closest-hit phase, and the host-side count that says so
(tests/test_trace_half_eight_queue.py on the CPU, tests/test_gpu_trace_half_eight.py on the device).

Six objects, each a square in a plane z = const cut into a FAN of 32 triangles from its corner A to points on the two far edges, stacked in
z, facing the camera.  The 16 x 16-pixel frame at focal 400 looks along the z axis at a patch of +-3 units beside A, far from the far
edges: every triangle (A, P, Q) has its box from A to max(P, Q), which holds that patch, so every node's box does and every ray passes
every node of every object.  The host mirror's builder makes leaves of up to 8 triangles: 32 triangles are 7 nodes an object -- the root,
two inner nodes of 16 triangles, four leaves of 8 -- 42 in the scene.

A half-tile wave (32 rays) with root masks queues both children of every passing inner root, six objects at a time (384 / (2 * 32)):
2 x 32 x 6 = 384 entries, all inner nodes, which a 384-entry queue just holds.  The first pop takes 64 of them, each passes and is inner,
so 128 children are due while 320 wait: 448 > 384, and the wave finishes those subtrees with the stackless walk.  A 512-entry queue holds
the 448 (they are leaves: the queue only drains from there) and never overflows; a 256-entry queue takes four objects at a time,
2 x 32 x 4 = 256, and overflows at the first pop as well (192 + 128 = 320).

The light stands beside the stack, behind the front square: the shadow rays of the frame's right half cross the second square, those of
the left half pass beside it.

grid40: forty small squares of 12 triangles each (a root and two leaves), eight by five side by side with overlapping rims at forty depths.
More than 32 objects, so there are no root masks and every wave tests the roots itself -- on a scene whose boxes overlap little, which
the shipped choice renders with the fused trace kernel and its tile spans (the 40-object soup of tests/test_gpu_trace_half_seven.py goes to
the packet kernels)."""
import numpy as np

import scenes
from simple_raytracer_amd import abi

W = H = 16
FOCAL = 400.0
N_OBJECTS = 6
SEGMENTS = 16                 # per far edge: 2 * 16 = 32 triangles an object
LO, HI = -20.0, 380.0         # the square; the far-edge points are 25 apart, so the first and the last triangle's boxes reach +5
LIGHT = (-120.0, 0.0, 160.0)
NODES_PER_OBJECT = 7
RAYS_PER_WAVE = 32


def fan(z, lo_x=LO, lo_y=LO, size=HI - LO, segments=SEGMENTS):
    a = [lo_x, lo_y, z, 1.0]
    hx, hy = lo_x + size, lo_y + size
    rim = [(hx, y) for y in np.linspace(lo_y, hy, segments + 1)] + [(x, hy) for x in np.linspace(lo_x, hx, segments + 1)[::-1][1:]]
    return np.array([[a, [p[0], p[1], z, 1.0], [q[0], q[1], z, 1.0]] for p, q in zip(rim[:-1], rim[1:])], np.float32)


def recipe():
    r = scenes.Recipe()
    meshes = {}
    for k in range(N_OBJECTS):
        meshes[f"fan{k}"] = fan(100.0 + 10.0 * k)
        r.load(f"fan{k}.obj", f"fan{k}")
        r.color(f"fan{k}.obj", scenes.SOUP_PALETTE[k % len(scenes.SOUP_PALETTE)])
        r.bvh(f"fan{k}.obj")
    r.light = LIGHT
    return r, meshes


def flat_scene():
    from simple_raytracer_amd import host
    r, meshes = recipe()
    return host.build_flat_scene(r, meshes), r.light


def params(L, flags=0):
    return abi.make_params(W, H, abi.light_staircase(LIGHT, L), focal=FOCAL, flags=flags)


def frame_rays():
    """(H * W) x 6: origin and direction of the frame's primary rays, pixel (row, col) at index row * W + col."""
    col, row = np.meshgrid(np.arange(W), np.arange(H))
    d = np.stack([col - W // 2, row - H // 2, np.full_like(col, FOCAL)], -1).reshape(-1, 3).astype(np.float32)
    return np.concatenate([np.zeros_like(d), d], 1)


def half_tile_waves():
    """The pixel indices (row * W + col) of every half-tile wave's 32 rays: 8 x 4 pixels, two waves a tile."""
    out = []
    for ty in range(H // 8):
        for tx in range(W // 8):
            for h in range(2):
                out.append([(ty * 8 + h * 4 + y) * W + tx * 8 + x for y in range(4) for x in range(8)])
    return out


def closest_phase_queue(flat, passes, cap):
    """The node queue of one half-tile wave in the closest-hit phase with root masks (closest_hit_phase, srt_kernels.h: the 32 B records,
    entries in node-major order), counted on the host.  passes: rays x nodes, does the ray pass the node's box.  Returns (the highest
    fill, the entries the pushes asked room for when they first did not fit -- 0: never)."""
    left, right = flat.node_left.astype(np.int64), flat.node_right.astype(np.int64)
    n_rays = passes.shape[0]
    obj_g = min(cap // (2 * n_rays), 16)
    high = wanted = 0
    roots = flat.obj_root.astype(np.int64)
    for obj0 in range(0, len(roots), obj_g):
        q = []
        group = roots[obj0:obj0 + obj_g]
        pairs = [(int(root), ray) for root in group for ray in range(n_rays)]       # lane k: ray k & 31, object k >> 5
        for base in range(0, len(pairs), 64):
            inner = [(root, ray) for root, ray in pairs[base:base + 64] if passes[ray, root] and left[root] >= 0]
            q += [(int(right[root]), ray) for root, ray in inner] + [(int(left[root]), ray) for root, ray in inner]
        assert len(q) <= cap, "the roots' children always fit: P * OBJ_G <= NQCAP / 2"
        high = max(high, len(q))
        while q:
            m = min(len(q), 64)
            popped, q = q[len(q) - m:], q[:len(q) - m]
            inner = [(node, ray) for node, ray in popped if passes[ray, node] and left[node] >= 0]
            if len(q) + 2 * len(inner) <= cap:
                q += [(int(right[node]), ray) for node, ray in inner] + [(int(left[node]), ray) for node, ray in inner]
                high = max(high, len(q))
            elif not wanted:
                wanted = len(q) + 2 * len(inner)      # (the stackless walk finishes these subtrees: nothing is queued)
    return high, wanted


GRID_PITCH, GRID_SIDE = 60.0, 72.0      # squares wider than their pitch: neighbours overlap in the frame, the nearer one shadows the other
GRID_LIGHT = (200.0, -300.0, 0.0)


def grid40_scene():
    """(flat scene, light)"""
    from simple_raytracer_amd import host
    r = scenes.Recipe()
    meshes = {}
    for k in range(40):
        i, j = k % 8, k // 8
        meshes[f"sq{k}"] = fan(400.0 + 5.0 * ((k * 7) % 40), (i - 4) * GRID_PITCH - 6.0, (j - 2.5) * GRID_PITCH - 6.0, GRID_SIDE, 6)
        r.load(f"sq{k}.obj", f"sq{k}")
        r.color(f"sq{k}.obj", scenes.SOUP_PALETTE[k % len(scenes.SOUP_PALETTE)])
        r.bvh(f"sq{k}.obj")
    r.light = GRID_LIGHT
    flat = host.build_flat_scene(r, meshes)
    assert flat.n_objects == 40 and flat.n_nodes == 120
    return flat, r.light


def grid40_params(W, H, L, flags=0):
    """The grid is 492 x 312 at depths 400 .. 595: the frame sees it with a rim of background."""
    return abi.make_params(W, H, abi.light_staircase(GRID_LIGHT, L), focal=W * 0.9, flags=flags)
