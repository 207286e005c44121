"""What tests/test_gpu_trace_whole.py and tests/trace_whole_graph_case.py share: the scenes that put the whole-frame trace kernel's pair
loops (k_trace_nq_whole8_spans, srt_kernels.h: two named triangle records, tested in turn, a tail for an odd count) through every way
they can end.

The host builder always halves an object's root and then halves a node while it holds more than 8 triangles, its triangles sorted by
their first vertex: an object of n <= 16 triangles is a root over two leaves of n / 2 and n - n / 2, so 16 triangles make two leaves at
the builder's maximum of 8.  LEAVES: a wall of 16 (8 + 8), and in front of it objects of 6 (3 + 3), 4 (2 + 2), 3 (1 + 2) and 1 (0 + 1)
triangles that overlap each other, so that the (leaf, ray) pairs of one triangle batch hold different counts -- a lane that ends in record
set A (1, 3) beside a lane that ends in set B (2, 8).  BLIND_FIRST / BLIND_LAST: a wall and, towards the light, an object of 16 triangles
of which ONE is large enough to shadow anything -- the first of its leaf (the shadow loop stops with the next record in flight) or the last
(it runs through all four pairs); the other fifteen are slivers off to one side, which is what sorts the large one to an end."""
import numpy as np

import scenes
import wave8_scenes as w8
from simple_raytracer_amd import abi

V_GENERAL = 68        # the shipped choice with the general frame's kernels kept (k_trace_nq_wave8_spans, k_shade_tile_spans)
FOCAL = 100.0
LIGHT = w8.LEDGE_LIGHT
LEAF_MAX_BUILT = 8    # the host builder's largest leaf (srt_host.cpp: halve while > 8)


def tris(z, *corners):
    """Triangles in the plane z = const from (x, y) triples."""
    return np.array([[[x, y, z, 1.0] for (x, y) in c] for c in corners], np.float32)


def _flat(meshes):
    from simple_raytracer_amd import host
    r = scenes.Recipe()
    for k, name in enumerate(meshes):
        r.load(f"{name}.obj", name)
        r.color(f"{name}.obj", scenes.SOUP_PALETTE[k % len(scenes.SOUP_PALETTE)])
        r.bvh(f"{name}.obj")
    r.light = LIGHT
    flat = host.build_flat_scene(r, meshes)
    assert flat.n_objects == len(meshes)
    return flat


def leaf_counts(flat):
    """object name -> the triangle counts of its leaves, in node order."""
    first = np.concatenate([np.asarray(flat.obj_root, np.int64), [len(flat.node_count)]])
    assert (np.diff(first) > 0).all()
    out = {}
    for ob in range(flat.n_objects):
        c = np.asarray(flat.node_count[first[ob]:first[ob + 1]])
        out[flat.names[ob].split(".")[0]] = [int(x) for x in c[c > 0]]
    return out


def fan(z, a, rim):
    """Triangles (a, rim[k], rim[k + 1]) in the plane z = const."""
    return tris(z, *[(a, p, q) for p, q in zip(rim[:-1], rim[1:])])


def leaves_scene():
    meshes = {"wall": w8.rect(500.0, -150.0, -100.0, 150.0, 100.0, 8),
              "six": w8.rect(400.0, -100.0, -60.0, 20.0, 30.0, 3),
              "three": fan(350.0, (-40, -50), [(60, -50), (60, 0), (60, 50), (-40, 50)]),
              "four": w8.rect(300.0, 0.0, -30.0, 80.0, 40.0, 2),
              "one": tris(250.0, ((-60, -20), (10, -20), (-25, 45)))}
    flat = _flat(meshes)
    assert leaf_counts(flat) == {"wall": [LEAF_MAX_BUILT, LEAF_MAX_BUILT], "six": [3, 3], "three": [1, 2], "four": [2, 2], "one": [1]}, leaf_counts(flat)
    return flat


def blind_scene(big_at):
    """big_at: 0 or 7, where in its leaf the one shadowing triangle of the blind lies."""
    side = 1.0 if big_at == 0 else -1.0      # slivers to the right: the large triangle sorts first; to the left: last
    slivers = [((side * (150 + 6 * k), 70), (side * (150 + 6 * k) + 2, 70), (side * (150 + 6 * k), 72)) for k in range(15)]
    big = ((-20, -45), (70, -45), (-20, 10))
    flat = _flat({"wall": w8.rect(400.0, -100.0, -60.0, 100.0, 50.0), "blind": tris(300.0, big, *slivers)})
    assert leaf_counts(flat)["blind"] == [LEAF_MAX_BUILT, LEAF_MAX_BUILT]
    ob = [n.split(".")[0] for n in flat.names].index("blind")
    own = np.asarray(flat.tri_points, np.float32).reshape(-1, 3, 4)[np.asarray(flat.tri_obj) == ob]
    e1, e2 = own[:, 1, :2] - own[:, 0, :2], own[:, 2, :2] - own[:, 0, :2]
    area = np.abs(e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])
    assert int(area.argmax()) == (0 if big_at == 0 else 15), "the large triangle is the first of the first leaf, or the last of the second"
    return flat


def params(W, H, L, flags=0):
    return abi.make_params(W, H, abi.light_staircase(LIGHT, L), focal=FOCAL, flags=flags)
