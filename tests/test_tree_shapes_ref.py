"""CPU: the generator of tests/tree_shapes.py and the yardsticks of tests/test_gpu_tree_shapes.py, right on their own -- every family
meets the layout contract of include/srt.h, its tight boxes are the reference's fold, the query yardsticks accept trees no builder
makes, and the oracle alone shows that each family reaches the device path it is for, on the very frames and rays the GPU tests use."""
import numpy as np
import pytest

import pose_ref
import ray_query_ref as rq
import ray_range_ref as rr
import shade_query_ref as sq
import tree_shapes as ts
from simple_raytracer_amd import abi

LEAF_MAX = 31


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_layout(flat):
    """include/srt.h, "Layout contract", restated: every node is reachable from exactly one root; a leaf has left == right == -1 and
    owns [first, first + count), 0 <= count (<= 31, the limit of a leaf word); an inner node has two children; walking all objects' trees
    DFS left-first meets the leaves' ranges contiguously in increasing order, covering [0, n_tris) exactly once; tri_obj[i] is the
    object whose tree owns triangle i."""
    N = flat.n_nodes
    seen = np.zeros(N, int)
    cursor = 0
    for k, root in enumerate(flat.obj_root):
        stack = [int(root)]
        while stack:
            i = stack.pop()
            assert 0 <= i < N
            seen[i] += 1
            l, r = int(flat.node_left[i]), int(flat.node_right[i])
            if l < 0 and r < 0:
                assert l == -1 and r == -1
                c = int(flat.node_count[i])
                assert 0 <= c <= LEAF_MAX
                if c:
                    assert int(flat.node_first[i]) == cursor
                assert (flat.tri_obj[cursor:cursor + c] == k).all()
                cursor += c
            else:
                assert l >= 0 and r >= 0, "full binary"
                stack.append(r); stack.append(l)
    assert (seen == 1).all() and cursor == flat.n_tris


@pytest.mark.parametrize("name", ts.FAMILIES)
def test_layout_contract(name):
    flat = ts.family(name)
    check_layout(flat)
    assert flat.tri_points.shape == (flat.n_tris, 3, 4) and np.isfinite(flat.tri_points).all()
    if name.startswith("roots"):
        assert flat.n_nodes == flat.n_objects == int(name[5:]) and (ts.node_depth(flat) == 0).all()
        sizes = set(flat.node_count.tolist())
        assert (name == "roots300" and sizes == {1, 2, 3}) or {0, 31} <= sizes
    if name.startswith("comb"):
        d = ts.node_depth(flat)
        comb = d[:2 * int(name[4:]) + 1]
        assert comb.max() == int(name[4:]) and d[2 * int(name[4:]) + 1] == 0, "object 0 is a comb of exactly this height"
        leaf = flat.node_left < 0
        assert set(flat.node_count[leaf][:int(name[4:]) + 1].tolist()) == {1, 2}
    if name in ("sliced", "shuffled", "loose", "shrunk"):
        assert flat.n_objects == 3 and 140 <= flat.n_tris <= 160
        assert set(ts.LEAF_SIZES) <= set(flat.node_count[flat.node_left < 0].tolist())


def test_shapes():
    """What each shape is: which children are leaves, the height, and the visit order the shape implies."""
    tris = np.ones((10, 3, 4), np.float32); tris[:, 0, 0] = np.arange(10)       # the source index in a coordinate
    leaves = (1, 2, 3, 4)
    for shape, visit in (("left_comb", [6, 7, 8, 9, 3, 4, 5, 1, 2, 0]), ("right_comb", list(range(10))), ("random", list(range(10))),
                         ("zigzag", [0, 3, 4, 5, 6, 7, 8, 9, 1, 2])):
        f = ts.flat_scene([dict(tris=tris, leaves=leaves, shape=shape, seed=1)])
        check_layout(f)
        assert f.tri_points[:, 0, 0].astype(int).tolist() == visit, shape
        inner = np.flatnonzero(f.node_left >= 0)
        l_leaf, r_leaf = f.node_left[f.node_left[inner]] < 0, f.node_left[f.node_right[inner]] < 0
        if shape == "left_comb":
            assert r_leaf.all() and ts.node_depth(f).max() == 3
        if shape == "right_comb":
            assert l_leaf.all() and ts.node_depth(f).max() == 3
        if shape == "zigzag":
            assert (l_leaf | r_leaf).all() and not l_leaf.all() and not r_leaf.all() and ts.node_depth(f).max() == 3
    f = ts.flat_scene([dict(tris=tris[:5], leaves=(5,), shape="root_leaf"), dict(tris=tris[:0], leaves=(0,), shape="root_leaf")])
    check_layout(f)
    assert f.n_nodes == 2 and f.obj_root.tolist() == [0, 1]
    with pytest.raises(AssertionError):
        ts.flat_scene([dict(tris=tris, leaves=(5, 5), shape="root_leaf")])


def test_shuffled_restated_into_preorder_is_sliced():
    a, b = ts.family("sliced"), ts.family("shuffled")
    assert int(b.obj_root.min()) > 0, "roots are not first"
    kids = b.node_left[b.node_left >= 0]
    assert (np.abs(kids - np.flatnonzero(b.node_left >= 0)) > 1).sum() >= 3, "children are far from their parents"
    assert not np.array_equal(a.node_left, b.node_left)
    p = ts.to_preorder(b)
    for k in abi.FlatScene.ARRAYS:
        x, y = getattr(a, k), getattr(p, k)
        assert (x is None and y is None) or np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), k
    pa = ts.to_preorder(a)
    assert np.array_equal(pa.node_left, a.node_left) and np.array_equal(pa.obj_root, a.obj_root), "the generator's own order is pre-order"


@pytest.mark.parametrize("name", [n for n in ts.FAMILIES if n not in ("loose", "shrunk")])
def test_tight_boxes(name):
    """pose_ref's box restatement at the identity pose gives the generator's tight boxes bit for bit, and both are the brute-force
    min / max over the triangles below each node."""
    flat = ts.family(name)
    ident = np.tile(np.eye(4, dtype=np.float32).reshape(16), (flat.n_objects, 1))
    pts = pose_ref.transform_objects(flat, ident)
    assert np.array_equal(bits(pts), bits(flat.tri_points)), "the identity pose moves nothing"
    mn, mx = pose_ref.boxes(flat, pts)
    assert np.array_equal(bits(mn), bits(flat.node_min)) and np.array_equal(bits(mx), bits(flat.node_max))
    xyz = flat.tri_points[..., :3]
    def below(i):
        if flat.node_left[i] < 0:
            return list(range(int(flat.node_first[i]), int(flat.node_first[i]) + int(flat.node_count[i])))
        return below(int(flat.node_left[i])) + below(int(flat.node_right[i]))
    import sys
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 2000))
    empty = 0
    for i in range(flat.n_nodes):
        v = xyz[below(i)].reshape(-1, 3)
        if len(v):
            assert np.array_equal(flat.node_min[i], v.min(0)) and np.array_equal(flat.node_max[i], v.max(0)), i
        else:
            empty += 1
            assert (flat.node_min[i] == ts.FLT_MAX).all() and (flat.node_max[i] == -ts.FLT_MAX).all(), i
    assert empty or name in ("comb255", "comb256", "roots300")


def test_loose_and_shrunk_boxes():
    tight, loose, shrunk = ts.family("sliced"), ts.family("loose"), ts.family("shrunk")
    full = tight.node_min[:, 0] < ts.FLT_MAX
    assert (loose.node_min[full] < tight.node_min[full]).all() and (loose.node_max[full] > tight.node_max[full]).all()
    assert np.array_equal(bits(loose.node_min[~full]), bits(tight.node_min[~full]))
    inner = np.flatnonzero(loose.node_left >= 0)
    out = 0
    for side in (loose.node_left, loose.node_right):
        c = side[inner]
        ok = full[c]
        out += int(((loose.node_min[c][ok] < loose.node_min[inner][ok]) | (loose.node_max[c][ok] > loose.node_max[inner][ok])).any(1).sum())
    assert out >= 5, "children stick out of their parents"
    leaf = shrunk.node_left < 0
    assert np.array_equal(bits(shrunk.node_min[~leaf]), bits(tight.node_min[~leaf])) and np.array_equal(bits(shrunk.node_max[~leaf]), bits(tight.node_max[~leaf]))
    cut = np.flatnonzero(leaf & (shrunk.node_min > tight.node_min).all(1) & (shrunk.node_max < tight.node_max).all(1))
    assert cut.size >= 4 and (shrunk.node_min[cut] < shrunk.node_max[cut]).all()
    assert (shrunk.node_count[cut] > 8).any(), "a sliced leaf is among the shrunk ones"


# ---- the oracle reaches the paths ----------------------------------------------------------------------------------------------------
def winners(flat, hit):
    """(leaf node, slice of 8 inside the leaf) of the hits among `hit`."""
    node, pos = ts.tri_leaf(flat)
    h = hit[hit >= 0]
    return node[h], pos[h] // 8


@pytest.mark.parametrize("name", ts.FAMILIES)
def test_hits_and_misses(oracle, name):
    """At least 10 % of the rays hit and at least 10 % miss: the plain frame, the sheared camera frame, the ray batch."""
    r = ts.reference(oracle, name)
    for what, hit in (("frame", r["frame"]["hit_id"]), ("camera", r["camera"]["hit_id"]), ("rays", r["ray_hit"])):
        share = float((hit >= 0).mean())
        print(name, what, "hit share", round(share, 3))
        assert 0.1 <= share <= 0.9, (name, what, share)
    assert r["rays"].shape == (ts.N_UNRELATED + ts.N_AIMED, 6)


@pytest.mark.parametrize("name", ts.FAMILIES)
def test_query_yardsticks_accept_the_family(oracle, name):
    """ray_range_ref on these trees: its closest hit without bounds is the oracle's, ray by ray on the batch and pixel by pixel on both
    frames (a frame is its rays); ray_query_ref and shade_query_ref trace the same hits."""
    r = ts.reference(oracle, name)
    flat = r["flat"]
    c = rr.candidates(oracle, flat, r["rays"])
    hit, t = rr.closest(c)
    assert np.array_equal(hit, r["ray_hit"]) and np.array_equal(bits(t), bits(r["ray_t"]))
    for cam, key in ((False, "frame"), (True, "camera")):
        h, tt = rr.closest(rr.candidates(oracle, flat, ts.frame_rays(cam)))
        assert np.array_equal(h, r[key]["hit_id"].reshape(-1)) and np.array_equal(bits(tt), bits(r[key]["t"].reshape(-1))), key
    some = r["rays"][::23]
    h2, t2 = rq.oracle_trace(oracle, flat, some)
    assert np.array_equal(h2, r["ray_hit"][::23]) and np.array_equal(bits(t2), bits(r["ray_t"][::23]))
    h3, t3, lin, rgb8 = sq.oracle_shade(oracle, flat, some, abi.light_staircase(ts.LIGHT, 2))
    assert np.array_equal(h3, h2) and np.array_equal(bits(t3), bits(t2)) and (lin[h3 >= 0] != 0).any()
    occ = rr.occluded(c, flat)
    assert 0 < occ.sum() < occ.size


def test_sliced_reaches_every_slice(oracle):
    """Rays enter leaves of more than 8, 16 and 24 triangles, and the winner lies in the second, third and fourth slice of 8 -- on the
    frame, on the ray batch, and among the aimed rays alone."""
    for name in ("sliced", "shuffled", "loose"):
        r = ts.reference(oracle, name)
        flat = r["flat"]
        for what, hit in (("frame", r["frame"]["hit_id"].reshape(-1)), ("rays", r["ray_hit"]), ("aimed", r["ray_hit"][ts.N_UNRELATED:])):
            node, sl = winners(flat, hit)
            print(name, what, "winners per slice", np.bincount(sl, minlength=4).tolist())
            assert (np.bincount(sl, minlength=4)[:4] >= (1 if what == "aimed" else 3)).all(), (name, what)
            for limit in (8, 16, 24):
                assert (flat.node_count[node] > limit).any()
        c = rr.candidates(oracle, flat, r["rays"])
        leaf_of, _ = ts.tri_leaf(flat)
        entered = np.unique(leaf_of[c.tri])
        for limit in (8, 16, 24):
            assert (flat.node_count[entered] > limit).sum() >= 2, limit


@pytest.mark.parametrize("name", ["comb255", "comb256"])
def test_comb_is_won_deep_down(oracle, name):
    r = ts.reference(oracle, name)
    flat = r["flat"]
    depth = ts.node_depth(flat)
    for what, hit in (("frame", r["frame"]["hit_id"].reshape(-1)), ("rays", r["ray_hit"])):
        node, _ = winners(flat, hit)
        print(name, what, "deepest winning leaf", int(depth[node].max()), "winners at depth >= 200:", int((depth[node] >= 200).sum()))
        assert (depth[node] >= 200).sum() >= 5, what
    assert (flat.tri_obj[r["frame"]["hit_id"][r["frame"]["hit_id"] >= 0]] == 1).any(), "the zigzag object is seen"


@pytest.mark.parametrize("name", ["roots5", "roots17", "roots32", "roots33", "roots300"])
def test_roots_last_object_is_hit_and_tiles_differ(oracle, name):
    """The last object (32 in roots33: the one beyond the 32-bit root mask) is hit, and the 64 rays of some 8 x 8 tile pass different
    subsets of the root boxes."""
    r = ts.reference(oracle, name)
    flat = r["flat"]
    last = flat.n_objects - 1
    hit = r["frame"]["hit_id"].reshape(-1)
    assert (flat.tri_obj[hit[hit >= 0]] == last).sum() >= 3
    reach = rr.reached_nodes(oracle, flat, ts.frame_rays())[:, flat.obj_root.astype(np.int64)].reshape(ts.H, ts.W, -1)
    mixed = 0
    for y in range(0, ts.H, 8):
        for x in range(0, ts.W, 8):
            tile = reach[y:y + 8, x:x + 8].reshape(-1, flat.n_objects)
            mixed += len(np.unique(tile, axis=0)) >= 2
    print(name, "tiles whose rays pass different subsets of the root boxes:", mixed)
    assert mixed >= 10, mixed


def test_loose_and_shrunk_boxes_decide_hits(oracle):
    """The hit ids differ from `sliced`'s, so the boxes really decided something (same triangles, same rays)."""
    base = ts.reference(oracle, "sliced")
    for name in ("loose", "shrunk"):
        r = ts.reference(oracle, name)
        n = sum(int((r[k]["hit_id"] != base[k]["hit_id"]).sum()) for k in ("frame", "camera")) + int((r["ray_hit"] != base["ray_hit"]).sum())
        print(name, "hit ids that differ from sliced's", n)
        assert n >= 1, name
        work = r["ray_node_tests"] + r["ray_tri_tests"]
        assert work != base["ray_node_tests"] + base["ray_tri_tests"], name


def test_ties(oracle):
    """A pixel with t == 0; hits tied across two objects, which go to the lowest id; hits tied inside a sliced leaf, between its first
    and its third slice."""
    r = ts.reference(oracle, "ties")
    flat = r["flat"]
    fr = r["frame"]
    t0 = fr["t"] == 0
    assert t0.sum() >= 100 and (flat.tri_obj[fr["hit_id"][t0]] == 2).all()
    c = rr.candidates(oracle, flat, ts.frame_rays())
    hit, t = rr.closest(c)
    at_min = (c.t != -np.inf) & (bits(c.t + np.float32(0.0)) == bits(t + np.float32(0.0))[c.ray]) & (hit[c.ray] >= 0)
    leaf_of, pos = ts.tri_leaf(flat)
    n_rays = hit.size
    per_obj = np.zeros((n_rays, flat.n_objects), bool)
    per_obj[c.ray[at_min], flat.tri_obj[c.tri[at_min]]] = True
    across = per_obj[:, 0] & per_obj[:, 1]
    print("pixels with t == 0:", int(t0.sum()), "tied across objects:", int(across.sum()))
    assert across.sum() >= 100 and (flat.tri_obj[hit[across]] == 0).all(), "the lowest id wins"
    big = int(np.flatnonzero((flat.node_left < 0) & (flat.node_count == 22))[0])
    in_big = at_min & (leaf_of[c.tri] == big)
    sl = np.zeros((n_rays, 4), bool)
    sl[c.ray[in_big], pos[c.tri[in_big]] // 8] = True
    inside = sl[:, 0] & sl[:, 2]
    print("tied inside the sliced leaf:", int(inside.sum()))
    assert inside.sum() >= 10 and (pos[hit[inside]] < 8).all()
    both = c.t[(c.t == 0) & at_min]
    assert np.signbit(both).any() and (~np.signbit(both)).any(), "t = +0 and t = -0 both occur"
