"""GPU (-m gpu): srt_closest_segments at the edges of its definition (tests/segment_edges.py) -- crossings at t = 0 and 1 and one ulp outside,
segments in the triangle's plane, along an edge and at a vertex, den exactly 0 and beside it, u exactly 0 and 1, the closed radius at the
winner's own dist2, radii 0, -0, negative, NaN and +inf, end points NaN, infinite and 1e19, d with a zero, a subnormal and a 2^127
component, a zero-area triangle, one that is not finite and an empty leaf -- every output and both counters against tests/segment_ref.py
as bits, a NaN on both sides counting as equal.  All of them are ordinary inputs: the call stays memory-safe."""
import numpy as np
import pytest

import segment_edges as se
import segment_ref as sr

F = np.float32


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


def test_the_edge_inputs_are_what_they_are_named():
    """No GPU: the yardstick on the edge inputs gives what the names promise."""
    flat = se.scene()
    names, seg, rad = se.cases()
    want = sr.closest_segments(flat, seg, rad)
    row = {(n, bool(np.isinf(r))): i for i, (n, r) in enumerate(zip(names, rad))}
    at = lambda n, unbounded=False: row[(n, unbounded)]
    tri, feat, s, d2 = want["tri"], want["feature"], want["s"], want["dist2"]
    t0, t1 = se.canonical(flat, 0), se.canonical(flat, 1)             # the unit triangle and its neighbour, by their canonical ids
    assert feat[at("crossing at t = 0")] == 5 and s[at("crossing at t = 0")] == 0 and feat[at("crossing at t = 1")] == 5 and s[at("crossing at t = 1")] == 1
    assert feat[at("crossing, A one ulp above the plane")] != 5 and feat[at("crossing, A one ulp below the plane")] == 5
    assert feat[at("crossing, B one ulp above the plane")] != 5 and feat[at("crossing, B one ulp below the plane")] == 5
    assert tri[at("crossing on the shared diagonal")] == min(t0, t1) and d2[at("crossing on the shared diagonal")] == 0
    own = lambda n: names.index(n + " (its own radius)")
    assert tri[own("r * r == dist2")] == t0 and d2[own("r * r == dist2")] == F(0.25) and tri[own("r one ulp below")] == -1
    assert tri[own("r == 0 on a crossing")] == t0 and tri[own("r == -0 on a crossing")] == t0 and tri[own("r == 0 beside")] == -1
    assert tri[own("r negative")] == -1 and tri[own("r NaN")] == -1
    assert want["node_tests_each"][own("r negative")] == 0 and want["node_tests_each"][own("r NaN")] == 0 and want["node_tests_each"][own("r == -0 on a crossing")] > 0
    assert feat[at("u exactly 0")] == 2 and tuple(want["vw"][at("u exactly 0")]) == (0.0, 0.0) and tuple(want["vw"][at("u exactly 1")]) == (1.0, 0.0)
    assert {"den < 0", "den == 0", "den > 0"} & set(names) >= {"den == 0", "den > 0"}
    # the sloped rule either side: a zero, a subnormal and an overflowing component are not sloped; 2^-126 .. 2^127 are (their reciprocals are finite)
    _, _, d = sr.split(seg)
    sloped, _ = sr.sloped(d)
    for n, is_sloped in (("d.x == 0", False), ("d.x subnormal", False), ("d.x 2^-126", True), ("d.x 2^-100", True), ("d.x 2^126", True), ("d.x 2^127", True),
                         ("d.x overflows", False)):
        assert sloped[at(n)] == is_sloped, n
    assert want["node_tests_each"][at("sloped, a miss of every box")] == 1          # (the root fails: nothing else is tested)
    every = sr.closest_segments(flat, seg, rad, stage2=False)
    assert every["tri_tests"] > want["tri_tests"] and every["node_tests"] >= want["node_tests"]                                # (box test 2 is live on these inputs)
    assert np.isinf(rad).sum() > 40 and (want["tri_tests_each"][np.isinf(rad)] == flat.n_tris).all()      # (zero-area, not finite: candidates)
    assert (flat.node_count[(flat.node_left < 0)] == 0).any()                      # (the empty leaf)


@pytest.mark.gpu
def test_at_the_edges(srt):
    flat = se.scene()
    names, seg, rad = se.cases()
    want = sr.closest_segments(flat, seg, rad)
    ds = srt.DeviceScene(flat)
    got = ds.closest_segments(seg, radius=rad, count=True)
    for i, name in enumerate(names):                     # (row by row, so that a failure names its case)
        sr.same({k: got[k][i:i + 1] for k in sr.SAME_KEYS}, {k: want[k][i:i + 1] for k in sr.SAME_KEYS}, f"{name}, r {rad[i]}", nan_equal=True)
    sr.same_counts(got["stats"], want, len(seg), "the edge cases")
    # one at a time: a segment's result does not depend on its batch
    for i in (0, len(seg) // 2, len(seg) - 1):
        one = ds.closest_segments(seg[i:i + 1], radius=rad[i:i + 1], count=True)
        sr.same(one, {k: want[k][i:i + 1] for k in sr.SAME_KEYS}, names[i] + ", alone", nan_equal=True)
        assert (one["stats"]["node_tests_primary"], one["stats"]["tri_tests_primary"]) == (want["node_tests_each"][i], want["tri_tests_each"][i])
    # NULL radius: +inf for all
    unbounded = sr.closest_segments(flat, seg)
    free = ds.closest_segments(seg, count=True)
    sr.same(free, unbounded, "the edge cases without a radius", nan_equal=True)
    sr.same_counts(free["stats"], unbounded, len(seg), "the edge cases without a radius")
    ds.close()
