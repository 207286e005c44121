"""CPU-only: the arithmetic behind the overflow case of tests/test_gpu_trace_half_eight.py, on the host mirror's tree (the scene and the
count: tests/half_eight_scenes.py).  Every ray of the frame passes every node; each of the eight half-tile waves fills a 384-entry queue
to the brim with the six roots' children, asks for 448 entries at its first pop and so takes the stackless walk; 512 entries hold it all
and 256 overflow too."""
import numpy as np

import half_eight_scenes as he
import ray_range_ref as rr


def test_fan_scene_overflows_384_entries_and_not_512(oracle):
    flat, _ = he.flat_scene()
    assert flat.n_objects == he.N_OBJECTS and flat.n_tris == he.N_OBJECTS * 2 * he.SEGMENTS
    assert flat.n_nodes == he.N_OBJECTS * he.NODES_PER_OBJECT
    leaf = flat.node_left < 0
    assert int(leaf.sum()) == 4 * he.N_OBJECTS and (flat.node_count[leaf] == 8).all()
    for root in flat.obj_root:                      # the root's children are inner nodes: what the first pop tests and finds inner
        assert flat.node_left[flat.node_left[root]] >= 0 and flat.node_left[flat.node_right[root]] >= 0
    reach = rr.reached_nodes(oracle, flat, he.frame_rays())
    assert reach.all(), "every ray passes every node"
    waves = he.half_tile_waves()
    assert len(waves) == 8 and sorted(sum(waves, [])) == list(range(he.W * he.H))
    for rays in waves:
        passes = reach[np.asarray(rays)]
        assert he.closest_phase_queue(flat, passes, 384) == (384, 448)
        assert he.closest_phase_queue(flat, passes, 512) == (448, 0)
        assert he.closest_phase_queue(flat, passes, 256) == (256, 320)
        assert he.closest_phase_queue(flat, passes, 160)[1] > 160      # (variant 14's queue overflows here as anywhere)


def test_the_frame_is_all_hits_with_a_shadow_edge(oracle):
    flat, _ = he.flat_scene()
    c = oracle.render(flat, he.params(1))
    assert (c["hit_id"] >= 0).all()
    front = int(np.argmin(flat.node_min[flat.obj_root.astype(np.int64), 2]))
    assert (flat.tri_obj[c["hit_id"]] == front).all(), "the nearest square wins every pixel"
    lit = c["rgb_linear"].sum(-1)
    assert lit[:, :4].min() > 3.0 * lit[:, 12:].max(), "left columns lit, right columns in the second square's shadow"
