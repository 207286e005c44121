"""CPU: the yardstick of the visibility masks (tests/visibility_ref.py) against what it extends, and the input conditions of every case
tests/test_gpu_visibility.py uses.  With all-ones masks it is shadow_rule_ref's rows bit for bit; the filter on the candidate set is the
oracle's own 1 x 1 frames on the flat scene with the hidden objects removed (visibility_ref.sub_scene), ids mapped back and t by bits;
every mask and every srt_visibility triple of the GPU cases changes some rays and leaves others."""
import numpy as np
import pytest

import ray_query_ref as rq
import ray_range_ref as rr
import shade_path_ref as sp
import shadow_rule_ref as sh
import surface_ref as sf
import tree_shapes as ts
import visibility_ref as vr

bits = sf.bits


def test_all_ones_masks_are_the_shadow_rule_yardstick(oracle):
    name = "cubes4_a40"
    flat, rays, lights, refl = sh.lamp_case(name)
    for table in (None, np.full(flat.n_objects, vr.ALL, np.uint32), vr.case_table(flat)):
        segs = vr.trace(oracle, flat, rays, lights, vr.DEPTH, (vr.ALL, vr.ALL, vr.ALL), table, vr.BOUNCE_T_MIN, colours=vr.case_colours(oracle, name),
                        cands=vr.case_memo(oracle, name))
        for rule in (None, sh.SELF):
            sp.assert_same(vr.shade_paths_of(oracle, flat, segs, vr.DEPTH, rule, refl), sh.case_reference(oracle, name, rule), f"all ones, rule {rule}")


def test_the_frame_yardstick_at_spp_1_is_the_path_yardstick(oracle):
    import render_paths_ref as rpr
    name = "cubes4_a40"
    flat, _, lights, refl = sh.lamp_case(name)
    p = rpr.camera_params(name, lights, 16, 9)
    rays, live = rpr.frame_rays_owned(p)
    assert live.all()
    vis, table = vr.case_vis(name, 0), vr.case_table(flat)
    a = rpr.flat_rows(vr.render_paths(oracle, flat, p, 2, vis, table, refl, vr.BOUNCE_T_MIN, rule=sh.ENDED))
    sp.assert_same(a, vr.shade_paths(oracle, flat, rays.reshape(-1, 6), lights, 2, vis, table, refl, vr.BOUNCE_T_MIN, rule=sh.ENDED), "16 x 9 frame")


def check_against_sub_scene(oracle, flat, rays, c, hide):
    table, m = vr.hidden(flat, *hide)
    hit, t = vr.closest(c, flat, m, table)
    sub, ids = vr.sub_scene(flat, [k for k in range(flat.n_objects) if k not in hide])
    assert sub.n_objects == flat.n_objects - len(hide) and sub.n_tris == ids.size
    o_hit, o_t = rq.oracle_trace(oracle, sub, rays)
    assert np.array_equal(vr.map_back(o_hit, ids), hit), hide
    assert np.array_equal(bits(o_t), bits(t)), hide
    return hit


@pytest.mark.parametrize("hide", [0, 1, 2, 3])
def test_a_hidden_object_is_the_oracle_on_the_reduced_scene(oracle, hide):
    name = "cubes4_a40"
    flat, rays, _, _ = sh.lamp_case(name)
    c = vr.case_candidates(oracle, name)
    hit = check_against_sub_scene(oracle, flat, rays, c, (hide,))
    assert not (flat.tri_obj[hit[hit >= 0]] == hide).any()
    assert (flat.tri_obj[rr.closest(c)[0][rr.closest(c)[0] >= 0]] == hide).any(), "the hidden object was never hit"


def test_two_hidden_objects_of_many_roots(oracle):
    flat, rays = ts.family("roots33"), ts.ray_batch("roots33")
    c = rr.candidates(oracle, flat, rays)
    h0, _ = rr.closest(c)
    seen = np.bincount(flat.tri_obj[h0[h0 >= 0]], minlength=flat.n_objects)
    hide = tuple(sorted(int(k) for k in np.argsort(-seen, kind="stable")[:2]))      # the two objects most rays hit
    hit = check_against_sub_scene(oracle, flat, rays, c, hide)
    assert (hit != h0).any()
    # bit k % 32: objects 0 and 32 share a bit, so hiding one through the ray mask hides the other
    table, m = vr.hidden(flat, 0)
    assert table[0] == table[32] and np.array_equal(vr.closest(c, flat, m, table)[0], vr.closest(c, flat, None, np.where(np.isin(np.arange(33), (0, 32)), 0, vr.ALL))[0])


@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_ray_masks_meet_their_input_conditions(oracle, name):
    flat, rays, _, _ = sh.lamp_case(name)
    c = vr.case_candidates(oracle, name)
    table = vr.case_table(flat)
    for hide in vr.HIDDEN_FROM_RAYS[name]:
        got = vr.mask_conditions(flat, c, vr.hidden(flat, hide)[1], table)
        print(name, "hidden", hide, got)
        assert got["other"] > 0 and got["miss"] > 0 and got["same"] > 0, (name, hide, got)
    # the masks as the GPU case deals them: each hiding kind still does all three on its own share of the rays
    masks, kind = vr.ray_masks(name, rays.shape[0])
    h0, _ = rr.closest(c)
    h1, _ = vr.closest(c, flat, masks, table)
    for k in range(vr.FIRST_HIDING_KIND, vr.FIRST_HIDING_KIND + len(vr.HIDDEN_FROM_RAYS[name])):
        sel = kind == k
        assert ((h1 != h0) & (h1 >= 0))[sel].any() and ((h0 >= 0) & (h1 < 0))[sel].any() and ((h1 == h0) & (h0 >= 0))[sel].any(), (name, k)
    assert (h1[kind == 0] < 0).all() and (h1[kind == 2] < 0).all() and np.array_equal(h1[kind == 1], h0[kind == 1])


@pytest.mark.parametrize("name", list(sh.LAMPS))
def test_visibility_triples_meet_their_input_conditions(oracle, name):
    flat, rays, lights, _ = sh.lamp_case(name)
    plain = vr.trace(oracle, flat, rays, lights, vr.DEPTH, (vr.ALL, vr.ALL, vr.ALL), None, vr.BOUNCE_T_MIN, cands=vr.case_memo(oracle, name))
    for which in (0, 1):
        got = vr.vis_conditions(flat, plain, vr.case_trace(oracle, name, which, colours=False))
        print(name, vr.HIDE[name][which], got)
        assert got["segment0"] > 0, "the triple changes no segment 0"
        assert got["later"] > 0, "the triple changes no later segment of a path whose segment 0 stays"
        assert got["flipped"] > 0 and got["kept"] > 0, "the triple flips no shadow bit, or all of them"
