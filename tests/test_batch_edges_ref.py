"""The calls of tests/test_gpu_batch_edges.py (tests/batch_edges.py) are what they are named, on the CPU: by the restated hold rule, by
check_frame's preconditions and by the oracle's frames."""
import numpy as np
import pytest

import batch_edges as be
import gpu_frames as gf
import test_gpu_modes as tm


@pytest.fixture(scope="module")
def world():
    return be.prepare(tm.World(None))


@pytest.fixture(scope="module")
def facts(world):
    cache = {}
    def of(scene):
        if scene not in cache:
            cache[scene] = be.scene_facts(world.flat(scene)[0])
        return cache[scene]
    return of


def all_calls(world):
    """(call number, name, call) of every table; calls 6 and 7 reuse frames of these."""
    for (W, H) in be.EDGE_SIZES:
        for name, call in be.edge_calls(world, W, H).items():
            yield 1, f"{W}x{H} {name}", call
    for (W, H) in be.BOUNDARY_SIZES:
        for name, call in be.boundary_calls(world, W, H).items():
            yield 2, f"{W}x{H} {name}", call
    for (W, H) in be.BIG_SIZES:
        yield 3, f"{W}x{H}", be.big_call(world, W, H)
    for name, call in be.between_calls(world).items():
        yield 4, name, call
    for name in be.TABLE_CALLS:
        yield 5, name, be.table_call(world, name)
    for L in be.NULLS_L:
        for name, (call, _, _) in be.nulls_calls(world, L).items():
            yield 6, f"L {L} {name}", call


def with_shadow_div(p, div):
    q = type(p).from_buffer_copy(p)
    q._lights = p._lights
    if hasattr(p, "_ray_matrix"):
        q._ray_matrix = p._ray_matrix
    q.shadow_div = div
    return q


def blocked(world, oracle, f):
    """(hit, blocked) masks of a frame's live pixels: blocked = the colour depends on shadow_div, so some light sample's shadow ray is
    stopped.  A frame whose own shadow_div is 1 is compared at 5."""
    p = f.params
    flat = world.flat(f.scene)[0]
    a = oracle.render(flat, p if p.shadow_div != 1.0 else with_shadow_div(p, 5.0))
    b = oracle.render(flat, with_shadow_div(p, 1.0))
    live = gf.owned(p) >= 0
    hit = (a["hit_id"] >= 0) & live
    return hit, hit & (gf.bits(a["rgb_linear"]) != gf.bits(b["rgb_linear"])).any(-1)


def test_the_scene_of_call_3_is_over_32_mib_with_an_estimate_of_14_or_more(facts):
    f = facts(be.BIG)
    assert f.bytes > be.XCD_BYTES and f.overlap >= be.MID_OVERLAP and f.overlap < be.PACKET_OVERLAP and f.normals, f
    assert facts(be.BUNNY).overlap < be.MID_OVERLAP and facts(be.BUNNY).bytes < be.XCD_BYTES
    assert facts(be.SHINY) == facts(be.BUNNY)
    assert facts(be.SOUP).overlap > be.PACKET_OVERLAP and facts(be.SOUP).bytes < be.XCD_BYTES


def test_the_rule_gives_the_expected_class_and_every_frame_passes_check_frame(world, facts):
    seen = set()
    for number, name, call in all_calls(world):
        got = be.predict(call, facts)
        for k, (f, (cls, pipe)) in enumerate(zip(call, got)):
            assert (f.cls, f.pipeline) == (cls, pipe), (number, name, k, f.cls, f.pipeline, cls, pipe)
            assert be.frame_ok(facts(f.scene), f.params), (number, name, k)
            assert (f.pipeline == be.FUSED_HELD) == (f.cls == be.FUSED_CLASS) and (f.pipeline == be.PK_HELD) == (f.cls == be.PK_CLASS)
        seen.add(number)
    assert seen == {1, 2, 3, 4, 5, 6}


def test_held_frames_share_a_size_and_every_held_class_has_two_members(world):
    for number, name, call in all_calls(world):
        sizes = {be.local_size(f.params) for f in call if f.cls}
        assert len(sizes) == 1, (number, name, sizes)
        if number <= 4:      # (call 3 holds no fused frame: the records are over 32 MiB)
            for cls in (be.FUSED_CLASS, be.PK_CLASS):
                n = sum(1 for f in call if f.cls == cls)
                assert n >= 2 or (number == 3 and cls == be.FUSED_CLASS and n == 0), (number, name, cls, n)


def test_call_1_as_the_issue_words_it(world):
    n_calls = 0
    for (W, H) in be.EDGE_SIZES:
        calls = be.edge_calls(world, W, H)
        assert len(calls) == len(tm.edge_layouts(W, H)), "every layout of every edge size gives a share with rows and columns"
        for name, call in calls.items():
            n_calls += 1
            for cls, L in ((be.FUSED_CLASS, 2), (be.PK_CLASS, 16)):
                fs = [f for f in call if f.cls == cls]
                assert [f.params.n_lights for f in fs] == [L] * 3
                assert sum(1 for f in fs if f.params.flags & be.SMOOTH) == 1 and sum(1 for f in fs if f.params.flags & be.IN_FLIGHT) == 1
                lit = {(f.params.focal, f.params.shadow_div, f.params.reinhard, f.params.gamma, bytes(f.params.background)) for f in fs}
                assert len(lit) == 3 and len({f.params._lights.tobytes() for f in fs}) == 3, "own literals and own light inside one launch"
                if fs[0].params.block_cols:
                    assert len({f.params.block_first for f in fs}) == min(3, fs[0].params.block_stride), "a tile deal's frames differ in block_first"
            odd = [f for f in call if not f.cls]
            assert len(odd) == 1 and odd[0].pipeline == tm.FUSED and 0 < call.index(odd[0]) < len(call) - 1
            assert be.local_size(odd[0].params) != be.local_size(call[0].params) and (odd[0].params.width, odd[0].params.height) == (W, H)
    assert n_calls == 37      # nine sizes x (whole, two tile deals), every other row where H >= 2 (seven), blocks of eight rows where H > 8 (three)


def test_every_whole_frame_of_call_1_hits_geometry(world, oracle):
    for (W, H) in be.EDGE_SIZES:
        for f in be.edge_calls(world, W, H)["{}"]:
            if f.cls:
                assert (world.oracle(oracle, f.scene, f.params)["hit_id"] >= 0).any(), (W, H, f.params.focal)


# Tile deals of call 1 in which ONE frame of each class owns pixels: the frame lies inside one block of the deal, one block_first owns that
# block and the other frames of the class own padding only.  That frame sees a few pixels of the bunny's front, at most 3.4 units across,
# while one step of the light staircase moves a shadow's edge by more: its pixels are shadowed alike.  It is the frame lit from under the
# slab (be.EDGE_LIGHTS), so every pixel of these calls has blocked samples, and none is without.
DEAL_16, DEAL_8 = "{'block_rows': 8, 'block_cols': 16, 'block_stride': 3, 'block_first': 2}", "{'block_rows': 8, 'block_cols': 8, 'block_stride': 2, 'block_first': 1}"
ONE_OWNER = {(1, 1, DEAL_16), (1, 1, DEAL_8), (3, 2, DEAL_16), (3, 2, DEAL_8), (8, 8, DEAL_16), (8, 8, DEAL_8), (9, 7, DEAL_16)}


def shadow_evidence(world, oracle, call, cls):
    """(frames of the class that own a hit pixel, hit pixels with a blocked sample, hit pixels with none) over a call's frames of a class."""
    owners = n_blocked = n_free = 0
    for f in call:
        if f.cls == cls:
            hit, blk = blocked(world, oracle, f)
            owners += bool(hit.any()); n_blocked += int(blk.sum()); n_free += int((hit & ~blk).sum())
    return owners, n_blocked, n_free


def test_every_held_class_has_shadowed_and_unshadowed_hit_pixels(world, oracle):
    one_owner = set()
    for number, name, call in all_calls(world):
        if number == 5 and len(call) > 4:
            call = call[:3] + call[-1:]      # (the frames of a table call repeat three lights: the first three and the last stand for all)
        for cls in (be.FUSED_CLASS, be.PK_CLASS):
            if not any(f.cls == cls for f in call) or (number == 5 and len(call) == 1):
                continue
            owners, n_blocked, n_free = shadow_evidence(world, oracle, call, cls)
            if number == 1 and owners == 1:
                one_owner.add((call[0].params.width, call[0].params.height, name.split(" ", 1)[1]))
                assert n_blocked > 0, (name, cls)
                continue
            assert n_blocked > 0 and n_free > 0, (number, name, cls, owners, n_blocked, n_free)
    assert one_owner == ONE_OWNER


def test_the_unheld_frames_of_call_4_are_what_they_are_named(world, oracle):
    call = be.between_calls(world)["in place"]
    kinds = [(f.scene, f.params.n_lights, bool(f.params.ray_matrix), f.params.spp, bool(f.params.flags & be.COUNT), be.variant(f.params), f.cls) for f in call]
    assert kinds == [(be.BUNNY, 2, False, 1, False, 0, be.FUSED_CLASS), (be.BUNNY, 2, True, 1, False, 0, None), (be.BUNNY, 2, False, 1, False, 0, be.FUSED_CLASS),
                     (be.BUNNY, 2, False, 4, False, 0, None), (be.BUNNY, 2, False, 1, True, 0, None), (be.SOUP, 2, False, 1, False, 0, None),
                     (be.BUNNY, 16, False, 1, False, 0, be.PK_CLASS), (be.BUNNY, 16, False, 1, False, 64, be.PK_CLASS), (be.BUNNY, 2, False, 1, False, 0, None),
                     (be.BUNNY, 2, False, 1, False, 0, be.FUSED_CLASS)]
    assert be.local_size(call[8].params) == (33, 0) and call[8].pipeline == be.NOT_RENDERED
    orders = be.between_calls(world)
    assert orders["first"][0].params.width == 33 and orders["last"][-1].params.width == 33 and len(orders["first"]) == len(orders["last"]) == 10
    for f in call:
        if be.local_size(f.params)[1]:
            c = world.oracle(oracle, f.scene, f.params)
            hit = c["hit_id"] >= 0
            assert hit.sum() > 20 and (f.scene == be.SOUP or (~hit).any()), (f.scene, int(hit.sum()))
    c = world.oracle(oracle, be.BUNNY, call[0].params)
    seen = np.unique(world.flat(be.BUNNY)[0].tri_obj[c["hit_id"][c["hit_id"] >= 0]])
    assert list(seen) == [0, 1], "the bunny and the slab under it"


def test_the_table_calls_give_launches_of_36_1_and_1(world):
    got = {name: be.launches(be.table_call(world, name)) for name in be.TABLE_CALLS}
    assert got == {"36 fused": {"fused": [36], "pk": []}, "37 fused": {"fused": [36, 1], "pk": []}, "1 fused": {"fused": [1], "pk": []},
                   "37 pk": {"fused": [], "pk": [36, 1]}}
    for (W, H) in be.BOUNDARY_SIZES:
        for call in be.boundary_calls(world, W, H).values():
            assert be.launches(call) == {"fused": [2], "pk": [6]}, "L = 16 .. 129 in ONE packet launch"
            assert {(f.params.n_lights + 63) // 64 for f in call if f.cls == be.PK_CLASS} == {1, 2, 3}, "one, two and three shadow words per pixel side by side"
        assert [f.params.n_lights for f in be.boundary_calls(world, W, H)["reversed"]] == list(be.BOUNDARY_L)[::-1]


def test_call_6_mixes_the_shading_kernels_and_names_its_null_outputs(world):
    assert gf.int_shininess_only(world.flat(be.BUNNY)[0]) and not gf.int_shininess_only(world.flat(be.SHINY)[0])
    for L in be.NULLS_L:
        calls = be.nulls_calls(world, L)
        call, nulls, tables = calls["entries"]
        assert {f.scene for f in call} == {be.BUNNY, be.SHINY} and all(f.cls for f in call)
        assert sorted(nulls.values()) == [(be.HIT, be.T), (be.LIN,)] and tables == ()
        assert calls["t table"][2] == (be.T,)


