"""GPU (-m gpu): srt_render_device_batch at the frame edges and light-count boundaries every single-frame chain is pinned at -- the calls
of tests/batch_edges.py, whose properties tests/test_batch_edges_ref.py proves on the CPU.  They reach the kernels no single render runs
(k_trace_nq_batch's ROW_Z build, k_closest_hit_nq_batch, k_shadow_pk_batch, k_shade_tile_batch) and the host rules around them
(plan_frame's hold rule, BatchCollector, the launches of FRAME_TAB_MAX frames in render_device_batch_impl).

Every call goes through lib.FrameBatch over handles shared from one device scene per scene, into gpu_frames.PinnedFrame buffers
(sentinels, one guard row).  Every frame of every call is
  * the oracle's, at both bars of test_gpu_modes.World.check (gpu_frames.compare; compare_exact against the oracle with the device's pow);
  * untouched in its padding and guard row, and in every output the call passed as NULL;
  * counted like the oracle's frame by srt_sync (primary, hit and shadow rays, rows; a counting frame also in its node and triangle tests);
  * labelled by srt_scene_pipeline as the case table says, " (batched)" exactly where the restated hold rule holds the frame;
  * bit for bit the same params rendered alone on a spare shared handle.
No tolerance is introduced here."""
import numpy as np
import pytest

import batch_edges as be
import gpu_frames as gf
import test_gpu_modes as tm
from test_gpu_tree_shapes import WORK

pytestmark = pytest.mark.gpu
OUTPUTS = ("hit_id", "t", "rgb_linear", "rgb8")      # in the order of srt_render_device_batch's tables (be.HIT, be.T, be.LIN, be.RGB8)
COUNTED = ("primary_rays", "hit_rays", "shadow_rays", "rows")


@pytest.fixture(scope="module")
def srt():
    from simple_raytracer_amd import lib
    lib.load()
    return lib


class Pool(tm.World):
    """test_gpu_modes.World, and per scene one spare handle shared from its device scene: what renders a frame alone."""

    def __init__(self, srt):
        super().__init__(srt)
        self.spares = {}

    def spare(self, scene):
        if scene not in self.spares:
            self.spares[scene] = self.ds(scene).share()
        return self.spares[scene]

    def close(self):
        for h in list(self.spares.values()) + list(self.scenes.values()):
            h.close()


@pytest.fixture(scope="module")
def world(srt):
    w = be.prepare(Pool(srt))
    yield w
    w.close()


def same_frame(got, want, live, what):
    assert np.array_equal(got["hit_id"][live], want["hit_id"][live]), f"{what}: hit ids"
    assert np.array_equal(gf.bits(got["t"][live]), gf.bits(want["t"][live])), f"{what}: t"
    assert np.array_equal(gf.bits(got["rgb_linear"][live]), gf.bits(want["rgb_linear"][live])), f"{what}: rgb_linear"
    assert np.array_equal(got["rgb8"][live], want["rgb8"][live]), f"{what}: rgb8"
    for key in COUNTED:
        assert got["stats"][key] == want["stats"][key], (what, key, got["stats"][key], want["stats"][key])


def check_frame(srt, oracle, world, f, h, b, st, missing, what):
    """One frame of a call that has been rendered and synchronised: see the module's docstring.  Returns the frame's outputs."""
    p = f.params
    own = gf.owned(p)
    assert h.pipeline == f.pipeline, (what, h.pipeline, f.pipeline)
    b.check_untouched(own, what)
    for k, (a, s) in enumerate(((b.hit, gf.SENTINEL_HIT), (b.t, gf.SENTINEL_F32), (b.lin, gf.SENTINEL_F32), (b.rgb8, gf.SENTINEL_U8))):
        assert k not in missing or (a == s).all(), f"{what}: {OUTPUTS[k]} was passed as NULL and its buffer was written"
    got = b.out()
    got["stats"] = st
    if own.shape[0] == 0:
        assert all(st[key] == 0 for key in COUNTED), (what, st)      # nothing launched, nothing pending: an idle handle reports zero rays
        return got
    alone, pipe = gf.render_pinned(srt, world.spare(f.scene), p)
    assert pipe == f.pipeline.replace(" (batched)", ""), (what, pipe)
    for k in missing:
        got[OUTPUTS[k]] = alone[OUTPUTS[k]]      # an output the call did not ask for: the lone render's, which meets the same two bars itself
    if missing:
        world.check(srt, oracle, f.scene, alone, p, what + " alone")
    c = world.check(srt, oracle, f.scene, got, p, what)
    assert st["rows"] == c["stats"]["rows"] == own.shape[0], (what, st["rows"])
    if p.flags & be.COUNT:
        for key in WORK:
            assert st[key] == c["stats"][key], (what, key, st[key], c["stats"][key])
        assert c["stats"]["node_tests_primary"] > 0
    same_frame(got, alone, own >= 0, what + " against the frame alone")
    return got


def run_call(srt, oracle, world, call, what, handles=None, nulls=None, null_tables=()):
    """Renders a call and checks every frame of it; returns the frames' outputs.  handles: the call's handles (left open); else fresh ones."""
    L = srt.load()
    nulls = nulls or {}
    mine = handles is None
    if mine:
        handles = [world.ds(f.scene).share() for f in call]
    bufs = []
    try:
        for f in call:
            cols, rows = be.local_size(f.params)
            bufs.append(gf.PinnedFrame(L, rows, cols))
        tables = [None if k in null_tables else [0 if k in nulls.get(i, ()) else b.ptrs[k] for i, b in enumerate(bufs)] for k in range(4)]
        srt.FrameBatch(handles, [f.params for f in call], *tables).render()
        stats = [h.sync() for h in handles]
        return [check_frame(srt, oracle, world, f, h, b, st, set(null_tables) | set(nulls.get(i, ())), f"{what} frame {i} (L {f.params.n_lights})")
                for i, (f, h, b, st) in enumerate(zip(call, handles, bufs, stats))]
    finally:
        for b in bufs:
            b.free()
        if mine:
            for h in handles:
                h.close()


def test_the_scenes_facts_are_the_librarys(srt, world):
    """The overlap estimate and the record bytes the restated rule is fed with (tests/batch_edges.py) are what the handles report."""
    for scene in (be.BUNNY, be.SHINY, be.BIG, be.SOUP):
        facts, ds = be.scene_facts(world.flat(scene)[0]), world.ds(scene)
        assert abs(ds.overlap_estimate - facts.overlap) <= 1e-9 * facts.overlap, (scene, ds.overlap_estimate, facts.overlap)
        assert ds.device_bytes == facts.bytes == world.spare(scene).device_bytes, (scene, ds.device_bytes, facts.bytes)


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", be.EDGE_SIZES)
def test_frame_edges_in_both_held_classes(srt, oracle, world, W, H):
    """Per layout one call: three frames of L = 2 and three of L = 16 in one launch each, own lights and literals, smooth normals, the
    in-flight hint, block_first 0, 1, 2 of a tile deal side by side; a frame of another local size comes out unbatched and correct."""
    for name, call in be.edge_calls(world, W, H).items():
        outs = run_call(srt, oracle, world, call, f"{W}x{H} {name}")
        if name == "{}":
            assert all((o["hit_id"] >= 0).any() for o in outs), "every whole frame hits geometry"


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("forward", "reversed"))
@pytest.mark.parametrize("W,H", be.BOUNDARY_SIZES)
def test_light_count_boundaries_in_one_launch(srt, oracle, world, W, H, order):
    """L = 0 | 1, 7 | 8, 15 | 16 .. 129 in one call: frames of one, two and three shadow words per pixel in ONE packet launch whose waves
    are sized from max_lights = 129; reversed, max_lights is known from the first held frame and the smallest list comes last."""
    run_call(srt, oracle, world, be.boundary_calls(world, W, H)[order], f"{W}x{H} {order}")


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", be.BIG_SIZES)
def test_held_packet_frames_below_16_samples_on_a_scene_over_32_mib(srt, oracle, world, W, H):
    """main_nocats: the estimate of 17 puts 8 and 15 samples into the held packet class, the 35 MiB of records set xcd_rows in every
    frame's DevParams -- the batch kernels are built without the row deal and must not read it -- and keep the L = 3 frames out of the
    fused class: they run the XCD-row build of k_trace_nq inside the batch call."""
    assert world.ds(be.BIG).device_bytes > be.XCD_BYTES and world.ds(be.BIG).overlap_estimate >= be.MID_OVERLAP
    run_call(srt, oracle, world, be.big_call(world, W, H), f"{be.BIG} {W}x{H}")


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("in place", "first", "last"))
def test_frames_a_batch_must_not_hold_between_frames_it_holds(srt, oracle, world, order):
    """Camera, spp = 4, counting, packet closest hit, a share that owns no rows: launched as they come (or not at all) between, before and
    behind held frames.  The no-rows frame writes nothing and reports zero rays; variant 64 is held, as the rule says."""
    call = be.between_calls(world)[order]
    outs = run_call(srt, oracle, world, call, f"between, the no-rows frame {order}")
    empty = [o for f, o in zip(call, outs) if be.local_size(f.params)[1] == 0]
    assert len(empty) == 1 and empty[0]["hit_id"].shape == (0, 33)


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(be.TABLE_CALLS))
def test_table_lengths_at_a_ragged_size(srt, oracle, world, name):
    """9 x 7: launches of 36, 36 + 1 and 1 frames of the fused class, 36 + 1 of the packet class -- grids of (2, held, 1)."""
    call = be.table_call(world, name)
    assert sum(be.launches(call).values(), []) in ([36], [36, 1], [1])
    run_call(srt, oracle, world, call, name)


def test_a_call_of_no_frames_touches_nothing(srt, world):
    """n = 0 with tables that name a handle and buffers all the same: SRT_OK, the buffers keep their sentinels, the handle stays idle."""
    f = be.table_call(world, "1 fused")[0]
    srt.FrameBatch([], []).render()
    h = world.ds(f.scene).share()
    cols, rows = be.local_size(f.params)
    b = gf.PinnedFrame(srt.load(), rows, cols)
    try:
        fb = srt.FrameBatch([h], [f.params], *[[b.ptrs[k]] for k in range(4)])
        fb.n = 0
        fb.render()
        st = h.sync()
        assert h.pipeline == be.NOT_RENDERED and all(st[key] == 0 for key in COUNTED), (h.pipeline, st)
        b.check_untouched(np.full((rows, cols), -1), "n = 0")
    finally:
        b.free()
        h.close()


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("entries", "t table"))
@pytest.mark.parametrize("L", be.NULLS_L)
def test_mixed_shading_kernels_and_null_outputs(srt, oracle, world, L, name):
    """A shininess of 64.5 on two of the four handles: batch_int_shin is false and the golden frames take the general shading kernel too.
    hit_id and t entries, an rgb_linear entry and the whole t table passed as NULL: the workspace stands in, the other outputs are right."""
    call, nulls, tables = be.nulls_calls(world, L)[name]
    run_call(srt, oracle, world, call, f"L {L} {name}", nulls=nulls, null_tables=tables)


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------
def test_the_same_handles_through_two_different_calls(srt, oracle, world):
    """The 64 x 48 boundary call, the 1 x 1 edge call on its first handles, the boundary call again: workspaces and quadrant lists shrink and
    regrow, the counter sets alternate, the second big call starts from the heavy lists of the first.  First and third are the same bits."""
    big, small = be.boundary_calls(world, 64, 48)["forward"], be.edge_calls(world, 1, 1)["{}"]
    handles = [world.ds(be.BUNNY).share() for _ in big]
    try:
        first = run_call(srt, oracle, world, big, "first", handles=handles)
        run_call(srt, oracle, world, small, "1x1 between", handles=handles[:len(small)])
        third = run_call(srt, oracle, world, big, "third", handles=handles)
        for k, (a, b) in enumerate(zip(first, third)):
            same_frame(b, a, np.ones(a["hit_id"].shape, bool), f"third against first, frame {k}")
    finally:
        for h in handles:
            h.close()
