"""The yardstick of shaded paths under a shadow rule (include/srt.h, "Shadow rays with an end": srt_shade_paths_shadow and
srt_render_paths_shadow).  It adds no arithmetic: every number comes from a helper that already pins an existing call.

  * Per segment.  The winners are shade_range_ref.winners.  The unshadowed colour of every (hit, light) is the single-triangle reduction
    shade_range_ref.samples performs.  The shadowed bit of (hit, light) under a rule (t_min, t_max, self_shadow) is
    ray_range_ref.occluded on the candidates of the shadow ray so -> L - so (ray_query_ref.shadow_rays: so = o + d * t, d * t first), with
    the interval (t_min, t_max) for every ray and skip_obj = -1 (self_shadow) or the hit's object -- the header's definition, word for
    word.  Rule None is the reference's rule: nothing bounds t and the hit's object is skipped (the bits shade_range_ref.samples itself
    returns; asserted equal).  The sum is shade_range_ref.compose.
  * Paths.  The loop of shade_path_ref.shade_paths: surface_ref.surface gives obj and the bounce, a mirrored ray's interval is
    (bounce_t_min, +inf), an ended path carries a zero ray and the interval (1, 0); shade_path_ref.finish mixes.
  * Frames.  What render_paths_ref.render_paths does for srt_render_paths -- the rays of the owned pixels per sub-sample, the mixed sums
    added in sub-sample order, divided by float32(spp), tone-mapped once -- on the paths above.

Neither the walk nor a colour depends on the rule: trace() computes the segments, the colours and the candidates of the shadow rays once,
and shade_paths_of() composes them under any number of rules.  One tiny oracle render per hit and light: keep batches at the sizes of
shade_path_ref.FRAMES and at most 3 lights."""
import numpy as np

import path_walk_ref as pw
import ray_range_ref as rr
import render_paths_ref as rpr
import shade_path_ref as sp
import shade_range_ref as sr
import surface_ref as sf
from simple_raytracer_amd import abi

INF = np.float32(np.inf)
NAN = np.float32(np.nan)

# the two rules of the GPU tests, and the intervals that change nothing at flags = 0
SELF = (1e-3, 1.0, True)
ENDED = (1e-3, 1.0, False)
IDENTITIES = {"(0, inf)": (0.0, INF, False), "(-inf, inf)": (-INF, INF, False), "(NaN, NaN)": (NAN, NAN, False)}
NO_SHADOWS = (2.0, 1.0, False)         # t_min > t_max: nothing is in range
Segment = pw.Segment                   # (the rows of a segment live beside the walk that builds them)


def shadow_bits(flat, seg, rule):
    """n_hit x n_lights bool: the sample is shadowed under `rule` (None: the reference's rule)."""
    nh = seg.sel.size
    nl = seg.cand.n_rays // nh if nh else 0
    if nh == 0 or nl == 0:
        return np.zeros((nh, nl), bool)
    if rule is None:
        tr, skip = None, np.tile(seg.skip, nl)
    else:
        t_min, t_max, self_shadow = rule
        tr = np.tile(np.array([t_min, t_max], np.float32), (seg.cand.n_rays, 1))
        skip = np.full(seg.cand.n_rays, -1, np.int64) if self_shadow else np.tile(seg.skip, nl)
    return rr.occluded(seg.cand, flat, tr, skip).reshape(nl, nh).T.astype(bool)


def trace(oracle, flat, rays, lights, depth, bounce_t_min=1e-3, t_range=None, flags=0, colours=True, **literals):
    """The segments of every path (a list of Segment, one per segment walked): shade_path_ref.shade_paths' loop without the sums, the
    winners and the candidates straight from the oracle.  colours = False leaves the oracle renders out (the bits alone: for looking at a
    case's input conditions)."""
    lights = np.ascontiguousarray(lights, np.float32).reshape(-1, 3)
    smooth = bool(flags & abi.SRT_FLAG_SMOOTH_NORMALS)

    def segment(cur, going, hit, t, obj):
        seg = pw.segment_of(flat, cur, going, hit, t, obj, lights, lambda srays: rr.candidates(oracle, flat, srays), None)
        if colours:
            seg.colour, reference_bits = sr.samples(oracle, flat, cur, hit, t, lights, flags, **literals)
            assert np.array_equal(reference_bits, shadow_bits(flat, seg, None)), "rule None is not the reference's rule"
        return seg
    return pw.walk(rays, depth, winners=lambda b, cur, tr: sr.winners(oracle, flat, cur, tr), segment=segment,
                   surface=lambda cur, hit, t: sf.surface(oracle, flat, cur, hit, t, smooth), bounce_t_min=bounce_t_min, t_range=t_range)


def shade_paths_of(oracle, flat, segs, depth, rule=None, reflectance=None, bits=None, **literals):
    """srt_shade_paths_shadow of a trace under `rule`: dict of rgb_linear, rgb8 and the seg_* arrays (depth x n ...).
    bits: the shadowed bits per segment to use instead of the rule's (a list of n_hit x n_lights bool)."""
    n = segs[0].hit.shape[0]
    out = {"seg_hit_id": np.full((depth, n), -1, np.int32), "seg_t": np.full((depth, n), INF, np.float32), "seg_obj": np.full((depth, n), -1, np.int32),
           "seg_rgb_linear": np.zeros((depth, n, 3), np.float32), "seg_rays": np.zeros((depth, n, 6), np.float32)}
    for b, seg in enumerate(segs[:depth]):
        lin, _ = sr.compose(oracle, seg.hit, seg.colour, shadow_bits(flat, seg, rule) if bits is None else bits[b], **literals)
        out["seg_hit_id"][b], out["seg_t"][b], out["seg_obj"][b], out["seg_rgb_linear"][b], out["seg_rays"][b] = seg.hit, seg.t, seg.obj, lin, seg.rays
    out["rgb_linear"], out["rgb8"] = sp.finish(oracle, out, reflectance, **literals)
    return out


def shade_paths(oracle, flat, rays, lights, depth, reflectance=None, bounce_t_min=1e-3, t_range=None, flags=0, rule=None, **literals):
    """srt_shade_paths_shadow by the yardstick (shade_path_ref.shade_paths with one more argument)."""
    segs = trace(oracle, flat, rays, lights, depth, bounce_t_min, t_range, flags, **literals)
    return shade_paths_of(oracle, flat, segs, depth, rule, reflectance, **literals)


def render_paths(oracle, flat, p, depth, reflectance=None, bounce_t_min=1e-3, rule=None, fill=None):
    """srt_render_paths_shadow by the yardstick: render_paths_ref.compose_frame with the paths above.  Lights, literals and flags are p's."""
    shade = lambda rays, lights, flags, **lit: shade_paths(oracle, flat, rays, lights, depth, reflectance, bounce_t_min, flags=flags, rule=rule, **lit)
    return rpr.compose_frame(oracle, p, shade, fill=fill)


# ---- the cases of tests/test_gpu_shadow_rule.py ----------------------------------------------------------------------------------------
# shade_path_ref.FRAMES' cameras and frames, with a LAMP inside the scene instead of the far light (3 samples: abi.light_staircase):
# cubes4_a40 -- in the gap between the four cubes; cube_ground -- beside the cube, on the side away from the camera; ground_bunny -- between
# the bunny and the ground.  tests/test_shadow_rule_ref.py asserts on the yardstick that each case has an occluder beyond the lamp, a
# self-shadowed sample, and a pixel the rule changes through a bounce alone.
LAMPS = {"cube_ground": (120.0, 60.0, 330.0),
         "cubes4_a40": (-10.0, 0.0, 110.0),
         "ground_bunny": (-150.0, 100.0, 260.0)}
DEPTH, N_LIGHTS, BOUNCE_T_MIN = sp.DEPTH, sp.N_LIGHTS, sp.BOUNCE_T_MIN


def lamp_case(name):
    """(flat, rays, lights, reflectance) of a case: shade_path_ref.frame_case with the lamp's samples."""
    flat, rays, _, refl = sp.frame_case(name)
    return flat, rays, abi.light_staircase(np.asarray(LAMPS[name], np.float32), N_LIGHTS), refl


_cases = pw.CaseCache()


def case_trace(oracle, name):
    """The trace of a case: computed once, shared, never changed."""
    def make():
        flat, rays, lights, _ = lamp_case(name)
        return trace(oracle, flat, rays, lights, DEPTH, BOUNCE_T_MIN)
    return _cases.once(("trace", name), make)


def case_reference(oracle, name, rule):
    """The yardstick's rows of a case under `rule`: computed once, shared, never changed."""
    def make():
        flat, _, _, refl = lamp_case(name)
        return shade_paths_of(oracle, flat, case_trace(oracle, name), DEPTH, rule, refl)
    return _cases.once(("ref", name, pw.rule_key(rule)), make)


def conditions(flat, segs, ref_none, ref_self):
    """The input conditions of a case, on the yardstick (counts; every one must be > 0):
    beyond  -- (hit, light) pairs shadowed under the reference's rule and lit under (t_min, 1): the occluder is beyond the lamp;
    own     -- pairs lit under the reference's rule and shadowed under SELF: the hit object shadows itself;
    bounce  -- rays whose segment-0 sum is the same under rule None and SELF and whose mixed rgb8 differs: the rule shows through a
               segment >= 1 alone."""
    beyond = sum(int((shadow_bits(flat, s, None) & ~shadow_bits(flat, s, ENDED)).sum()) for s in segs)
    own = sum(int((~shadow_bits(flat, s, None) & shadow_bits(flat, s, SELF)).sum()) for s in segs)
    same0 = (sf.bits(ref_none["seg_rgb_linear"][0]) == sf.bits(ref_self["seg_rgb_linear"][0])).all(axis=1)
    bounce = int((same0 & (ref_none["rgb8"] != ref_self["rgb8"]).any(axis=1)).sum())
    return {"beyond": beyond, "own": own, "bounce": bounce}
