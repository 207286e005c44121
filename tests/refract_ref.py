"""The yardstick of refracting paths (include/srt.h, "Refracting paths": srt_shade_paths_refract and srt_render_paths_refract).  It adds no
arithmetic of its own except refract_dir, the header's formula in numpy float32 with one array operation per step:

  * a segment is what it is in every path yardstick: the winners, the shadow rays' candidate sets and surface_ref.surface (obj, the
    normal, the bounce row), collected by visibility_ref.trace's loop (visibility_ref.masked_walk, with another next ray) into
    shadow_rule_ref.Segment rows, so that masks (visibility_ref.visible / closest) and the shadow rule (shadow_rule_ref.shadow_bits) come
    in exactly as those files already compose them; without masks every ray kind sees every object;
  * segment b + 1's ray is segment b's bounce row, or -- where ior[obj] > 0 -- the same origin with refract_dir(d, normal, ior[obj]);
    the interval is (bounce_t_min, +inf) either way, and an ended path carries a zero ray and the interval (1, 0);
  * the mix is shade_path_ref.mix and the finish shade_path_ref.finish, through shadow_rule_ref.shade_paths_of.

tests/test_refract_ref.py pins a table without a positive entry to shade_path_ref.shade_paths bit for bit, and refract_dir to Snell's
law in float64."""
import numpy as np

import path_walk_ref as pw
import render_paths_ref as rpr
import shade_path_ref as sp
import surface_ref as sf
import visibility_ref as vr

F32 = np.float32
ALL = vr.ALL
MISS, MIRROR, ENTER, LEAVE, TIR = -1, 0, 1, 2, 3          # what a path does at the end of a segment (kinds())


def refract_steps(d, N, n):
    """The header's formula, row by row, with every step kept: dict of L, inv, I, c, entering, Nf, dv, eta, k, s, u, r (the refracted
    way, whatever k is) and out (what refract_dir returns).  d, N: m x 3 float32; n: m float32."""
    d, N = np.ascontiguousarray(d, np.float32).reshape(-1, 3), np.ascontiguousarray(N, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(n, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        inv = F32(1.0) / L
        I = d * inv[:, None]
        c = (N[:, 0] * I[:, 0] + N[:, 1] * I[:, 1]) + N[:, 2] * I[:, 2]
        entering = c < F32(0.0)
        Nf = np.where(entering[:, None], N, -N)
        dv = np.where(entering, c, -c)
        eta = np.where(entering, F32(1.0) / n, n)
        ee = eta * eta
        dd = dv * dv
        one_dd = F32(1.0) - dd
        k = F32(1.0) - ee * one_dd
        s = eta * dv + np.sqrt(k)
        eI = I * eta[:, None]
        sN = Nf * s[:, None]
        u = eI - sN
        r = u * L[:, None]
        out = np.where((k < F32(0.0))[:, None], sf.reflect(d, N), r)
    f = lambda a: a.astype(np.float32)
    return dict(L=f(L), inv=f(inv), I=f(I), c=f(c), entering=entering, Nf=f(Nf), dv=f(dv), eta=f(eta), k=f(k), s=f(s), u=f(u), r=f(r), out=f(out))


def refract_parts(d, N, n):
    """The header's formula, row by row: (r, entering, k).  d, N: m x 3 float32; n: m float32."""
    p = refract_steps(d, N, n)
    return p["out"], p["entering"], p["k"]


def refract_dir(d, N, n):
    """The direction of the next segment after a hit on a transmitting object: m x 3 float32."""
    return refract_parts(d, N, n)[0]


def assert_snell(d, N, r, n, entering, tol=1e-4):
    """Snell's law in float64 for the rows (d, N, n) -> r the formula refracted (k well above 0): against physics, not against the formula.
    The quantities compared are sines and cosines of unit vectors, so tol is both absolute and relative to 1; the length is compared
    relative to |d|."""
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    D, NN, R, n64 = (np.asarray(a, np.float32).astype(np.float64) for a in (d, N, r, n))
    NN = unit(NN)
    I = unit(D)
    cos_i = (I * NN).sum(axis=1)
    ent = cos_i < 0
    assert np.array_equal(ent, entering)
    eta = np.where(ent, 1.0 / n64, n64)
    Nf = np.where(ent[:, None], NN, -NN)
    Rh = unit(R)
    sin_i, sin_t = np.linalg.norm(np.cross(I, NN), axis=1), np.linalg.norm(np.cross(Rh, NN), axis=1)
    assert np.abs(sin_t - eta * sin_i).max() <= tol, "Snell's law"
    # in the plane of d and N: no component along I x N (where that axis exists), and on the far side of the tangent from I's
    axis = np.cross(I, NN)
    has = sin_i > 1e-3
    assert np.abs((Rh[has] * unit(axis[has])).sum(axis=1)).max() <= tol, "r leaves the plane of d and N"
    tang = I - cos_i[:, None] * NN
    bends = has & (eta * sin_i > tol)             # (a transmitted tangent below the tolerance may round to nothing in float32)
    assert ((Rh * tang).sum(axis=1)[bends] > 0).all(), "r bends to the wrong side of the normal"
    assert ((R * Nf).sum(axis=1) < 0).all(), "r does not go through the surface"
    len_r, len_d = np.linalg.norm(R, axis=1), np.linalg.norm(D, axis=1)
    assert (np.abs(len_r - len_d) / len_d).max() <= tol, "|r| is not |d|"
    # the answer itself: Snell's direction built in float64 from the angles
    cos_t = np.sqrt(1.0 - (eta * sin_i) ** 2)
    want = eta[:, None] * tang - cos_t[:, None] * Nf
    assert np.abs(Rh - unit(want)).max() <= tol


def next_rays(cur, s, ior):
    """The rays of the next segment: the bounce rows of surface_ref.surface `s` for the rays `cur`, with the refracted direction where
    the hit's object transmits.  Also what every ray does there (MISS, MIRROR, ENTER, LEAVE, TIR)."""
    nxt = np.ascontiguousarray(s["bounce"]).copy()                                # a miss row: the zero ray
    obj = s["obj"]
    kind = np.where(obj >= 0, MIRROR, MISS).astype(np.int8)
    ior = np.ascontiguousarray(ior, np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        glass = np.flatnonzero((obj >= 0) & (ior[np.maximum(obj, 0)] > F32(0.0)))
    if glass.size:
        r, entering, k = refract_parts(cur[glass, 3:6], s["normal"][glass], ior[obj[glass]])
        nxt[glass, 3:6] = r
        kind[glass] = np.where(k < F32(0.0), TIR, np.where(entering, ENTER, LEAVE))
    return nxt, kind


def trace(oracle, flat, rays, lights, depth, ior, vis=None, obj_mask=None, bounce_t_min=1e-3, t_range=None, flags=0, colours=None, cands=None):
    """visibility_ref.trace with the refracting next ray: (the Segments, what every ray does at the end of each).  vis None: all ones.
    colours None: the colours stay zero (the walks alone, for a case's input conditions); lights may then be empty."""
    cands = cands if cands is not None else vr.CandidateMemo(oracle, flat)
    vis = (ALL, ALL, ALL) if vis is None else vis
    kinds = []

    def refracting(cur, s):
        nxt, kind = next_rays(cur, s, ior)
        kinds.append(kind)
        return nxt
    return vr.masked_walk(oracle, flat, rays, lights, depth, vis, obj_mask, bounce_t_min, t_range, flags, colours, cands, refracting), kinds


def shade_paths(oracle, flat, rays, lights, depth, ior, reflectance=None, bounce_t_min=1e-3, t_range=None, flags=0, rule=None, vis=None, obj_mask=None,
                colours=None, cands=None, **literals):
    """srt_shade_paths_refract by the yardstick: dict of rgb_linear, rgb8 and the seg_* arrays (depth x n ...)."""
    lights = np.ascontiguousarray(lights, np.float32).reshape(-1, 3)
    colours = colours if colours is not None else vr.Colours(oracle, flat, lights, flags, **literals)
    segs, _ = trace(oracle, flat, rays, lights, depth, ior, vis, obj_mask, bounce_t_min, t_range, flags, colours, cands)
    return vr.shade_paths_of(oracle, flat, segs, depth, rule, reflectance, **literals)


def render_paths(oracle, flat, p, depth, ior, reflectance=None, bounce_t_min=1e-3, rule=None, vis=None, obj_mask=None, fill=None):
    """srt_render_paths_refract by the yardstick: render_paths_ref.compose_frame on the paths above, the candidate sets shared among the
    sub-samples."""
    memo = vr.CandidateMemo(oracle, flat)
    shade = lambda rays, lights, flags, **lit: shade_paths(oracle, flat, rays, lights, depth, ior, reflectance, bounce_t_min, flags=flags, rule=rule, vis=vis,
                                                           obj_mask=obj_mask, cands=memo, **lit)
    return rpr.compose_frame(oracle, p, shade, fill=fill)


# ---- the cases of tests/test_gpu_refract.py --------------------------------------------------------------------------------------------
# shade_path_ref.FRAMES' cameras, rays, lights (3) and reflectances; object 0 mirrors and every other object is glass of index 1.5.
# tests/test_refract_ref.py asserts on the yardstick that in every case some segment-0 hits mirror and some enter glass, that at some
# later segment some ray enters, some leaves and some is totally reflected, and that some ray misses segment 0.
DEPTHS = {"cubes4_a40": 4, "cube_ground": 4, "ground_bunny": 3}
N_LIGHTS, BOUNCE_T_MIN = sp.N_LIGHTS, sp.BOUNCE_T_MIN
GLASS = 1.5


def case_ior(flat):
    ior = np.full(flat.n_objects, GLASS, np.float32)
    ior[0] = 0.0
    return ior


def kind_counts(kinds):
    """Per segment walked: (mirror, enter, leave, tir, miss among the rays walked is not counted) as a dict."""
    return [{"mirror": int((k == MIRROR).sum()), "enter": int((k == ENTER).sum()), "leave": int((k == LEAVE).sum()), "tir": int((k == TIR).sum())} for k in kinds]


def condition(segs, kinds):
    """The input condition of a frame case, on the yardstick."""
    c = kind_counts(kinds)
    assert c[0]["mirror"] > 0 and c[0]["enter"] > 0, ("segment 0", c[0])
    assert (segs[0].hit < 0).any(), "no ray misses segment 0"
    assert any(k["enter"] > 0 and k["leave"] > 0 and k["tir"] > 0 for k in c[1:]), ("no later segment with entering, leaving and TIR", c)
    return c


_cases = pw.CaseCache()


def case_memo(oracle, name):
    return _cases.once(("memo", name), lambda: vr.CandidateMemo(oracle, sp.frame_case(name)[0]))


def case_colours(oracle, name):
    def make():
        flat, _, lights, _ = sp.frame_case(name)
        return vr.Colours(oracle, flat, lights)
    return _cases.once(("colours", name), make)


def case_walks(oracle, name):
    """The primary walks of a frame case (no lights, no colours): (segs, kinds), computed once."""
    def make():
        flat, rays, _, _ = sp.frame_case(name)
        return trace(oracle, flat, rays, np.zeros((0, 3), np.float32), DEPTHS[name], case_ior(flat), bounce_t_min=BOUNCE_T_MIN, cands=case_memo(oracle, name))
    return _cases.once(("walks", name), make)


def case_trace(oracle, name):
    """The full trace of a frame case: computed once, shared, never changed."""
    def make():
        flat, rays, lights, _ = sp.frame_case(name)
        return trace(oracle, flat, rays, lights, DEPTHS[name], case_ior(flat), bounce_t_min=BOUNCE_T_MIN, colours=case_colours(oracle, name), cands=case_memo(oracle, name))
    return _cases.once(("trace", name), make)


def case_reference(oracle, name, rule=None):
    """The yardstick's rows of a frame case under `rule`: computed once, shared, never changed."""
    def make():
        flat, _, _, refl = sp.frame_case(name)
        return vr.shade_paths_of(oracle, flat, case_trace(oracle, name)[0], DEPTHS[name], rule, refl)
    return _cases.once(("ref", name, pw.rule_key(rule)), make)
