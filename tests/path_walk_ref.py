"""What the path yardsticks (tests/shadow_rule_ref.py, visibility_ref.py, refract_ref.py, fresnel_ref.py) state once: the rows of one
segment (Segment, segment_of), the loop over the segments of a path (walk), and the memo of a case's costly parts (CaseCache).  No
arithmetic and no derivation of a winner lives here: every trace hands in how its winners, its surface rows, its shadow rays' candidates
and its next rays are found, and tests pin those derivations against one another.

tests/shade_path_ref.py's shade_paths keeps a loop of its own: it is the independent base the others are pinned to."""
from dataclasses import dataclass

import numpy as np

import ray_query_ref as rq
import ray_range_ref as rr

F32 = np.float32
INF = np.float32(np.inf)


@dataclass
class Segment:
    rays: np.ndarray              # n x 6: the rays the segment walked (a zero ray where the path has ended)
    going: np.ndarray             # n bool: the path was alive when the segment began
    hit: np.ndarray               # n int32
    t: np.ndarray                 # n float32
    obj: np.ndarray               # n int32
    sel: np.ndarray               # the rays that hit, in ray order
    colour: np.ndarray            # n_hit x n_lights x 3: every sample unshadowed (zeros when the trace was made without colours)
    srays: np.ndarray             # (n_lights * n_hit) x 6: the shadow rays, light-major
    cand: rr.Candidates           # their candidate sets
    skip: np.ndarray              # n_hit int64: the hit's object


def segment_of(flat, cur, going, hit, t, obj, lights, shadow_cands, colours):
    """The Segment of the rays `cur` with the winners (hit, t): the shadow rays of every hit towards every light (light-major), their
    candidate sets by shadow_cands(rays), the hit's object to skip, and the unshadowed colours by colours(cur, hit, t) (None: zeros)."""
    nl = lights.shape[0]
    sel = np.flatnonzero(hit >= 0)
    skip = flat.tri_obj[hit[sel]].astype(np.int64)
    srays = (np.concatenate([rq.shadow_rays(cur[sel], t[sel], lights[l]) for l in range(nl)]) if nl and sel.size else np.zeros((0, 6), np.float32))
    cand = shadow_cands(srays)
    colour = colours(cur, hit, t) if colours is not None else np.zeros((sel.size, nl, 3), np.float32)
    return Segment(np.where(going[:, None], cur, F32(0.0)), going, hit, t, obj, sel, colour, srays, cand, skip)


def bounce_interval(going, bounce_t_min):
    """The interval of a ray that leaves a hit, (bounce_t_min, +inf), and of a ray that stands for none, (1, 0): a miss by definition."""
    return np.stack([np.where(going, F32(bounce_t_min), F32(1.0)), np.where(going, INF, F32(0.0))], axis=1).astype(np.float32)


def mirror_rays(cur, s):
    """The next rays of a mirror path: the bounce rows of the surface (a miss row: the zero ray)."""
    return np.ascontiguousarray(s["bounce"])


def walk(rays, depth, *, winners, segment, surface, next_rays=mirror_rays, bounce_t_min=1e-3, t_range=None):
    """The segments of every path, one per segment walked (the walk stops when no path is alive):
    winners(b, cur, t_range) -> (hit, t) of segment b's rays; surface(cur, hit, t) -> surface_ref.surface's rows;
    segment(cur, going, hit, t, obj) -> what is kept of the segment; next_rays(cur, s) -> segment b + 1's rays."""
    cur = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    tr = None if t_range is None else np.ascontiguousarray(t_range, np.float32).reshape(-1, 2)
    going = np.ones(cur.shape[0], bool)
    segs = []
    for b in range(depth):
        if not going.any():
            break
        hit, t = winners(b, cur, tr)
        assert not (hit[~going] >= 0).any(), "an ended path hit something"
        s = surface(cur, hit, t)
        segs.append(segment(cur, going, hit, t, s["obj"]))
        going = hit >= 0
        cur = next_rays(cur, s)
        tr = bounce_interval(going, bounce_t_min)
    return segs


class CaseCache(dict):
    """What a case costs to compute, kept under a tuple: once(key, make) computes it on the first request, and a dict of arrays -- a
    reference -- is marked read-only as it goes in: computed once, shared, never changed."""

    def once(self, key, make):
        if key not in self:
            value = make()
            for a in value.values() if isinstance(value, dict) else ():
                a.setflags(write=False)
            self[key] = value
        return self[key]


def rule_key(rule):
    """A shadow rule as part of a key (NaN does not equal itself)."""
    return None if rule is None else tuple(str(v) for v in rule)
