"""The yardstick of mirror paths (include/srt.h, srt_shade_paths).  It adds no arithmetic of its own except the mix:

  * segment b is shade_range_ref.shade (hit_id, t, rgb_linear) plus surface_ref.surface (obj, the bounce row) on segment b's rays and
    intervals -- the yardsticks of srt_shade_rays_range and srt_surface_rays as they stand;
  * segment b + 1's rays are segment b's bounce rows, with the interval (bounce_t_min, +inf); a path that has ended carries a zero ray
    and the interval (1, 0), a miss by definition, so its rows are miss rows and nothing is rendered for it;
  * the mix is the header's loop in numpy float32, every multiply and add its own array operation;
  * rgb8: oracle.tonemap(pow="device") and the background rule, as shade_range_ref.compose does.

One tiny oracle render per hit and light: keep batches at a few hundred rays and at most 3 lights."""
import numpy as np

import shade_range_ref as sr
import surface_ref as sf
from path_walk_ref import CaseCache
from simple_raytracer_amd import abi

F32 = np.float32
INF = np.float32(np.inf)
SEG_KEYS = ("seg_hit_id", "seg_t", "seg_obj", "seg_rgb_linear", "seg_rays")
ALL_KEYS = ("rgb_linear", "rgb8") + SEG_KEYS


def mix(seg_hit, seg_obj, seg_lin, reflectance, dtype=np.float32):
    """The header's loop over the segments (depth x n ...), from the near end, in `dtype`: acc n x 3."""
    depth, n = seg_hit.shape
    acc = np.zeros((n, 3), dtype)
    W = np.ones(n, dtype)
    going = np.ones(n, bool)
    refl = None if reflectance is None else np.asarray(reflectance, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        for b in range(depth):
            going = going & (seg_hit[b] >= 0)
            nxt = going & (seg_hit[b + 1] >= 0) if b + 1 < depth else np.zeros(n, bool)
            k = np.zeros(n, dtype)
            if refl is not None:
                k[nxt] = refl[seg_obj[b][nxt]]
            a = (W * (dtype(1.0) - k)).astype(dtype)
            term = (a[:, None] * seg_lin[b].astype(dtype)).astype(dtype)
            acc = np.where(going[:, None], (acc + term).astype(dtype), acc)
            W = np.where(going, (W * k).astype(dtype), W)
    return acc


def shade_paths(oracle, flat, rays, lights, depth, reflectance=None, bounce_t_min=1e-3, t_range=None, flags=0, **literals):
    """srt_shade_paths by the yardstick: dict of rgb_linear, rgb8 and the seg_* arrays (depth x n ...)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    n = rays.shape[0]
    smooth = bool(flags & abi.SRT_FLAG_SMOOTH_NORMALS)
    out = {"seg_hit_id": np.full((depth, n), -1, np.int32), "seg_t": np.full((depth, n), INF, np.float32), "seg_obj": np.full((depth, n), -1, np.int32),
           "seg_rgb_linear": np.zeros((depth, n, 3), np.float32), "seg_rays": np.zeros((depth, n, 6), np.float32)}
    cur = rays
    tr = None if t_range is None else np.ascontiguousarray(t_range, np.float32).reshape(-1, 2)
    going = np.ones(n, bool)
    for b in range(depth):
        if not going.any():
            break
        hit, t, lin, _ = sr.shade(oracle, flat, cur, lights, t_range=tr, flags=flags, **literals)
        assert not (hit[~going] >= 0).any(), "an ended path hit something"
        s = sf.surface(oracle, flat, cur, hit, t, smooth)
        out["seg_hit_id"][b], out["seg_t"][b], out["seg_obj"][b], out["seg_rgb_linear"][b] = hit, t, s["obj"], lin
        out["seg_rays"][b] = np.where(going[:, None], cur, F32(0.0))
        going = hit >= 0
        cur = np.ascontiguousarray(s["bounce"])                                  # a miss row: the zero ray
        tr = np.stack([np.where(going, F32(bounce_t_min), F32(1.0)), np.where(going, INF, F32(0.0))], axis=1).astype(np.float32)
    out["rgb_linear"], out["rgb8"] = finish(oracle, out, reflectance, **literals)
    return out


def finish(oracle, seg, reflectance, reinhard=0.5, gamma=1.1, background=abi.REFERENCE_BACKGROUND, lin=None, **_):
    """(rgb_linear, rgb8) of the per-segment rows `seg` under a reflectance table: the mix (or `lin`, rows mixed otherwise), then tone map,
    quantiser and background rule as shade_range_ref.compose applies them (a ray whose segment 0 misses is not tone-mapped: it is the
    background)."""
    if lin is None:
        lin = mix(seg["seg_hit_id"], seg["seg_obj"], seg["seg_rgb_linear"], reflectance)
    _, q = oracle.tonemap(lin, reinhard, gamma, pow="device")
    q = q.copy()
    q[seg["seg_hit_id"][0] < 0] = 0
    q[np.all(q == 0, axis=1)] = np.asarray(background[:3], np.int32)
    return lin, q.astype(np.uint8)


# The frames of tests/test_gpu_shade_paths.py: (camera origin, target, focal) -- look_at cameras aimed down at the ground beside an
# object (cubes4_a40: into the gap between the cubes), so that some paths bounce between the two; tests/test_shade_path_ref.py checks
# the input condition of each on the yardstick.
FRAMES = {"cube_ground": ((-430.0, 0.0, 353.0), (-120.0, 105.0, 364.0), 88.0, (48, 27)),
          "cubes4_a40": ((98.0, -28.0, 10.0), (-9.0, 0.0, 105.0), 135.0, (48, 27)),
          "ground_bunny": ((-334.0, 52.0, 221.0), (-84.0, 120.0, 241.0), 72.0, (64, 36))}
DEPTH, N_LIGHTS, BOUNCE_T_MIN = 3, 3, 1e-3
REFLECTANCE = (0.6, 0.25, 0.4, 0.8)


def frame_case(name):
    """(flat, rays, lights, reflectance) of a frame case."""
    import golden_util as gu
    import ray_query_ref as rq
    import shade_query_ref as sq
    g = gu.GoldenScene(name)
    o, target, focal, (w, h) = FRAMES[name]
    rays = rq.frame_rays(w, h, sr.look_at(o, target), focal)
    refl = np.float32(REFLECTANCE[:int(g.flat.tri_obj.max()) + 1])
    return g.flat, rays, sq.lights_for(name, g.light, N_LIGHTS), refl


_cases = CaseCache()


def frame_reference(oracle, name):
    """The yardstick's rows of a frame case: computed once, shared, never changed."""
    def make():
        flat, rays, lights, refl = frame_case(name)
        return shade_paths(oracle, flat, rays, lights, DEPTH, refl, BOUNCE_T_MIN)
    return _cases.once(name, make)


def condition(ref):
    """The input condition of a case, on the yardstick: some path hits in every segment, some path ends by a miss at every segment >= 1,
    some ray misses segment 0."""
    hit = ref["seg_hit_id"] >= 0
    depth = hit.shape[0]
    assert hit.all(axis=0).any(), "no path hits in every segment"
    assert (~hit[0]).any(), "no ray misses segment 0"
    for b in range(1, depth):
        assert (hit[:b].all(axis=0) & ~hit[b]).any(), f"no path ends by a miss at segment {b}"


def assert_same(got, want, what, keys=ALL_KEYS):
    sf.assert_same(got, want, what, [k for k in keys if k in want])
