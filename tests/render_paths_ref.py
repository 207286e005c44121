"""The yardstick of mirror paths in a frame (include/srt.h, srt_render_paths).  It adds two things to tests/shade_path_ref.py, neither of
them arithmetic on colours beyond the header's spp rule:

  * frame_rays_owned(p): the rays of the LOCAL pixels of a call with params p, in numpy float32 -- which image pixel a local pixel is comes
    from abi.owned_pixels (the block and the tile deal), the direction is (i, j, focal) with i = x + (int)(-W / 2), j = y + (int)(-H / 2)
    plus the sub-pixel offset of sub-sample k, taken through the ray matrix with the oracle's association (M0 * dx + M1 * dy) + M2 * dz, or
    left as it stands without one.  Every arithmetic step is its own float32 array operation, so nothing is contracted.
  * compose_frame(...): a path yardstick on those rays, per sub-sample, and the header's rule for spp > 1: the mixed sums added in
    sub-sample order starting from sub-sample 0's, divided by float32(spp), tone-mapped once whatever was hit; seg reports sub-sample 0.
    render_paths(...) is that with shade_path_ref.shade_paths; the other path yardsticks compose their frames with it too.

Padding pixels (owned_pixels == -1) carry no ray: their rows are left out of the oracle's batch and come back as `fill`."""
import numpy as np

import shade_path_ref as sp
from path_walk_ref import CaseCache
from simple_raytracer_amd import abi

F32 = np.float32


def owned(p):
    """abi.owned_pixels of a call's params: [rows_local, cols_local] image pixel, -1 = padding."""
    return abi.owned_pixels(p.width, p.height, p.block_rows, p.block_first, p.block_stride, p.block_cols)


def matrix_of(p):
    """The 16 floats of p.ray_matrix, or None."""
    return np.ctypeslib.as_array(p.ray_matrix, shape=(16,)).copy() if p.ray_matrix else None


def sub_offsets(spp, k):
    """The offsets of sub-sample k of an m x m grid, as float32: ((k % m) + 0.5) / m - 0.5 and ((k / m) + 0.5) / m - 0.5."""
    if spp == 1:
        return F32(0.0), F32(0.0)
    m = int(round(spp ** 0.5))
    assert m * m == spp
    a = F32(F32(k % m) + F32(0.5))
    b = F32(F32(k // m) + F32(0.5))
    a = F32(a / F32(m))
    b = F32(b / F32(m))
    return F32(a - F32(0.5)), F32(b - F32(0.5))


def frame_rays_owned(p, k=0):
    """(rays [rows_local, cols_local, 6] float32, live [rows_local, cols_local] bool) of sub-sample k of a call with params p; the ray of
    a padding pixel is zero."""
    own = owned(p)
    live = own >= 0
    W, H = int(p.width), int(p.height)
    x = np.where(live, own % W, 0)
    y = np.where(live, own // W, 0)
    i0, j0 = int(-F32(W) / 2), int(-F32(H) / 2)               # (int)(-(float)W / 2): truncation
    sx, sy = sub_offsets(int(p.spp), k)
    dx = (i0 + x).astype(np.float32)
    dy = (j0 + y).astype(np.float32)
    dx = dx + sx
    dy = dy + sy
    dz = np.full(own.shape, F32(p.focal), np.float32)
    rays = np.zeros(own.shape + (6,), np.float32)
    M = matrix_of(p)
    if M is None:
        rays[..., 3], rays[..., 4], rays[..., 5] = dx, dy, dz
    else:
        m = np.ascontiguousarray(M, np.float32).reshape(4, 4)    # m[c] = column c
        for a in range(3):
            rays[..., a] = m[3, a]
            p0 = m[0, a] * dx
            p1 = m[1, a] * dy
            p2 = m[2, a] * dz
            s0 = p0 + p1
            rays[..., 3 + a] = s0 + p2
    rays[~live] = F32(0.0)
    return rays, live


def lights_of(p):
    return np.ctypeslib.as_array(p.light_pos, shape=(int(p.n_lights), 3)).copy() if p.n_lights else np.zeros((0, 3), np.float32)


def compose_frame(oracle, p, shade, keys=sp.ALL_KEYS, leading=lambda key: key.startswith("seg_"), fill=None):
    """The frame of a call with params p by the header's rule: shade(rays, lights, flags, **literals) -> a yardstick dict for the rays of
    the owned pixels, per sub-sample; the mixed sums added in sub-sample order starting from sub-sample 0's, divided by float32(spp),
    tone-mapped once whatever was hit, the background rule; the other rows are sub-sample 0's.  Every key of `keys` is scattered into
    [rows, cols, ...] -- behind a leading depth axis where leading(key) -- and padding pixels hold `fill` (default 0).  Lights, literals and
    flags are p's."""
    own = owned(p)
    sel = np.flatnonzero((own >= 0).reshape(-1))
    lit = dict(shadow_div=float(p.shadow_div), reinhard=float(p.reinhard), gamma=float(p.gamma), background=tuple(int(c) for c in p.background[:3]))
    flags = int(p.flags) & abi.SRT_FLAG_SMOOTH_NORMALS
    spp = int(p.spp)
    first, total = None, None
    for k in range(spp):
        rays, _ = frame_rays_owned(p, k)
        o = shade(rays.reshape(-1, 6)[sel], lights_of(p), flags, **lit)
        if k == 0:
            first, total = o, o["rgb_linear"].copy()
        else:
            total = (total + o["rgb_linear"]).astype(np.float32)
    if spp > 1:
        with np.errstate(all="ignore"):
            lin = (total / F32(spp)).astype(np.float32)
        _, q = oracle.tonemap(lin, lit["reinhard"], lit["gamma"], pow="device")
        q = q.copy()
        q[np.all(q == 0, axis=1)] = np.asarray(lit["background"], np.int32)
        first = dict(first, rgb_linear=lin, rgb8=q.astype(np.uint8))
    out = {}
    for key in keys:
        v = first[key]
        lead = v.shape[:1] if leading(key) else ()
        tail = v.shape[len(lead) + 1:]
        full = np.zeros(lead + (own.size,) + tail, v.dtype) if fill is None else np.full(lead + (own.size,) + tail, fill, v.dtype)
        full[(slice(None),) * len(lead) + (sel,)] = v
        out[key] = full.reshape(lead + own.shape + tail)
    return out


def render_paths(oracle, flat, p, depth, reflectance=None, bounce_t_min=1e-3, fill=None):
    """srt_render_paths by the yardstick: dict of rgb_linear [rows, cols, 3], rgb8, and seg_* [depth, rows, cols, ...]; padding pixels
    hold `fill` (default 0).  Lights, literals and flags are p's."""
    shade = lambda rays, lights, flags, **lit: sp.shade_paths(oracle, flat, rays, lights, depth, reflectance, bounce_t_min, flags=flags, **lit)
    return compose_frame(oracle, p, shade, fill=fill)


def flat_rows(o):
    """A frame-shaped result as shade_paths lays it out: [rows, cols, ...] -> [n, ...], [depth, rows, cols, ...] -> [depth, n, ...]."""
    out = {}
    for key, v in o.items():
        if key in sp.SEG_KEYS:
            out[key] = v.reshape((v.shape[0], v.shape[1] * v.shape[2]) + v.shape[3:])
        elif key in ("rgb_linear", "rgb8"):
            out[key] = v.reshape((-1,) + v.shape[2:])
    return out


# ---- the frame cases of tests/test_gpu_render_paths.py --------------------------------------------------------------------------------
W, H = 37, 23                      # partial 8 x 8 and 16 x 16 tiles in both directions
DEPTH = 3


def camera_params(name, lights, w=W, h=H, **kw):
    """A frame of shade_path_ref.FRAMES[name]'s camera at w x h: the same field of view (the focal scaled with the width)."""
    import shade_range_ref as sr
    o, target, focal, (w0, _) = sp.FRAMES[name]
    return abi.make_params(w, h, lights, focal=focal * w / w0, ray_matrix=sr.look_at(o, target), **kw)


PLAIN_FOCAL = 22.0                 # ground_bunny without a matrix at W x H: the bunny's foot on the ground fills the frame's centre
FACING_CAMERA = ((-90.0, -60.0, 262.0), (10.0, 0.0, 300.0), 14.0, 16)      # facing_quads' camera in tests/test_gpu_shade_paths.py (origin, target, focal at width)

# name -> (scene, camera mode, (w, h), light samples, flags): depth-3 frames.  tests/test_render_paths_ref.py asserts the input condition
# of each on the yardstick: at least 100 pixels whose segment 1 hits and at least 20 whose segment 2 hits.
CASES = {"ground_bunny, camera": ("ground_bunny", True, (W, H), 2, 0),
         # 8+ light samples, and two chunks of them (64 + 1).  The yardstick renders one oracle frame per hit and sample (65 samples at
         # 37 x 23: minutes), so these two take the smallest frame that still meets the input condition (189 / 100 / 42 hit pixels in
         # segments 0 / 1 / 2) and has partial tiles in both directions and two workgroups.
         "ground_bunny, camera, 16 lights": ("ground_bunny", True, (19, 11), 16, 0),
         "ground_bunny, camera, 65 lights": ("ground_bunny", True, (19, 11), 65, 0),
         "ground_bunny, no matrix": ("ground_bunny", False, (W, H), 1, 0),
         "cubes4_a40, camera": ("cubes4_a40", True, (64, 48), 2, 0),
         "texquad, flat": ("texquad", True, (64, 48), 2, 0),
         "texquad, smooth": ("texquad", True, (64, 48), 2, abi.SRT_FLAG_SMOOTH_NORMALS)}


def facing_quads():
    """texquad with vertex normals, plus a copy of its textured sheet (object 1: nodes 3.., triangles 12..) 70 nearer in z, as object 2:
    two sheets that face one another (the scene tests/test_gpu_shade_paths.py builds for its smooth-normal case, restated here so that
    this helper imports no test module)."""
    import dataclasses
    import golden_util as gu
    import shade_query_ref as sq
    f = sq.texquad_with_normals(gu.GoldenScene("texquad"))
    n0, t0, nn, nt = 3, 12, len(f.node_left), f.n_tris
    dz = np.float32([0.0, 0.0, -70.0])
    link = lambda a: np.where(a[n0:] >= 0, a[n0:] + (nn - n0), a[n0:]).astype(np.int32)
    pts = np.ascontiguousarray(f.tri_points, np.float32).reshape(-1, 3, 4)[t0:].copy()
    pts[..., :3] += dz
    cat = lambda a, b: np.ascontiguousarray(np.concatenate([np.asarray(a), np.asarray(b).astype(np.asarray(a).dtype)]))
    return dataclasses.replace(
        f, node_min=cat(f.node_min, f.node_min[n0:] + dz), node_max=cat(f.node_max, f.node_max[n0:] + dz), node_left=cat(f.node_left, link(f.node_left)),
        node_right=cat(f.node_right, link(f.node_right)), node_first=cat(f.node_first, np.where(f.node_first[n0:] >= 0, f.node_first[n0:] + (nt - t0), f.node_first[n0:])),
        node_count=cat(f.node_count, f.node_count[n0:]), obj_root=cat(f.obj_root, [nn]), tri_points=cat(np.asarray(f.tri_points).reshape(-1, 3, 4), pts),
        tri_obj=cat(f.tri_obj, np.full(nt - t0, 2)), obj_color=cat(np.asarray(f.obj_color).reshape(-1, 3), [[0.3, 0.8, 0.2]]),
        obj_material=cat(np.asarray(f.obj_material).reshape(-1, 3), [[0.2, 0.5, 15.0]]), tri_tex=cat(f.tri_tex, f.tri_tex[t0:]),
        tri_texcoord=cat(f.tri_texcoord, f.tri_texcoord[t0:]), tri_normals=cat(f.tri_normals, f.tri_normals[t0:]))


def case(name):
    """(flat, params, reflectance) of a frame case."""
    import golden_util as gu
    import shade_query_ref as sq
    import shade_range_ref as sr
    scene, camera, (w, h), n_lights, flags = CASES[name]
    if scene == "texquad":
        flat = facing_quads()
        o, target, focal, w0 = FACING_CAMERA
        lights = abi.light_staircase(np.float32([260.0, -420.0, -60.0]), n_lights)
        return flat, abi.make_params(w, h, lights, focal=focal * w / w0, ray_matrix=sr.look_at(o, target), flags=flags), np.float32([0.3, 0.5, 0.7])
    g = gu.GoldenScene(scene)
    lights = sq.lights_for(scene, g.light, n_lights)
    p = camera_params(scene, lights, w, h, flags=flags) if camera else abi.make_params(w, h, lights, focal=PLAIN_FOCAL * w / W, flags=flags)
    return g.flat, p, np.float32(sp.REFLECTANCE[:int(g.flat.tri_obj.max()) + 1])


_cases = CaseCache()


def case_reference(oracle, name):
    """The yardstick's frame of a case: computed once, shared, never changed."""
    def make():
        flat, p, refl = case(name)
        return render_paths(oracle, flat, p, DEPTH, refl, sp.BOUNCE_T_MIN)
    return _cases.once(name, make)


def condition(ref):
    """The input condition of a depth > 1 frame case, on the yardstick."""
    hit = ref["seg_hit_id"] >= 0
    assert hit[1].sum() >= 100, f"segment 1 hits in {int(hit[1].sum())} pixels"
    assert hit[2].sum() >= 20, f"segment 2 hits in {int(hit[2].sum())} pixels"
    assert (~hit[0]).any(), "no pixel misses"
