"""The yardstick of the shaded query with a per-ray t interval (include/srt.h, srt_shade_rays_range): the colour of a hit that need not
be the closest one, reduced to what the oracle offers as it stands.

  * The winner (id, t) of a ray and its interval: ray_range_ref.candidates + ray_range_ref.closest -- the oracle's slab and triangle
    tests, the header's definition of "in range" in numpy.
  * The unshadowed colour of hit h under ONE light L: oracle.render(pow="device") of the ray's 1 x 1 camera-mode frame
    (shade_query_ref.ray_params, lights = [L], the caller's literals and flags) on a SINGLE-TRIANGLE flat scene: one object with the
    colour and material of h's object; one leaf node whose box is the box of the leaf that owns h in the full scene (the ray passed that
    box there: h is a candidate); the one triangle with h's raw points, texcoords, normals and texture id; the scene's own texture
    table.  The oracle's closest hit on that scene is then triangle 0 at the t bits h has in the full scene (the same triangle test on
    the same operands; asserted), nothing can shadow it (the only object is the hit's own, which in_shadow skips), and rgb_linear is
    0 + phong(...) for that light -- texture lookup, flat or interpolated normal, integer shininess all by the oracle itself, at
    o + d * t with the ray's own o and d.
  * The shadow bit of (hit, light): ray_range_ref.occluded on the candidates of the shadow ray so -> L - so with h's object skipped and
    nothing bounding t; so = o + d * t in float32, d * t first, then o +, as in_shadow does (ray_query_ref.shadow_rays).
  * The sum: from 0 in light order, one float32 add per sample; a shadowed sample is divided by shadow_div per component first.
    The sample taken from the 1 x 1 frame is 0 + phong, not phong: the two differ only where a component is -0 (read as +0), and a sum
    that starts at +0 never becomes -0, so adding either zero -- divided or not -- leaves it as it is.
  * Tone map and quantiser: oracle.tonemap(pow="device"); all-black becomes the background.

With no interval, or an identity interval, the winner is the oracle's closest hit and the composition is the oracle's own loop over the
lights written out: tests/test_shade_range_ref.py pins it to shade_query_ref.oracle_shade, the full-scene 1 x 1 frame, bit for bit."""
import numpy as np

from simple_raytracer_amd import abi
import ray_query_ref as rq
import ray_range_ref as rr
import shade_query_ref as sq


def look_at(origin, target, up=(0.05, 0.1, 1.0)):
    """A camera-mode ray matrix (column-major: right, up, forward, origin) looking from `origin` at `target`; no axis-aligned column, so
    that no direction component is -0."""
    o = np.asarray(origin, np.float64)
    f = np.asarray(target, np.float64) - o; f /= np.linalg.norm(f)
    r = np.cross(np.asarray(up, np.float64), f); r /= np.linalg.norm(r)
    u = np.cross(f, r)
    M = np.zeros((4, 4)); M[0, :3] = r; M[1, :3] = u; M[2, :3] = f; M[3, :3] = o; M[3, 3] = 1.0
    return np.ascontiguousarray(M.reshape(-1), np.float32)


# The batch of the device-form case (tests/shade_range_device_case.py runs it in a child process; tests/test_gpu_shade_range.py pins the
# host form on the same batch against the yardstick): one definition for both.
DEVICE_CASE_SCENE, DEVICE_CASE_N, DEVICE_CASE_LIGHTS = "cubes4_a40", 257, 3


def device_case_inputs(flat):
    """(rays, lights) of the device-form case on GoldenScene(DEVICE_CASE_SCENE).flat."""
    rays = rq.unrelated_rays(flat, DEVICE_CASE_N, seed=5)
    return rays, abi.light_staircase(np.asarray(rq.SHADOW_LIGHT[DEVICE_CASE_SCENE], np.float32), DEVICE_CASE_LIGHTS)


def device_case_intervals(plain_hit, plain_t):
    """One interval per ray around the ray's own unbounded hit (a miss: around 50), four kinds dealt round robin: behind the hit, just
    short of it, the closed point, a random-free window (t / 2, 3 t / 2)."""
    inf = np.float32(np.inf)
    n = plain_hit.shape[0]
    t1 = np.where(plain_hit >= 0, plain_t, np.float32(50.0)).astype(np.float32)
    kind = np.arange(n) % 4
    tr = np.empty((n, 2), np.float32)
    tr[:, 0] = np.select([kind == 0, kind == 1, kind == 2], [np.nextafter(t1, inf), 0.0, t1], t1 * np.float32(0.5))
    tr[:, 1] = np.select([kind == 0, kind == 1, kind == 2], [inf, np.nextafter(t1, -inf), t1], t1 * np.float32(1.5))
    return tr


def winners(oracle, flat, rays, t_range=None):
    """(hit_id, t) of every ray inside its interval (None: unbounded): ray_range_ref's closest hit."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    return rr.closest(rr.candidates(oracle, flat, rays), t_range)


def owning_leaf(flat, tri):
    """The leaf node whose triangle range holds each id of `tri`."""
    leaf = np.flatnonzero((flat.node_left < 0) & (flat.node_right < 0))
    first = flat.node_first[leaf].astype(np.int64)
    order = np.argsort(first, kind="stable")
    leaf, first = leaf[order], first[order]
    k = np.searchsorted(first, np.asarray(tri, np.int64), side="right") - 1
    own = leaf[k]
    assert ((flat.node_first[own] <= tri) & (tri < flat.node_first[own] + flat.node_count[own])).all(), "a triangle outside every leaf"
    return own


def single_triangle_scene(flat, h, leaf):
    """The flat scene that holds triangle h alone, under one leaf with the box of `leaf`."""
    obj = int(flat.tri_obj[h])
    one = lambda a, k: None if a is None else np.ascontiguousarray(a.reshape(flat.n_tris, k)[h:h + 1])
    return abi.FlatScene(
        node_min=flat.node_min.reshape(-1, 3)[leaf:leaf + 1], node_max=flat.node_max.reshape(-1, 3)[leaf:leaf + 1],
        node_left=np.int32([-1]), node_right=np.int32([-1]), node_first=np.int32([0]), node_count=np.int32([1]), obj_root=np.uint32([0]),
        tri_points=one(flat.tri_points, 12), tri_obj=np.int32([0]),
        obj_color=flat.obj_color.reshape(-1, 3)[obj:obj + 1], obj_material=flat.obj_material.reshape(-1, 3)[obj:obj + 1],
        tri_tex=flat.tri_tex[h:h + 1], tri_texcoord=one(flat.tri_texcoord, 6), tri_normals=one(flat.tri_normals, 9),
        tex_rgb=flat.tex_rgb, tex_off=flat.tex_off, tex_w=flat.tex_w, tex_h=flat.tex_h)


def samples(oracle, flat, rays, hit, t, lights, flags=0, **literals):
    """For the rays that hit (in ray order): colour (n_hit x n_lights x 3 float32, each sample unshadowed) and shadowed (n_hit x
    n_lights bool)."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    lights = np.ascontiguousarray(lights, np.float32).reshape(-1, 3)
    sel = np.flatnonzero(hit >= 0)
    nh, nl = sel.size, lights.shape[0]
    colour = np.zeros((nh, nl, 3), np.float32)
    shadowed = np.zeros((nh, nl), bool)
    if nh == 0 or nl == 0:
        return colour, shadowed
    leaf = owning_leaf(flat, hit[sel])
    for k, i in enumerate(sel):
        one = single_triangle_scene(flat, int(hit[i]), int(leaf[k]))
        for l in range(nl):
            c = oracle.render(one, sq.ray_params(rays[i], lights[l:l + 1], flags=flags, **literals), n_threads=1, pow="device")
            assert c["hit_id"][0, 0] == 0 and sq.bits(c["t"])[0, 0] == sq.bits(t[i:i + 1])[0], "the single-triangle frame hits elsewhere"
            colour[k, l] = c["rgb_linear"][0, 0]
    skip = flat.tri_obj[hit[sel]].astype(np.int64)
    srays = np.concatenate([rq.shadow_rays(rays[sel], t[sel], lights[l]) for l in range(nl)])      # light-major
    c = rr.candidates(oracle, flat, srays)
    shadowed[:] = rr.occluded(c, flat, None, np.tile(skip, nl)).reshape(nl, nh).T.astype(bool)
    return colour, shadowed


def compose(oracle, hit, colour, shadowed, shadow_div=5.0, reinhard=0.5, gamma=1.1, background=abi.REFERENCE_BACKGROUND):
    """(rgb_linear n x 3, rgb8 n x 3): the sum over the samples in light order, tone map, quantiser, background rule."""
    n = hit.shape[0]
    lin = np.zeros((n, 3), np.float32)
    acc = np.zeros((colour.shape[0], 3), np.float32)
    div = np.float32(shadow_div)
    with np.errstate(all="ignore"):
        for l in range(colour.shape[1]):
            c = colour[:, l]
            c = np.where(shadowed[:, l, None], c / div, c).astype(np.float32)
            acc = (acc + c).astype(np.float32)
    lin[hit >= 0] = acc
    _, q = oracle.tonemap(lin, reinhard, gamma, pow="device")
    q = q.copy()
    q[np.all(q == 0, axis=1)] = np.asarray(background[:3], np.int32)
    return lin, q.astype(np.uint8)


def shade(oracle, flat, rays, lights, t_range=None, flags=0, **literals):
    """(hit_id n, t n, rgb_linear n x 3, rgb8 n x 3) of srt_shade_rays_range by the composition above."""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    hit, t = winners(oracle, flat, rays, t_range)
    colour, shadowed = samples(oracle, flat, rays, hit, t, lights, flags, **literals)
    lin, rgb8 = compose(oracle, hit, colour, shadowed, **literals)
    return hit, t, lin, rgb8
