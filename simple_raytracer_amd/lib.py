"""ctypes binding of the C ABI in include/srt.h and its extension headers include/srt_points.h, include/srt_nearest.h,
include/srt_signed.h, include/srt_points_multi.h and include/srt_segments.h (libsrt_hip.so).

The product path has NO CPU fallback: if the HIP library is missing or no GPU is visible, this
raises.  (The CPU restatement under oracle/ is test infrastructure and is never imported here.)
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsrt_hip.so")

ABI_SYMBOLS = tuple(abi.PROTOTYPES)           # every symbol include/srt.h declares
POINT_SYMBOLS = tuple(abi.POINT_PROTOTYPES)    # every symbol include/srt_points.h declares
NEAREST_SYMBOLS = tuple(abi.NEAREST_PROTOTYPES)    # every symbol include/srt_nearest.h declares
SIGNED_SYMBOLS = tuple(abi.SIGNED_PROTOTYPES)    # every symbol include/srt_signed.h declares
POINT_MULTI_SYMBOLS = tuple(abi.POINT_MULTI_PROTOTYPES)    # every symbol include/srt_points_multi.h declares
SEGMENT_SYMBOLS = tuple(abi.SEGMENT_PROTOTYPES)    # every symbol include/srt_segments.h declares
MULTI_HIT_MAX = abi.SRT_MULTI_HIT_MAX
POINT_MULTI_MAX = abi.POINT_MULTI_MAX

_f32p, _i32p, _u8p, _u32p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
_lib = None


class SrtError(RuntimeError):
    def __init__(self, code, where):
        L = load()
        msg = L.srt_strerror(code).decode()
        super().__init__(f"{where}: {msg} (code {code}, hip error {L.srt_last_hip_error()})")
        self.code = code


def load(path=None):
    """Load libsrt_hip.so; fail loudly if it has not been built (python -m simple_raytracer_amd.build).
    path: another build of the same library (a measurement variant, see build.py) -- loaded and bound, not kept as the product's."""
    global _lib
    if _lib is None or path is not None:
        if not os.path.exists(path or LIB_PATH):
            raise RuntimeError(f"{path or LIB_PATH} is missing: the HIP extension must be built "
                               "(python -m simple_raytracer_amd.build); there is no CPU fallback")
        L = C.CDLL(path or LIB_PATH)
        for name, (restype, argtypes) in {**abi.PROTOTYPES, **abi.POINT_PROTOTYPES, **abi.NEAREST_PROTOTYPES, **abi.SIGNED_PROTOTYPES,
                                            **abi.POINT_MULTI_PROTOTYPES, **abi.SEGMENT_PROTOTYPES}.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        if path is not None:
            return L
        _lib = L
    return _lib


def _check(rc, where):
    if rc != abi.SRT_OK:
        raise SrtError(rc, where)


class DeviceScene:
    """A flat scene resident on one HIP device (opaque srt_scene handle)."""

    def __init__(self, flat: abi.FlatScene, device: int = 0, library=None):
        self.L = library if library is not None else load()
        self.flat = flat
        self.device = device
        h = C.c_void_p()
        d = flat.desc()
        _check(self.L.srt_scene_create(device, C.byref(d), C.byref(h)), "srt_scene_create")
        self.h = h

    def share(self):
        """srt_scene_share: another handle (own workspace and counters) on this scene's device records."""
        o = object.__new__(DeviceScene)
        o.L, o.flat, o.device = self.L, self.flat, self.device
        h = C.c_void_p()
        _check(self.L.srt_scene_share(self.h, C.byref(h)), "srt_scene_share")
        o.h = h
        return o

    def update(self, flat: abi.FlatScene, stream=0):
        """srt_scene_update: new geometry with the same counts into the existing device allocations (asynchronous on `stream`)."""
        d = flat.desc()
        _check(self.L.srt_scene_update(self.h, C.byref(d), stream), "srt_scene_update")
        self.flat = flat

    def set_source(self, tri_texcoord=None, tri_normals=None, tri_tex=None):
        """srt_scene_set_source: per-triangle attributes in SOURCE order (objects concatenated), for update_frame."""
        _check(self.L.srt_scene_set_source(self.h, _host(_array(tri_texcoord, np.float32), _f32p), _host(_array(tri_normals, np.float32), _f32p),
                                           _host(_array(tri_tex, np.int32), _i32p)), "srt_scene_set_source")

    def update_frame(self, points, order, node_min, node_max, obj_color=None, obj_material=None, stream=0):
        """srt_scene_update_frame: per object the transformed points in source order (n x 3 x 4), the build's permutation (n), the node
        boxes in DFS pre-order (m x 3 each); the records are derived on the device."""
        n = len(points)
        pts = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in points]
        ords = [np.ascontiguousarray(x, np.uint32) for x in order]
        mn = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in node_min]
        mx = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in node_max]
        g = abi.FrameGeometry()
        g.n_objects = n
        nt = (C.c_uint32 * n)(*[o.shape[0] for o in ords]); nn = (C.c_uint32 * n)(*[m.shape[0] // 3 for m in mn])
        pp = (_f32p * n)(*[p.ctypes.data_as(_f32p) for p in pts]); po = (C.POINTER(C.c_uint32) * n)(*[o.ctypes.data_as(C.POINTER(C.c_uint32)) for o in ords])
        pmn = (_f32p * n)(*[m.ctypes.data_as(_f32p) for m in mn]); pmx = (_f32p * n)(*[m.ctypes.data_as(_f32p) for m in mx])
        g.obj_n_tris, g.obj_n_nodes, g.obj_points, g.obj_order, g.obj_node_min, g.obj_node_max = nt, nn, pp, po, pmn, pmx
        col, mat = _array(obj_color, np.float32), _array(obj_material, np.float32)
        g.obj_color, g.obj_material = _host(col, _f32p), _host(mat, _f32p)
        _check(self.L.srt_scene_update_frame(self.h, C.byref(g), stream), "srt_scene_update_frame")

    def set_pose_source(self, tri_points=None):
        """srt_scene_set_pose_source: the points (n_tris x 3 x 4, the scene's visit order) the poses are applied to; default: the flat scene's."""
        pts = np.ascontiguousarray(self.flat.tri_points if tri_points is None else tri_points, np.float32)
        assert pts.size == 12 * self.flat.n_tris, "tri_points: n_tris x 3 x 4"
        _check(self.L.srt_scene_set_pose_source(self.h, pts.ctypes.data_as(_f32p)), "srt_scene_set_pose_source")

    def pose(self, matrices, obj_color=None, obj_material=None, stream=0):
        """srt_scene_pose: one column-major 4x4 matrix per object (n_objects x 16); points, triangle records and boxes follow on the device."""
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        _check(self.L.srt_scene_pose(self.h, m.shape[0], _host(m, _f32p), _host(_array(obj_color, np.float32), _f32p), _host(_array(obj_material, np.float32), _f32p),
                                     stream), "srt_scene_pose")

    def set_object_masks(self, masks, stream=0):
        """srt_scene_set_object_masks: one uint32 per object (host array), or None = all ones.  Object k takes part in a masked walk with
        mask m iff (masks[k] & m) != 0; every handle that shares this scene's records sees the table; asynchronous on `stream`."""
        m = None if masks is None else np.ascontiguousarray(masks, np.uint32).reshape(-1)
        n = self.flat.n_objects if m is None else m.shape[0]
        _check(self.L.srt_scene_set_object_masks(self.h, n, _host(m, _u32p), stream), "srt_scene_set_object_masks")

    def refit_prepare(self, tri_vertex=None, n_verts=0):
        """srt_scene_refit_prepare: the refit's schedule, once per tree; tri_vertex (n_tris x 3 vertex numbers, the scene's visit order,
        host array) and n_verts prepare the indexed form as well."""
        tv = _array(tri_vertex, np.uint32)
        assert tv is None or tv.size == 3 * self.flat.n_tris, "tri_vertex: n_tris x 3"
        _check(self.L.srt_scene_refit_prepare(self.h, n_verts, _host(tv, _u32p)), "srt_scene_refit_prepare")

    def refit_device(self, points, stride=4, n_verts=0, normals=0, stream=0):
        """srt_scene_refit_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, async on `stream`.  n_verts 0: points =
        n_tris x 3 points of `stride` floats in visit order (normals n_tris x 9); else n_verts points gathered through the prepared
        indices (normals n_verts x 3).  self.flat is NOT updated: it keeps the scene the handle was created or last updated from."""
        g = abi.RefitDesc(n_verts, stride, points, normals)
        _check(self.L.srt_scene_refit_device(self.h, C.byref(g), stream), "srt_scene_refit_device")

    def records(self):
        """srt_debug_scene_records: the device records as raw numpy arrays (dict)."""
        nN, nT, nO = self.flat.n_nodes, self.flat.n_tris, self.flat.n_objects
        out = {"nodes": np.zeros((nN, 8), np.uint32), "tris": np.zeros((nT, 12), np.uint32), "tris_o": np.zeros((nT, 12), np.uint32),
               "wide": np.zeros(((nN - nO) // 2, 16), np.uint32), "root_nodes": np.zeros((nO, 8), np.uint32),
               "tri_texcoord": np.zeros((nT, 6), np.float32), "tri_normals": np.zeros((nT, 9), np.float32), "tri_tex": np.full(nT, -7, np.int32)}
        v = lambda k: out[k].ctypes.data
        _check(self.L.srt_debug_scene_records(self.h, v("nodes"), v("tris"), v("tris_o"), v("wide"), v("root_nodes"), _host(out["tri_texcoord"], _f32p),
                                              _host(out["tri_normals"], _f32p), _host(out["tri_tex"], _i32p)), "srt_debug_scene_records")
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.srt_scene_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_bytes(self):
        return int(self.L.srt_scene_device_bytes(self.h))

    @property
    def pipeline(self):
        """Kernels of the last render, in launch order."""
        return self.L.srt_scene_pipeline(self.h).decode()

    @property
    def overlap_estimate(self):
        return float(self.L.srt_scene_overlap_estimate(self.h))

    def rows(self, params):
        return int(self.L.srt_rows_owned(C.byref(params)))

    def cols(self, params):
        """Width of the rows a call with these params writes (params.width unless the frame is dealt in tiles)."""
        return int(self.L.srt_cols_owned(C.byref(params)))

    def render(self, params: abi.Params, want=("hit_id", "t", "rgb_linear", "rgb8")):
        """srt_render: host buffers out.  Returns dict of numpy arrays + 'stats'."""
        out, g = _outputs(want, (self.rows(params), self.cols(params)), _FRAME)
        return _with_stats(out, self.L.srt_render, "srt_render", self.h, C.byref(params), g("hit_id"), g("t"), g("rgb_linear"), g("rgb8"))

    def render_device(self, params: abi.Params, stream=0, hit_id=0, t=0, rgb_linear=0, rgb8=0):
        """srt_render_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, async on `stream`."""
        _check(self.L.srt_render_device(self.h, C.byref(params), stream, hit_id, t, rgb_linear, rgb8), "srt_render_device")

    def trace_rays(self, rays, want=("hit_id", "t", "bary"), count=False, t_range=None, ray_mask=None):
        """srt_trace_rays: the closest hit of every ray of `rays` (n x 6: origin xyz, direction xyz; host array).  Returns a dict of
        the arrays named in `want` (hit_id n, t n, bary n x 3) + 'stats'; count=True fills the node / triangle test counts.
        t_range (n x 2: t_min, t_max per ray): srt_trace_rays_range, the closest hit inside each ray's closed interval.
        ray_mask (n uint32, or True = all ones): srt_trace_rays_masked, the closest hit among the objects whose mask (set_object_masks)
        shares a bit with the ray's."""
        r, n = _rays(rays)
        out, g = _outputs(want, (n,), _CLOSEST)
        fn, name, mid = _ray_call(self.L, "srt_trace_rays", "", _t_range(t_range, n), _host_mask(ray_mask, n))
        return _with_stats(out, fn, name, self.h, n, r, *mid, _query_flags(count=count), g("hit_id"), g("t"), g("bary"))

    def occluded(self, rays, skip_obj=None, t_range=None, ray_mask=None):
        """srt_occluded: one uint8 per ray of `rays` (n x 6, host array), 1 = something other than object skip_obj[i] is hit at any t.
        t_range (n x 2: t_min, t_max per ray): srt_occluded_range, ... is hit at a t inside the ray's closed interval.
        ray_mask (n uint32, or True = all ones): srt_occluded_masked, ... among the objects whose mask shares a bit with the ray's."""
        r, n = _rays(rays)
        sk = None if skip_obj is None else np.ascontiguousarray(skip_obj, np.int32).reshape(-1)
        assert sk is None or sk.shape[0] == n, "skip_obj: one entry per ray"
        occ = np.empty(n, np.uint8)
        fn, name, mid = _ray_call(self.L, "srt_occluded", "", _t_range(t_range, n), _host_mask(ray_mask, n))
        _check(fn(self.h, n, r, *mid, _host(sk, _i32p), _host(occ, _u8p)), name)
        return occ

    def trace_rays_device(self, n, rays, stream=0, hit_id=0, t=0, bary=0, count=False, t_range=None, ray_mask=None):
        """srt_trace_rays_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`.
        t_range (a device pointer to n x 2 floats): srt_trace_rays_range_device.
        ray_mask (a device pointer to n uint32, or 0 = all ones): srt_trace_rays_masked_device."""
        fn, name, mid = _ray_call(self.L, "srt_trace_rays", "_device", t_range, _device_mask(ray_mask))
        _check(fn(self.h, n, rays, *mid, _query_flags(count=count), stream, hit_id, t, bary), name)

    def occluded_device(self, n, rays, occluded, skip_obj=0, stream=0, t_range=None, ray_mask=None):
        """srt_occluded_device: raw device pointers in, asynchronous on `stream`.  t_range (a device pointer to n x 2 floats):
        srt_occluded_range_device.  ray_mask (a device pointer to n uint32, or 0 = all ones): srt_occluded_masked_device."""
        fn, name, mid = _ray_call(self.L, "srt_occluded", "_device", t_range, _device_mask(ray_mask))
        _check(fn(self.h, n, rays, *mid, skip_obj, stream, occluded), name)

    def trace_rays_multi(self, rays, k, want=("n_hits", "hit_id", "t", "bary"), count=False, t_range=None):
        """srt_trace_rays_multi: the k nearest hits of every ray of `rays` (n x 6, host array) in one walk, nearest first, equal t by id.
        Returns a dict of the arrays named in `want` (n_hits n uint32 -- the full count, it may exceed k --, hit_id n x k, t n x k,
        bary n x k x 3; unused slots -1, +inf, 0) + 'stats'.  t_range (n x 2: t_min, t_max per ray): only hits inside the closed interval."""
        r, n = _rays(rays)
        k = int(k)
        out, g = _outputs(want, (n,), {"n_hits": (np.uint32, ())})
        rows, g_rows = _outputs(want, (n, max(k, 0)), _CLOSEST)
        out.update(rows)
        return _with_stats(out, self.L.srt_trace_rays_multi, "srt_trace_rays_multi", self.h, n, r, _t_range(t_range, n), k, _query_flags(count=count), g("n_hits"),
                           g_rows("hit_id"), g_rows("t"), g_rows("bary"))

    def trace_rays_multi_device(self, n, rays, k, stream=0, n_hits=0, hit_id=0, t=0, bary=0, count=False, t_range=None):
        """srt_trace_rays_multi_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`; t_range a
        device pointer to n x 2 floats, or None."""
        _check(self.L.srt_trace_rays_multi_device(self.h, n, rays, t_range or 0, k, _query_flags(count=count), stream, n_hits, hit_id, t, bary),
               "srt_trace_rays_multi_device")

    def shade_rays(self, rays, params: abi.Params, want=("hit_id", "t", "rgb_linear", "rgb8"), count=False, t_range=None):
        """srt_shade_rays: the colour that comes back along every ray of `rays` (n x 6, host array) under the lights, literals and flags
        of `params` (its frame geometry is ignored).  Returns a dict of the arrays named in `want` (hit_id n, t n, rgb_linear n x 3,
        rgb8 n x 3) + 'stats'; count=True adds SRT_FLAG_COUNT_WORK for this call.
        t_range (n x 2: t_min, t_max per ray): srt_shade_rays_range, the colour of the closest hit inside each ray's closed interval."""
        r, n = _rays(rays)
        out, g = _outputs(want, (n,), _FRAME)
        fn, name, mid = _ray_call(self.L, "srt_shade_rays", "", _t_range(t_range, n), None)
        with _flags(params, count=count):
            return _with_stats(out, fn, name, self.h, n, r, *mid, C.byref(params), g("hit_id"), g("t"), g("rgb_linear"), g("rgb8"))

    def shade_rays_device(self, n, rays, params: abi.Params, stream=0, hit_id=0, t=0, rgb_linear=0, rgb8=0, t_range=None):
        """srt_shade_rays_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`; the light table
        of `params` is a host array.  t_range (a device pointer to n x 2 floats): srt_shade_rays_range_device."""
        fn, name, mid = _ray_call(self.L, "srt_shade_rays", "_device", t_range, None)
        _check(fn(self.h, n, rays, *mid, C.byref(params), stream, hit_id, t, rgb_linear, rgb8), name)

    def surface_rays(self, rays, want=("hit_id", "t", "obj", "point", "normal", "color", "material", "bounce"), smooth=False, count=False, t_range=None):
        """srt_surface_rays: the closest hit of every ray of `rays` (n x 6, host array) and the surface under it.  Returns a dict of the
        arrays named in `want` (hit_id n, t n, obj n, point / normal / color / material n x 3, bounce n x 6: the mirrored ray) + 'stats'.
        smooth: SRT_FLAG_SMOOTH_NORMALS; count: SRT_FLAG_COUNT_WORK; t_range (n x 2: t_min, t_max per ray): the closest hit inside each
        ray's closed interval."""
        r, n = _rays(rays)
        out, g = _outputs(want, (n,), {**_HIT, **_SURFACE})
        so = abi.SurfaceOut(*_addresses(out, _SURFACE))
        return _with_stats(out, self.L.srt_surface_rays, "srt_surface_rays", self.h, n, r, _t_range(t_range, n), _query_flags(smooth, count), g("hit_id"), g("t"),
                           C.byref(so))

    def surface_rays_device(self, n, rays, stream=0, hit_id=0, t=0, obj=0, point=0, normal=0, color=0, material=0, bounce=0, smooth=False, count=False, t_range=None):
        """srt_surface_rays_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`; t_range a device
        pointer to n x 2 floats, or None."""
        so = _wanted(abi.SurfaceOut, obj, point, normal, color, material, bounce)
        _check(self.L.srt_surface_rays_device(self.h, n, rays, t_range or 0, _query_flags(smooth, count), stream, hit_id, t, C.byref(so)), "srt_surface_rays_device")

    def surface_hits(self, rays, hit_id, t, want=("obj", "point", "normal", "color", "material", "bounce"), smooth=False):
        """srt_surface_hits: the surface under hits the caller already holds -- `hit_id` (n) and `t` (n) of the rays `rays` (n x 6, host
        arrays): a render's, srt_trace_rays', a column of srt_trace_rays_multi.  No walk.  Returns a dict of the arrays named in `want`."""
        r, n = _rays(rays)
        out, _ = _outputs(want, (n,), _SURFACE)
        so = abi.SurfaceOut(*_addresses(out, _SURFACE))
        _check(self.L.srt_surface_hits(self.h, n, r, *_hits(hit_id, t, n), _query_flags(smooth), C.byref(so)), "srt_surface_hits")
        return out

    def surface_hits_device(self, n, rays, hit_id, t, stream=0, obj=0, point=0, normal=0, color=0, material=0, bounce=0, smooth=False):
        """srt_surface_hits_device: raw device pointers (ints) in -- the rays, their hit ids and t --, asynchronous on `stream`."""
        so = _wanted(abi.SurfaceOut, obj, point, normal, color, material, bounce)
        _check(self.L.srt_surface_hits_device(self.h, n, rays, hit_id, t, _query_flags(smooth), stream, C.byref(so)), "srt_surface_hits_device")

    def ao_rays(self, rays, dirs, t_min=1e-3, t_max=np.inf, t_range=None, skip_self=False, visibility=None, smooth=False, count=False,
                want=("hit_id", "t", "n_occluded", "ao", "occ_bits")):
        """srt_ao_rays: the closest hit of every ray of `rays` (n x 6, host array) and how open the surface is there -- `dirs` (K x 3, in the
        hit's local frame, z along the normal that faces the ray: ao_directions) are turned into the hit's frame and walked as occlusion
        rays from the hit point; a direction is blocked iff something lies inside the closed (t_min, t_max), in units of the direction.
        Returns a dict of the arrays named in `want` (hit_id n, t n, n_occluded n uint32, ao n = (K - n_occluded) / K, occ_bits n x W uint32
        with W = (K + 31) // 32, bit k & 31 of word k >> 5 for direction k) + 'stats'.  t_range (n x 2): the interval of the closest hit.
        skip_self: SRT_AO_SKIP_SELF, the hit's own object blocks nothing.  visibility: None, or (primary, bounce, shadow) -- the closest
        hit is walked with primary, the AO rays with shadow.  smooth: SRT_FLAG_SMOOTH_NORMALS; count: SRT_FLAG_COUNT_WORK."""
        r, n = _rays(rays)
        desc, table = _ao_desc(dirs, t_min, t_max, skip_self)
        out, g = _outputs(want, (n,), _HIT)
        aout, arrays = _ao_out(want, n, desc.n_dirs)
        out.update(arrays)
        return _with_stats(out, self.L.srt_ao_rays, "srt_ao_rays", self.h, n, r, _t_range(t_range, n), _query_flags(smooth, count), C.byref(desc), _vis_ref(visibility),
                           g("hit_id"), g("t"), C.byref(aout))

    def ao_hits(self, rays, hit_id, t, dirs, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None, smooth=False, count=False,
                want=("n_occluded", "ao", "occ_bits")):
        """srt_ao_hits: ao_rays for hits the caller already holds -- `hit_id` (n) and `t` (n) of the rays `rays` (n x 6, host arrays): a
        render's with the frame's rays, trace_rays', a column of trace_rays_multi.  No closest-hit walk; an id outside [0, n_tris) is a
        miss row (n_occluded 0, ao 1).  Returns a dict of the arrays named in `want` + 'stats'."""
        r, n = _rays(rays)
        hits = _hits(hit_id, t, n)
        desc, table = _ao_desc(dirs, t_min, t_max, skip_self)
        aout, out = _ao_out(want, n, desc.n_dirs)
        return _with_stats(out, self.L.srt_ao_hits, "srt_ao_hits", self.h, n, r, *hits, _query_flags(smooth, count), C.byref(desc), _vis_ref(visibility), C.byref(aout))

    def _ao_device(self, name, head, dirs, n_dirs, t_min, t_max, skip_self, rot, visibility, smooth, count, stream, hit, outs):
        """The _device form of an ambient-occlusion call.  head: the arguments between the handle and the flags; rot: None, or the
        (rot_w, rot_h, address) of a frame call's srt_ao_frame; hit: the hit_id and t outputs, where the call has them; outs: the
        addresses of its srt_ao_out, or of a frame call's srt_ao_frame_out."""
        desc = abi.AoDesc(n_dirs, dirs or None, t_min, t_max, abi.SRT_AO_SKIP_SELF if skip_self else 0)
        frame = () if rot is None else (C.byref(abi.AoFrame(rot[0], rot[1], rot[2] or None)),)
        out = _wanted(abi.AoOut if rot is None else abi.AoFrameOut, *outs)
        _check(getattr(self.L, name)(self.h, *head, _query_flags(smooth, count), C.byref(desc), *frame, _vis_ref(visibility), stream, *hit, C.byref(out)), name)

    def ao_rays_device(self, n, rays, dirs, n_dirs, t_min=1e-3, t_max=np.inf, t_range=None, skip_self=False, visibility=None, smooth=False, count=False, stream=0,
                       hit_id=0, t=0, n_occluded=0, ao=0, occ_bits=0):
        """srt_ao_rays_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in -- the rays, the table `dirs` of n_dirs x 3 floats,
        t_range (n x 2 floats, or None) and the outputs (0: not wanted) --, asynchronous on `stream`."""
        self._ao_device("srt_ao_rays_device", (n, rays, t_range or 0), dirs, n_dirs, t_min, t_max, skip_self, None, visibility, smooth, count, stream, (hit_id, t),
                        (n_occluded, ao, occ_bits))

    def ao_hits_device(self, n, rays, hit_id, t, dirs, n_dirs, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None, smooth=False, count=False, stream=0,
                       n_occluded=0, ao=0, occ_bits=0):
        """srt_ao_hits_device: raw device pointers (ints) in -- the rays, their hit ids and t, the table --, asynchronous on `stream`."""
        self._ao_device("srt_ao_hits_device", (n, rays, hit_id, t), dirs, n_dirs, t_min, t_max, skip_self, None, visibility, smooth, count, stream, (),
                        (n_occluded, ao, occ_bits))

    def render_ao(self, params: abi.Params, dirs, rot=None, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None, smooth=False, count=False,
                  want=("hit_id", "t", "n_occluded", "ao", "occ_bits", "bent", "ao8"), fill=None):
        """srt_render_ao: ao_rays for the rays of the frame's own pixels -- the local pixels of a call with `params` (its block or tile deal,
        camera matrix and spp included); no ray array is built.  rot: None, or an h x w x 2 table of (cos, sin) (ao_rotations) -- the pixel
        at image (x, y) turns `dirs` about z by entry (y % h, x % w) before its frame is applied.  Returns a dict of the arrays named in
        `want` -- hit_id, t, n_occluded, ao, ao8 [rows, cols], occ_bits [rows, cols, W], bent [rows, cols, 3]: the sum of the directions that
        are not blocked, as walked -- + 'stats'.  With spp > 1 ao is the mean over the sub-samples, the other arrays are sub-sample 0's.
        fill: a value every array holds before the call (padding pixels of a tile deal keep it).  The rest as in ao_rays."""
        lead = (self.rows(params), self.cols(params))
        desc, table = _ao_desc(dirs, t_min, t_max, skip_self)
        frame, turns = _ao_frame(rot)
        out, g = _outputs(want, lead, _HIT, fill)
        fout, arrays = _ao_frame_out(want, lead, desc.n_dirs, fill)
        out.update(arrays)
        return _with_stats(out, self.L.srt_render_ao, "srt_render_ao", self.h, C.byref(params), _query_flags(smooth, count), C.byref(desc), C.byref(frame),
                           _vis_ref(visibility), g("hit_id"), g("t"), C.byref(fout))

    def render_ao_hits(self, params: abi.Params, hit_id, t, dirs, rot=None, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None, smooth=False, count=False,
                       want=("n_occluded", "ao", "occ_bits", "bent", "ao8"), fill=None):
        """srt_render_ao_hits: render_ao for hits the caller already holds -- `hit_id` and `t` [rows, cols] as render(params) returns them
        (host arrays).  No closest-hit walk; only sub-sample 0's ray is used; an id outside [0, n_tris) is a miss row (n_occluded 0, ao 1,
        bent 0, ao8 255).  Returns a dict of the arrays named in `want` + 'stats'."""
        lead = (self.rows(params), self.cols(params))
        hits = _hits(hit_id, t, lead[0] * lead[1], "hit_id, t: one entry per local pixel")
        desc, table = _ao_desc(dirs, t_min, t_max, skip_self)
        frame, turns = _ao_frame(rot)
        fout, out = _ao_frame_out(want, lead, desc.n_dirs, fill)
        return _with_stats(out, self.L.srt_render_ao_hits, "srt_render_ao_hits", self.h, C.byref(params), *hits, _query_flags(smooth, count), C.byref(desc),
                           C.byref(frame), _vis_ref(visibility), C.byref(fout))

    def render_ao_device(self, params: abi.Params, dirs, n_dirs, rot=0, rot_w=0, rot_h=0, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None, smooth=False,
                         count=False, stream=0, hit_id=0, t=0, n_occluded=0, ao=0, occ_bits=0, bent=0, ao8=0):
        """srt_render_ao_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in -- the table `dirs` of n_dirs x 3 floats, the
        rotation table `rot` of rot_h x rot_w x 2 floats (0: none) and the outputs of the call's local pixels (0: not wanted) --,
        asynchronous on `stream`, one launch."""
        self._ao_device("srt_render_ao_device", (C.byref(params),), dirs, n_dirs, t_min, t_max, skip_self, (rot_w, rot_h, rot), visibility, smooth, count, stream,
                        (hit_id, t), (n_occluded, ao, occ_bits, bent, ao8))

    def render_ao_hits_device(self, params: abi.Params, hit_id, t, dirs, n_dirs, rot=0, rot_w=0, rot_h=0, t_min=1e-3, t_max=np.inf, skip_self=False, visibility=None,
                              smooth=False, count=False, stream=0, n_occluded=0, ao=0, occ_bits=0, bent=0, ao8=0):
        """srt_render_ao_hits_device: raw device pointers (ints) in -- a render's hit_id / t of the same `params`, the tables --, asynchronous
        on `stream`, one launch."""
        self._ao_device("srt_render_ao_hits_device", (C.byref(params), hit_id, t), dirs, n_dirs, t_min, t_max, skip_self, (rot_w, rot_h, rot), visibility, smooth, count,
                        stream, (), (n_occluded, ao, occ_bits, bent, ao8))

    def _paths_host(self, kind, head, lead, params, depth, reflectance, bounce_t_min, want, count, smooth, fill, shadow, visibility, ior, fresnel=None):
        """The host form of a path call: srt_<kind>_paths and its _shadow, _masked, _refract and _fresnel forms.  head: the arguments
        before the params; lead: the shape of one segment's rows."""
        refl = None if reflectance is None else np.ascontiguousarray(reflectance, np.float32).reshape(-1)
        out, g = _outputs(want, lead, _PATH_SUMS, fill)
        seg, _ = _outputs(want, (max(int(depth), 0),) + lead, _PATH_SEGMENTS, fill)
        out.update(seg)
        po = abi.PathOut(*_addresses(seg, _PATH_SEGMENTS))
        pd = abi.PathDesc(depth, bounce_t_min, refl.ctypes.data if refl is not None else None)
        refr, table = _refraction(ior, self.flat.n_objects)
        fres, f0 = None, None
        if fresnel is not None:
            f0 = np.ascontiguousarray(fresnel, np.float32).reshape(-1)
            assert f0.shape[0] == self.flat.n_objects, "fresnel: one float per object"
            side, _ = _outputs(want, (max(int(depth), 0),) + lead, _PATH_SIDE, fill)
            out.update(side)
            fout = abi.FresnelOut(*_addresses(side, _PATH_SIDE))
            fres = abi.Fresnel(f0.ctypes.data, 0, C.pointer(fout))
        fn, name, mid = _path_call(self.L, kind, "", abi.shadow_rule(shadow), abi.visibility(visibility), refr, fres)
        with _flags(params, count=count, smooth=smooth):
            return _with_stats(out, fn, name, *head, C.byref(params), C.byref(pd), *mid, g("rgb_linear"), g("rgb8"), C.byref(po))

    def _paths_device(self, kind, head, params, depth, reflectance, bounce_t_min, stream, rgb_linear, rgb8, segments, shadow, visibility, ior, fresnel=None, side=()):
        """The device form of a path call.  ior: None, or a device pointer (0: the _refract call without a table).  fresnel: None, or a
        device pointer to f0 (0: the _fresnel call without a table); side: the four device pointers of its srt_fresnel_out."""
        pd = abi.PathDesc(depth, bounce_t_min, reflectance or None)
        po = _wanted(abi.PathOut, *segments)
        refr = None if ior is None else abi.Refraction(ior or None, 0)
        fres = None
        if fresnel is not None:
            fout = _wanted(abi.FresnelOut, *side)
            fres = abi.Fresnel(fresnel or None, 0, C.pointer(fout))
        fn, name, mid = _path_call(self.L, kind, "_device", abi.shadow_rule(shadow), abi.visibility(visibility), refr, fres)
        _check(fn(*head, C.byref(params), C.byref(pd), *mid, stream, rgb_linear, rgb8, C.byref(po)), name)

    def shade_paths(self, rays, params: abi.Params, depth, reflectance=None, bounce_t_min=1e-3, t_range=None,
                    want=("rgb_linear", "rgb8", "seg_hit_id", "seg_t", "seg_obj", "seg_rgb_linear", "seg_rays"), count=False, smooth=False, shadow=None,
                    visibility=None, ior=None, fresnel=None):
        """srt_shade_paths: every ray of `rays` (n x 6, host array) followed through up to `depth` mirror bounces, each hit shaded as
        shade_rays(t_range=...) shades it, the segments mixed by `reflectance` (one float per object, or None = all 0).  A mirrored ray's
        interval is (bounce_t_min, +inf); t_range (n x 2) bounds segment 0.  Returns a dict of the arrays named in `want` -- rgb_linear
        n x 3 (mixed), rgb8 n x 3, and per segment seg_hit_id / seg_t / seg_obj depth x n, seg_rgb_linear depth x n x 3, seg_rays
        depth x n x 6 -- + 'stats'.  count / smooth add SRT_FLAG_COUNT_WORK / SRT_FLAG_SMOOTH_NORMALS for this call.
        shadow: None = the reference's shadow rule (unbounded, the hit object left out), or (t_min, t_max, self_shadow): a shadow
        ray blocks only inside the closed (t_min, t_max) in units of light - hit point, and with self_shadow the hit object's own tree
        is walked too (srt_*_paths_shadow).
        visibility: None, or (primary, bounce, shadow) -- the object masks segment 0, every later segment and every shadow ray are
        walked with (srt_*_paths_masked; set_object_masks gives the objects their bits).
        ior: None, or one float per object (host array) -- object k with ior[k] > 0 is glass: a ray that hits it goes on THROUGH the
        surface, bent by Snell's law, instead of being mirrored (srt_*_paths_refract); reflectance keeps weighting what follows.
        fresnel: None, or one float per object (host array), f0, the reflectance at normal incidence (schlick_f0(ior) for a dielectric)
        -- at a hit on an object k with ior[k] > 0 and f0[k] >= 0 the mirrored ray is walked and shaded once as a side ray, and its sum
        enters the mix with Schlick's weight (srt_*_paths_fresnel).  `want` may then name side_hit_id / side_t / fresnel (depth x n) and
        side_rgb_linear (depth x n x 3): per segment, the side ray's hit, its sum and the weight F."""
        r, n = _rays(rays)
        head = (self.h, n, r, _t_range(t_range, n))
        return self._paths_host("shade", head, (n,), params, depth, reflectance, bounce_t_min, want, count, smooth, None, shadow, visibility, ior, fresnel)

    def shade_paths_device(self, n, rays, params: abi.Params, depth, reflectance=0, bounce_t_min=1e-3, t_range=None, stream=0, rgb_linear=0, rgb8=0, seg_hit_id=0,
                           seg_t=0, seg_obj=0, seg_rgb_linear=0, seg_rays=0, shadow=None, visibility=None, ior=None, fresnel=None, side_hit_id=0, side_t=0,
                           side_rgb_linear=0, side_fresnel=0):
        """srt_shade_paths_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`, one launch.  The
        light table of `params` is a host array; `reflectance` is a DEVICE pointer to n_objects floats (0 = all 0); t_range a device
        pointer to n x 2 floats, or None; the seg_* outputs are depth x n rows, segment-major.  The flags are those of `params`.
        shadow, visibility: as in shade_paths.  ior: None, or a DEVICE pointer to n_objects floats (0 = no table): srt_shade_paths_refract_device.
        fresnel: None, or a DEVICE pointer to the n_objects floats of f0 (0 = no table): srt_shade_paths_fresnel_device; the side_* outputs are
        the depth x n rows of its srt_fresnel_out."""
        head = (self.h, n, rays, t_range or 0)
        self._paths_device("shade", head, params, depth, reflectance, bounce_t_min, stream, rgb_linear, rgb8, (seg_hit_id, seg_t, seg_obj, seg_rgb_linear, seg_rays),
                           shadow, visibility, ior, fresnel, (side_hit_id, side_t, side_rgb_linear, side_fresnel))

    def render_paths(self, params: abi.Params, depth, reflectance=None, bounce_t_min=1e-3,
                     want=("rgb_linear", "rgb8", "seg_hit_id", "seg_t", "seg_obj", "seg_rgb_linear", "seg_rays"), count=False, smooth=False, fill=None, shadow=None,
                     visibility=None, ior=None, fresnel=None):
        """srt_render_paths: shade_paths for the rays of the frame's own pixels -- the local pixels of a call with `params` (its block or
        tile deal, camera matrix and spp included); no ray array is built.  Returns a dict of the arrays named in `want` -- rgb_linear
        [rows, cols, 3] (mixed), rgb8 [rows, cols, 3], and per segment seg_hit_id / seg_t / seg_obj [depth, rows, cols], seg_rgb_linear
        [depth, rows, cols, 3], seg_rays [depth, rows, cols, 6] -- + 'stats'.  count / smooth add SRT_FLAG_COUNT_WORK /
        SRT_FLAG_SMOOTH_NORMALS for this call.  fill: a value every array holds before the call (padding pixels of a tile deal keep it).
        shadow, visibility, ior, fresnel: as in shade_paths; the side_* arrays and fresnel are [depth, rows, cols(, 3)]."""
        lead = (self.rows(params), self.cols(params))
        return self._paths_host("render", (self.h,), lead, params, depth, reflectance, bounce_t_min, want, count, smooth, fill, shadow, visibility, ior, fresnel)

    def render_paths_device(self, params: abi.Params, depth, reflectance=0, bounce_t_min=1e-3, stream=0, rgb_linear=0, rgb8=0, seg_hit_id=0, seg_t=0, seg_obj=0,
                            seg_rgb_linear=0, seg_rays=0, shadow=None, visibility=None, ior=None, fresnel=None, side_hit_id=0, side_t=0, side_rgb_linear=0,
                            side_fresnel=0):
        """srt_render_paths_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in, asynchronous on `stream`, one launch.  The
        light table of `params` is a host array; `reflectance` is a DEVICE pointer to n_objects floats (0 = all 0); the outputs are
        [rows, cols, ...] and the seg_* outputs [depth, rows, cols, ...] of the call's local pixels.  The flags are those of `params`.
        shadow, visibility: as in shade_paths.  ior, fresnel and the side_* outputs: as in shade_paths_device."""
        self._paths_device("render", (self.h,), params, depth, reflectance, bounce_t_min, stream, rgb_linear, rgb8, (seg_hit_id, seg_t, seg_obj, seg_rgb_linear, seg_rays),
                           shadow, visibility, ior, fresnel, (side_hit_id, side_t, side_rgb_linear, side_fresnel))

    def closest_points(self, points, radius=None, point_mask=None, count=False, want=("tri", "dist2", "point", "vw", "region")):
        """srt_closest_points: for every point of `points` (n x 3, host array) the nearest triangle within `radius` (n floats, one float for
        all, or None = +inf) and the nearest point on it.  Returns a dict of the arrays named in `want` -- tri n (-1: none within the
        radius), dist2 n (the squared distance, +inf: none), point n x 3, vw n x 2 (point = P1 + v e1 + w e2), region n uint8 (0 face, 1..3
        edges, 4..6 vertices) -- + 'stats'; count=True fills the node / triangle test counts.  The radius never shrinks during the walk: pass
        one for speed.  point_mask (n uint32, or None = all ones): only the objects whose mask (set_object_masks) shares a bit with the
        point's are searched."""
        return self._points("srt_closest_points", points, radius, point_mask, count, want)

    def _points(self, symbol, points, radius, point_mask, count, want):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (n,)), np.float32)
        pm = None if point_mask is None else _ray_mask(point_mask, n)
        out, _ = _outputs(want, (n,), _POINT)
        po = abi.PointOut(*_addresses(out, _POINT))
        return _with_stats(out, getattr(self.L, symbol), symbol, self.h, n, _host(pts, _f32p), _host(rad, _f32p), _host(pm, _u32p),
                           _query_flags(count=count), C.byref(po))

    def closest_points_device(self, n, d_points, radius=0, point_mask=0, stream=0, count=False, tri=0, dist2=0, point=0, vw=0, region=0):
        """srt_closest_points_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in -- the points (n x 3 floats), `radius` (n
        floats, 0 = +inf), `point_mask` (n uint32, 0 = all ones) and the outputs (0: not wanted) --, asynchronous on `stream`, one launch."""
        self._points_device("srt_closest_points_device", n, d_points, radius, point_mask, stream, count, (tri, dist2, point, vw, region))

    def _points_device(self, symbol, n, d_points, radius, point_mask, stream, count, outs):
        po = _wanted(abi.PointOut, *outs)
        _check(getattr(self.L, symbol)(self.h, n, d_points, radius or None, point_mask or None, _query_flags(count=count), stream, C.byref(po)), symbol)

    def nearest_points(self, points, radius=None, point_mask=None, count=False, want=("tri", "dist2", "point", "vw", "region")):
        """srt_nearest_points (include/srt_nearest.h): closest_points' arguments and closest_points' results, bit for bit, on every scene whose
        boxes nest -- but the walk also prunes by the best distance found so far, so no radius has to be chosen: None costs the
        neighbourhood of the answer, not the scene.  count=True: the counts are of the walk as it ran and depend on the batch."""
        return self._points("srt_nearest_points", points, radius, point_mask, count, want)

    def nearest_points_device(self, n, d_points, radius=0, point_mask=0, stream=0, count=False, tri=0, dist2=0, point=0, vw=0, region=0):
        """srt_nearest_points_device: closest_points_device's arguments, asynchronous on `stream`, one launch."""
        self._points_device("srt_nearest_points_device", n, d_points, radius, point_mask, stream, count, (tri, dist2, point, vw, region))

    def signed_points(self, points, radius=None, point_mask=None, dirs=None, parity=False, count=False,
                      want=("sdist", "inside", "winding", "crossings", "tri", "dist2", "point", "vw", "region")):
        """srt_signed_points (include/srt_signed.h): nearest_points' arguments and results, and per point a sign by winding along the rays
        (point, dirs[j]): sdist n (-sqrt(dist2) inside, +sqrt(dist2) outside), inside n uint8, winding n x n_dirs int32 (exits - entries),
        crossings n x n_dirs uint32.  dirs: n_dirs x 3 floats (1 .. 16 directions), or None = the header's three.  parity=True votes by
        crossings & 1 instead of winding > 0.  The sign does not depend on the radius; want=("inside",) runs no nearest phase at all.
        count=True: the sign rays' tests are stats' node_tests_shadow / tri_tests_shadow, the nearest phase's the primary pair."""
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n = pts.shape[0]
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (n,)), np.float32)
        pm = None if point_mask is None else _ray_mask(point_mask, n)
        d = None if dirs is None else np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        nd = 3 if d is None else d.shape[0]
        out, _ = _outputs(want, (n,), _POINT)
        so, _ = _outputs(want, (n,), {k: (ty, tail if tail is not None else (nd,)) for k, (ty, tail) in _SIGN.items()})
        sign = abi.Sign(None if d is None else d.ctypes.data, 0 if d is None else nd, abi.SIGN_PARITY if parity else 0)
        po, sg = abi.PointOut(*_addresses(out, _POINT)), abi.SignOut(*_addresses(so, _SIGN))
        return _with_stats({**so, **out}, self.L.srt_signed_points, "srt_signed_points", self.h, n, _host(pts, _f32p), _host(rad, _f32p), _host(pm, _u32p),
                           C.byref(sign), _query_flags(count=count), C.byref(po), C.byref(sg))

    def signed_points_device(self, n, d_points, radius=0, point_mask=0, dirs=0, n_dirs=0, parity=False, stream=0, count=False, sdist=0, inside=0, winding=0,
                             crossings=0, tri=0, dist2=0, point=0, vw=0, region=0):
        """srt_signed_points_device: raw device pointers (ints) in -- nearest_points_device's, `dirs` (n_dirs x 3 floats on the device; 0 with
        n_dirs 0 = the header's three) and the sign outputs (winding, crossings: n x n_dirs) --, asynchronous on `stream`, one launch."""
        sign = abi.Sign(dirs or None, n_dirs, abi.SIGN_PARITY if parity else 0)
        po, sg = _wanted(abi.PointOut, tri, dist2, point, vw, region), _wanted(abi.SignOut, sdist, inside, winding, crossings)
        _check(self.L.srt_signed_points_device(self.h, n, d_points, radius or None, point_mask or None, C.byref(sign), _query_flags(count=count), stream,
                                               C.byref(po), C.byref(sg)), "srt_signed_points_device")

    def closest_points_multi(self, points, k, radius=None, point_mask=None, count=False,
                             want=("n_within", "n_found", "tri", "dist2", "point", "vw", "region")):
        """srt_closest_points_multi (include/srt_points_multi.h): closest_points' arguments, and per point the k nearest triangles within
        `radius`, nearest first, equal dist2 by lowest id (k = 1 .. POINT_MULTI_MAX).  Returns a dict of the arrays named in `want` --
        n_within n uint32 (ALL triangles within the radius; it may exceed k), n_found n uint32 (the filled columns, min(k, n_within)),
        tri n x k (-1: an empty column), dist2 n x k (+inf), point n x k x 3, vw n x k x 2, region n x k -- + 'stats'.  Column 0 is
        closest_points' result; the radius never shrinks, and the counts under count=True are closest_points'."""
        return self._points_multi("srt_closest_points_multi", points, k, radius, point_mask, count, want)

    def nearest_points_multi(self, points, k, radius=None, point_mask=None, count=False, want=("n_found", "tri", "dist2", "point", "vw", "region")):
        """srt_nearest_points_multi: closest_points_multi's columns and n_found, bit for bit, on every scene whose boxes nest -- but the walk
        also prunes by the k-th best distance found so far, so no radius has to be chosen.  There is no n_within under pruning: naming it
        in `want` is an error.  count=True: the counts are of the walk as it ran and depend on the batch."""
        return self._points_multi("srt_nearest_points_multi", points, k, radius, point_mask, count, want)

    def _points_multi(self, symbol, points, k, radius, point_mask, count, want):
        pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        n, k = pts.shape[0], int(k)
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (n,)), np.float32)
        pm = None if point_mask is None else _ray_mask(point_mask, n)
        spec = {key: (ty, ()) if c is None else (ty, (max(k, 0),) + (() if c == 1 else (c,))) for key, (ty, c) in abi.POINT_MULTI_FIELDS.items()}
        out, _ = _outputs(want, (n,), spec)
        po = abi.PointMultiOut(*_addresses(out, spec))
        return _with_stats(out, getattr(self.L, symbol), symbol, self.h, n, _host(pts, _f32p), _host(rad, _f32p), _host(pm, _u32p), k,
                           _query_flags(count=count), C.byref(po))

    def closest_points_multi_device(self, n, d_points, k, radius=0, point_mask=0, stream=0, count=False, n_within=0, n_found=0, tri=0, dist2=0, point=0, vw=0,
                                    region=0):
        """srt_closest_points_multi_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in -- closest_points_device's, and the
        outputs (n_within, n_found: n; the others n x k rows; 0: not wanted) --, asynchronous on `stream`, one launch."""
        self._points_multi_device("srt_closest_points_multi_device", n, d_points, k, radius, point_mask, stream, count, (n_within, n_found, tri, dist2, point, vw, region))

    def nearest_points_multi_device(self, n, d_points, k, radius=0, point_mask=0, stream=0, count=False, n_found=0, tri=0, dist2=0, point=0, vw=0, region=0):
        """srt_nearest_points_multi_device: closest_points_multi_device's arguments without n_within, asynchronous on `stream`, one launch."""
        self._points_multi_device("srt_nearest_points_multi_device", n, d_points, k, radius, point_mask, stream, count, (0, n_found, tri, dist2, point, vw, region))

    def _points_multi_device(self, symbol, n, d_points, k, radius, point_mask, stream, count, outs):
        po = _wanted(abi.PointMultiOut, *outs)
        _check(getattr(self.L, symbol)(self.h, n, d_points, radius or None, point_mask or None, k, _query_flags(count=count), stream, C.byref(po)), symbol)

    def closest_segments(self, segments, radius=None, seg_mask=None, count=False, want=("tri", "dist2", "s", "point", "vw", "feature")):
        """srt_closest_segments (include/srt_segments.h): for every segment of `segments` (n x 6, host array: A, B) the nearest triangle
        within `radius` (n floats, one float for all, or None = +inf) of the segment.  Returns a dict of the arrays named in `want` -- tri n
        (-1: none within the radius), dist2 n (+0: the segment crosses the triangle, +inf: none), s n (the segment's closest point is
        A + (B - A) s), point n x 3 (the closest point on the triangle), vw n x 2 (point = P1 + v e1 + w e2), feature n uint8 (0 / 1 end A / B,
        2 / 3 / 4 triangle edge 1-2 / 2-3 / 1-3, 5 a crossing) -- + 'stats'; count=True fills the node / triangle test counts.  The radius
        never shrinks during the walk.  seg_mask (n uint32, or None = all ones): as closest_points' point_mask."""
        seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 6)
        n = seg.shape[0]
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (n,)), np.float32)
        sm = None if seg_mask is None else _ray_mask(seg_mask, n)
        out, _ = _outputs(want, (n,), _SEGMENT)
        so = abi.SegmentOut(*_addresses(out, _SEGMENT))
        return _with_stats(out, self.L.srt_closest_segments, "srt_closest_segments", self.h, n, _host(seg, _f32p), _host(rad, _f32p), _host(sm, _u32p),
                           _query_flags(count=count), C.byref(so))

    def closest_segments_device(self, n, d_segments, radius=0, seg_mask=0, stream=0, count=False, tri=0, dist2=0, s=0, point=0, vw=0, feature=0):
        """srt_closest_segments_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()) in -- the segments (n x 6 floats), `radius` (n
        floats, 0 = +inf), `seg_mask` (n uint32, 0 = all ones) and the outputs (0: not wanted) --, asynchronous on `stream`, one launch."""
        so = _wanted(abi.SegmentOut, tri, dist2, s, point, vw, feature)
        _check(self.L.srt_closest_segments_device(self.h, n, d_segments, radius or None, seg_mask or None, _query_flags(count=count), stream, C.byref(so)),
               "srt_closest_segments_device")

    def sync(self):
        return _with_stats({}, self.L.srt_sync, "srt_sync", self.h)["stats"]


class FrameBatch:
    """The argument tables of one srt_render_device_batch call, built once (a step of a bench or an orbit re-issues the same call):
    `scenes` are distinct DeviceScenes, `params` one abi.Params per frame, the outputs lists of raw device pointers (ints) or None."""

    def __init__(self, scenes, params, hit_id=None, t=None, rgb_linear=None, rgb8=None):
        n = len(scenes)
        assert len(params) == n
        self.L, self.n, self.scenes = load(), n, list(scenes)
        self.h = (C.c_void_p * n)(*[s.h for s in scenes])
        self.p = (abi.Params * n)()
        for i, q in enumerate(params):
            C.memmove(C.byref(self.p[i]), C.byref(q), C.sizeof(abi.Params))
        self._keep = list(params)             # the light arrays the params point to
        def table(v):
            if v is None:
                return None
            assert len(v) == n
            return (C.c_void_p * n)(*[C.c_void_p(int(x) if x else 0) for x in v])
        self.out = [table(v) for v in (hit_id, t, rgb_linear, rgb8)]

    def render(self, stream=0):
        _check(self.L.srt_render_device_batch(self.n, self.h, self.p, stream, *self.out), "srt_render_device_batch")


def _f(a):
    return np.ascontiguousarray(a, np.float32)


# the arrays a call can return: name -> (dtype, the shape of one ray's or pixel's entry)
_HIT = {"hit_id": (np.int32, ()), "t": (np.float32, ())}
_CLOSEST = {**_HIT, "bary": (np.float32, (3,))}
_FRAME = {**_HIT, "rgb_linear": (np.float32, (3,)), "rgb8": (np.uint8, (3,))}
_SURFACE = {k: (ty, () if c == 1 else (c,)) for k, (ty, c) in abi.SURFACE_FIELDS.items()}
_POINT = {k: (ty, () if c == 1 else (c,)) for k, (ty, c) in abi.POINT_FIELDS.items()}
_SEGMENT = {k: (ty, () if c == 1 else (c,)) for k, (ty, c) in abi.SEGMENT_FIELDS.items()}
_SIGN = {k: (ty, None if c is None else ()) for k, (ty, c) in abi.SIGN_FIELDS.items()}      # (None: one entry per direction)
_PATH_SUMS = {"rgb_linear": (np.float32, (3,)), "rgb8": (np.uint8, (3,))}
_PATH_SEGMENTS = {"seg_" + k: (ty, () if c == 1 else (c,)) for k, (ty, c) in abi.PATH_FIELDS.items()}
# the rows of srt_fresnel_out as result keys: side_hit_id, side_t, side_rgb_linear, fresnel
_PATH_SIDE = {("fresnel" if k == "fresnel" else "side_" + k): (ty, () if c == 1 else (c,)) for k, (ty, c) in abi.FRESNEL_FIELDS.items()}
_POINTER = {np.int32: _i32p, np.float32: _f32p, np.uint8: _u8p, np.uint32: _u32p}


def _outputs(want, lead, spec, fill=None):
    """Host arrays for the entries of `spec` that `want` names, each of shape lead + its own and holding `fill` where one is given.
    Returns (name -> array, g): g(name) is the array as a pointer of its type, or that type's NULL where it is not wanted."""
    new = np.empty if fill is None else (lambda shape, ty: np.full(shape, fill, ty))
    out = {k: new(lead + tail, ty) for k, (ty, tail) in spec.items() if k in want}
    return out, lambda k: out[k].ctypes.data_as(_POINTER[spec[k][0]]) if k in out else _POINTER[spec[k][0]]()


def _addresses(out, spec):
    """The arrays of `out` in the order of `spec`, as addresses (None: not wanted): the fields of an srt_surface_out or srt_path_out."""
    return [out[k].ctypes.data if k in out else None for k in spec]


class _flags:
    """params.flags with SRT_FLAG_COUNT_WORK / SRT_FLAG_SMOOTH_NORMALS added for the call inside the `with`, and as they were after it, also
    when it raises."""

    def __init__(self, params, count=False, smooth=False):
        self.params, self.extra = params, _query_flags(smooth, count)

    def __enter__(self):
        self.flags = self.params.flags
        self.params.flags = self.flags | self.extra

    def __exit__(self, *exc):
        self.params.flags = self.flags


def _host(a, ty):
    """A host array as the pointer a host entry point takes (the pointer keeps the array alive), or None for None."""
    return a.ctypes.data_as(ty) if a is not None else None


def _array(a, dtype):
    """An optional host array as a C-contiguous array of `dtype`, or None for None."""
    return None if a is None else np.ascontiguousarray(a, dtype)


def _rays(rays):
    """The rays of a host form (n x 6 float32) as the pointer it takes, and n."""
    r = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
    return _host(r, _f32p), r.shape[0]


def _hits(hit_id, t, n, what="hit_id, t: one entry per ray"):
    """The caller's hits of a host form, n of each, as the two pointers it takes."""
    hid, tt = np.ascontiguousarray(hit_id, np.int32).reshape(-1), np.ascontiguousarray(t, np.float32).reshape(-1)
    assert hid.shape[0] == n and tt.shape[0] == n, what
    return _host(hid, _i32p), _host(tt, _f32p)


def _query_flags(smooth=False, count=False):
    return (abi.SRT_FLAG_SMOOTH_NORMALS if smooth else 0) | (abi.SRT_FLAG_COUNT_WORK if count else 0)


def _with_stats(out, fn, name, *args):
    """A host form that ends in an srt_stats*: fn(*args, &stats), checked; returns `out` with the stats under 'stats'."""
    st = abi.Stats()
    _check(fn(*args, C.byref(st)), name)
    out["stats"] = st.as_dict()
    return out


def _wanted(struct, *addresses):
    """An out struct of a _device form over the caller's device addresses (0: not wanted)."""
    return struct(*(a or None for a in addresses))


def _host_mask(ray_mask, n):
    """The `mask` of _ray_call for a host form: None, or the masks of n rays as a pointer (NULL for True: all ones)."""
    return None if ray_mask is None else (_host(_ray_mask(ray_mask, n), _u32p),)


def _device_mask(ray_mask):
    """The `mask` of _ray_call for a _device form: None, or the device address of the masks (0: all ones)."""
    return None if ray_mask is None else (ray_mask or 0,)


def _ray_call(L, stem, suffix, t_range, mask):
    """Which form of a ray call its optional arguments ask for: per-ray masks (`mask` not None: a 1-tuple of them, as the C call takes
    them) the _masked form, else intervals (`t_range` not None) the _range form, else the call itself.  Returns (the C function, its
    name, the arguments it takes between the rays and the rest)."""
    if mask is not None:
        form, mid = "_masked", (t_range, *mask)
    elif t_range is not None:
        form, mid = "_range", (t_range,)
    else:
        form, mid = "", ()
    name = stem + form + suffix
    return getattr(L, name), name, mid


def _path_call(L, kind, suffix, rule, vis, refr, fres=None):
    """Which form of srt_<kind>_paths (kind: shade | render; suffix: "" | _device) its optional structs ask for: a Fresnel table the
    _fresnel form, else a refraction the _refract form, else masks the _masked form, else a rule the _shadow form, else the call itself.  Returns (the C function, its name,
    the arguments it takes between the path desc and the outputs)."""
    ref = lambda v: C.byref(v) if v is not None else None
    if fres is not None:
        form, mid = "_fresnel", (ref(rule), ref(vis), ref(refr), C.byref(fres))
    elif refr is not None:
        form, mid = "_refract", (ref(rule), ref(vis), C.byref(refr))
    elif vis is not None:
        form, mid = "_masked", (ref(rule), C.byref(vis))
    elif rule is not None:
        form, mid = "_shadow", (C.byref(rule),)
    else:
        form, mid = "", ()
    name = "srt_" + kind + "_paths" + form + suffix
    return getattr(L, name), name, mid


def _refraction(ior, n_objects):
    """(an abi.Refraction over a host table of n_objects floats, the array that keeps it alive), or (None, None) for None."""
    if ior is None:
        return None, None
    table = np.ascontiguousarray(ior, np.float32).reshape(-1)
    assert table.shape[0] == n_objects, "ior: one float per object"
    return abi.Refraction(table.ctypes.data, 0), table


def schlick_f0(ior):
    """The reflectance at normal incidence of a dielectric of index n in air, ((n - 1) / (n + 1))^2 as float32: the f0 of the Fresnel
    split for a table of float32 indices (an entry that does not transmit, n <= 0 or NaN, gets -1: no split).  The quotient and the
    square are taken in float64 and rounded once, so that an index of 1.5 gives float32(0.04), not its neighbour."""
    n = np.asarray(ior, np.float32)
    with np.errstate(all="ignore"):
        q = (n.astype(np.float64) - 1.0) / (n.astype(np.float64) + 1.0)
        f = (q * q).astype(np.float32)
    return np.where(n > np.float32(0.0), f, np.float32(-1.0)).astype(np.float32)


def _vis_ref(visibility):
    """None, a Visibility or (primary, bounce, shadow) as the srt_visibility* a call takes (None: NULL)."""
    v = abi.visibility(visibility)
    return C.byref(v) if v is not None else None


def _ao_desc(dirs, t_min, t_max, skip_self):
    """(an abi.AoDesc over a host table of K x 3 floats, the array that keeps it alive)."""
    table = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    return abi.AoDesc(table.shape[0], table.ctypes.data, t_min, t_max, abi.SRT_AO_SKIP_SELF if skip_self else 0), table


def _ao_out(want, n, n_dirs):
    """(an abi.AoOut over host arrays for the fields of srt_ao_out that `want` names, name -> array)."""
    shape = {"n_occluded": (n,), "ao": (n,), "occ_bits": (n, (n_dirs + 31) // 32)}
    out = {k: np.empty(shape[k], ty) for k, ty in abi.AO_FIELDS.items() if k in want}
    return abi.AoOut(*_addresses(out, abi.AO_FIELDS)), out


def _ao_frame(rot):
    """(an abi.AoFrame over a host table of h x w x 2 floats, the array that keeps it alive); rot None: no rotation."""
    if rot is None:
        return abi.AoFrame(0, 0, None), None
    table = np.ascontiguousarray(rot, np.float32)
    assert table.ndim == 3 and table.shape[2] == 2, "rot: h x w x 2 (cos, sin)"
    return abi.AoFrame(table.shape[1], table.shape[0], table.ctypes.data), table


def _ao_frame_out(want, lead, n_dirs, fill=None):
    """(an abi.AoFrameOut over host arrays for the fields of srt_ao_frame_out that `want` names, name -> array [rows, cols(, k)])."""
    new = np.empty if fill is None else (lambda shape, ty: np.full(shape, fill, ty))
    tail = lambda c: () if c == 1 else ((n_dirs + 31) // 32,) if c is None else (c,)
    out = {k: new(lead + tail(c), ty) for k, (ty, c) in abi.AO_FRAME_FIELDS.items() if k in want}
    return abi.AoFrameOut(*_addresses(out, abi.AO_FRAME_FIELDS)), out


def ao_rotations(w, h):
    """A deterministic h x w x 2 table of rotations (cos, sin) for render_ao / render_ao_hits (float32), computed in float64 and rounded
    once: entry k = iy * w + ix has the angle 2 pi frac((k + 0.5) * 0.6180339887498949) -- the golden-ratio sequence, so that neighbouring
    pixels of a small tile get well-separated turns of the direction table."""
    k = np.arange(int(w) * int(h), dtype=np.float64)
    a = 2.0 * np.pi * np.modf((k + 0.5) * 0.6180339887498949)[0]
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(np.float32).reshape(int(h), int(w), 2)


def ao_directions(n, cosine=True):
    """A deterministic table of n unit directions over the hemisphere z >= 0 for ao_rays / ao_hits (n x 3 float32), computed in float64 and
    rounded once: direction i has radius r = sqrt((i + 0.5) / n) in the xy plane at the golden-angle azimuth (i + 0.5) * pi * (3 - sqrt(5)) and
    z = sqrt(1 - r * r) -- cosine-distributed, so that the plain count is cosine-weighted.  cosine=False: uniform over the hemisphere,
    z = 1 - (i + 0.5) / n and r = sqrt(1 - z * z)."""
    i = np.arange(int(n), dtype=np.float64)
    u = (i + 0.5) / float(n)
    if cosine:
        r = np.sqrt(u); z = np.sqrt(1.0 - r * r)
    else:
        z = 1.0 - u; r = np.sqrt(1.0 - z * z)
    phi = (i + 0.5) * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def _ray_mask(ray_mask, n):
    """The masks of n rays as a host array (n uint32), or None for True (all ones: the masked call without per-ray masks)."""
    if ray_mask is True:
        return None
    rm = np.ascontiguousarray(ray_mask, np.uint32).reshape(-1)
    assert rm.shape[0] == n, "ray_mask: one uint32 per ray"
    return rm


def _t_range(t_range, n):
    """The t intervals of n rays (n x 2 float32) as the pointer a host form takes, or None."""
    if t_range is None:
        return None
    tr = np.ascontiguousarray(t_range, np.float32).reshape(-1, 2)
    assert tr.shape[0] == n, "t_range: one (t_min, t_max) per ray"
    return _host(tr, _f32p)


def kat_ray_aabb(ray_od, box, device=0):
    """Device slab test on vectors: returns (literal, branch-free, filtered, ambiguous) uint8 arrays."""
    L = load(); ray_od, box = _f(ray_od), _f(box); n = ray_od.shape[0]
    outs = [np.empty(n, np.uint8) for _ in range(4)]
    _check(L.srt_kat_ray_aabb(device, n, ray_od.ctypes.data_as(_f32p), box.ctypes.data_as(_f32p), *[o.ctypes.data_as(_u8p) for o in outs]), "srt_kat_ray_aabb")
    return outs


def kat_ray_triangle(ray_od, tri_points, device=0):
    L = load(); ray_od, tri_points = _f(ray_od), _f(tri_points); n = ray_od.shape[0]; t = np.empty(n, np.float32)
    _check(L.srt_kat_ray_triangle(device, n, ray_od.ctypes.data_as(_f32p), tri_points.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p)), "srt_kat_ray_triangle")
    return t


def kat_ray_triangle_origin(dir3, tri_points, device=0):
    """The origin form of the triangle test (what primary rays run): directions n x 3, the record derived as srt_scene_create does."""
    L = load(); dir3, tri_points = _f(dir3), _f(tri_points); n = dir3.shape[0]; t = np.empty(n, np.float32)
    _check(L.srt_kat_ray_triangle_origin(device, n, dir3.ctypes.data_as(_f32p), tri_points.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p)), "srt_kat_ray_triangle_origin")
    return t


def kat_barycentric(in15, device=0):
    L = load(); in15 = _f(in15); n = in15.shape[0]; out = np.empty((n, 3), np.float32)
    _check(L.srt_kat_barycentric(device, n, in15.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p)), "srt_kat_barycentric")
    return out


def kat_phong(in28, device=0):
    L = load(); in28 = _f(in28); n = in28.shape[0]; rgb = np.empty((n, 3), np.float32)
    _check(L.srt_kat_phong(device, n, in28.ctypes.data_as(_f32p), rgb.ctypes.data_as(_f32p)), "srt_kat_phong")
    return rgb


def kat_tonemap(lin, reinhard=0.5, gamma=1.1, device=0):
    L = load(); lin = _f(lin).reshape(-1, 3); n = lin.shape[0]
    tone = np.empty((n, 3), np.float32); q = np.empty((n, 3), np.int32)
    _check(L.srt_kat_tonemap(device, n, lin.ctypes.data_as(_f32p), reinhard, gamma, tone.ctypes.data_as(_f32p), q.ctypes.data_as(_i32p)), "srt_kat_tonemap")
    return tone, q


def kat_tone_filter(lin, reinhard=0.5, gamma=1.1, device=0):
    """(q, q_filter, decided) per value of `lin` (flat): the quantised tone map as the shading kernels compute it, the f32 filter's own
    candidate (-1 where it decided nothing) and whether the filter alone decided (srt_kat_tone_filter)."""
    L = load(); lin = _f(lin).reshape(-1); n = lin.shape[0]
    q = np.empty(n, np.int32); qf = np.empty(n, np.int32); dec = np.empty(n, np.uint8)
    _check(L.srt_kat_tone_filter(device, n, lin.ctypes.data_as(_f32p), reinhard, gamma, q.ctypes.data_as(_i32p), qf.ctypes.data_as(_i32p), dec.ctypes.data_as(_u8p)),
           "srt_kat_tone_filter")
    return q, qf, dec.astype(bool)


def kat_tone_filter_sweep(first_bits, last_bits, reinhard=0.5, gamma=1.1, device=0):
    """Every float with a bit pattern in [first_bits, last_bits] through the filter and the exact functions on the device
    (srt_kat_tone_filter_sweep): dict of values, undecided, decided_different, results_different, max_deviation, max_deviation_over_margin."""
    L = load()
    out = (C.c_double * 6)()
    _check(L.srt_kat_tone_filter_sweep(device, first_bits, last_bits, reinhard, gamma, out), "srt_kat_tone_filter_sweep")
    return {"values": int(out[0]), "undecided": int(out[1]), "decided_different": int(out[2]), "results_different": int(out[3]),
            "max_deviation": float(out[4]), "max_deviation_over_margin": float(out[5])}


def kat_interp_normal(in12, device=0):
    L = load(); in12 = _f(in12); n = in12.shape[0]; out = np.empty((n, 3), np.float32)
    _check(L.srt_kat_interp_normal(device, n, in12.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p)), "srt_kat_interp_normal")
    return out


def valu_rate(iters=2000, device=0):
    """(wave-instructions per SIMD-cycle, shader clock in GHz, the same rate over the whole launch span, waves per SIMD): srt_debug_valu_rate."""
    L = load()
    out = (C.c_double * 4)()
    _check(L.srt_debug_valu_rate(device, iters, out), "srt_debug_valu_rate")
    return float(out[0]), float(out[1]), float(out[2]), float(out[3])


def kat_pow(x, y, device=0):
    """The device powf on vectors: (shipped form, (float)pow(double)(x, y))."""
    L = load(); x, y = _f(x), _f(y); n = x.shape[0]; a = np.empty(n, np.float32); b = np.empty(n, np.float32)
    _check(L.srt_kat_pow(device, n, x.ctypes.data_as(_f32p), y.ctypes.data_as(_f32p), a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p)), "srt_kat_pow")
    return a, b
