"""ctypes mirror of include/srt.h -- its structs (STRUCTS), constants (SRT_*) and prototypes (PROTOTYPES), checked against the header by
tests/test_abi_mirror.py --, of its extension headers include/srt_points.h (POINT_STRUCTS, POINT_PROTOTYPES; tests/test_point_ref.py),
include/srt_nearest.h (NEAREST_PROTOTYPES; tests/test_nearest_ref.py), include/srt_signed.h (SIGNED_STRUCTS, SIGNED_PROTOTYPES;
tests/test_sign_ref.py), include/srt_points_multi.h (POINT_MULTI_STRUCTS, POINT_MULTI_PROTOTYPES; tests/test_points_multi_ref.py) and
include/srt_segments.h (SEGMENT_STRUCTS, SEGMENT_PROTOTYPES; tests/test_segment_ref.py), and a numpy container for the flat scene.

The flat scene is the reference's ObjectManager state (Object.h:59-89 in the reference) written out as
arrays; see include/srt.h for the layout contract.  This module holds no compute.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

SRT_ABI_VERSION = 3
SRT_OK = 0
SRT_ERR_ARG, SRT_ERR_LAYOUT, SRT_ERR_DEVICE, SRT_ERR_NO_GPU, SRT_ERR_TEXTURE, SRT_ERR_LIMIT, SRT_ERR_OOM = 1, 2, 3, 4, 5, 6, 7
SRT_FLAG_SMOOTH_NORMALS = 1 << 0
SRT_FLAG_COUNT_WORK = 1 << 1
SRT_FLAG_NO_TIMING = 1 << 2
SRT_FLAG_FRAMES_IN_FLIGHT = 1 << 3      # hint: other frames are in flight on the device (srt.h)

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_u8p = C.POINTER(C.c_uint8)


class SceneDesc(C.Structure):
    _fields_ = [
        ("n_objects", C.c_uint32), ("n_nodes", C.c_uint32), ("n_tris", C.c_uint32), ("n_textures", C.c_uint32),
        ("node_min", _f32p), ("node_max", _f32p),
        ("node_left", _i32p), ("node_right", _i32p), ("node_first", _i32p), ("node_count", _i32p),
        ("obj_root", _u32p),
        ("tri_points", _f32p), ("tri_obj", _i32p), ("tri_tex", _i32p), ("tri_texcoord", _f32p), ("tri_normals", _f32p),
        ("obj_color", _f32p), ("obj_material", _f32p),
        ("tex_rgb", _u8p), ("tex_off", _u64p), ("tex_w", _u32p), ("tex_h", _u32p),
    ]


class FrameGeometry(C.Structure):
    """srt_frame_geometry (include/srt.h, f1 device half): per-object pointer tables."""
    _fields_ = [
        ("n_objects", C.c_uint32),
        ("obj_n_tris", _u32p), ("obj_n_nodes", _u32p),
        ("obj_points", C.POINTER(_f32p)), ("obj_order", C.POINTER(_u32p)), ("obj_node_min", C.POINTER(_f32p)), ("obj_node_max", C.POINTER(_f32p)),
        ("obj_color", _f32p), ("obj_material", _f32p),
    ]


class RefitDesc(C.Structure):
    """srt_refit_desc (include/srt.h, REFIT): the caller's device buffers as addresses; n_verts 0 = the direct form."""
    _fields_ = [("n_verts", C.c_uint32), ("stride", C.c_uint32), ("d_points", C.c_void_p), ("d_normals", C.c_void_p)]


class Params(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("block_rows", C.c_uint32), ("block_first", C.c_uint32), ("block_stride", C.c_uint32), ("block_cols", C.c_uint32),
        ("focal", C.c_float),
        ("n_lights", C.c_uint32), ("light_pos", _f32p), ("ray_matrix", _f32p),
        ("shadow_div", C.c_float), ("reinhard", C.c_float), ("gamma", C.c_float),
        ("background", C.c_uint8 * 4),
        ("spp", C.c_uint32), ("flags", C.c_uint32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("primary_rays", C.c_uint64), ("hit_rays", C.c_uint64), ("shadow_rays", C.c_uint64),
        ("node_tests_primary", C.c_uint64), ("tri_tests_primary", C.c_uint64),
        ("node_tests_shadow", C.c_uint64), ("tri_tests_shadow", C.c_uint64),
        ("ms_primary", C.c_float), ("ms_shadow", C.c_float), ("ms_shade", C.c_float), ("ms_total", C.c_float),
        ("launches", C.c_uint32), ("rows", C.c_uint32),
    ]

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_}
        d["node_tests"] = d["node_tests_primary"] + d["node_tests_shadow"]
        d["tri_tests"] = d["tri_tests_primary"] + d["tri_tests_shadow"]
        return d


class SurfaceOut(C.Structure):
    """srt_surface_out: the arrays a surface query fills, as addresses (host arrays in the host forms, device pointers in the _device
    forms); 0 = not wanted."""
    _fields_ = [("obj", C.c_void_p), ("point", C.c_void_p), ("normal", C.c_void_p), ("color", C.c_void_p), ("material", C.c_void_p), ("bounce", C.c_void_p)]


SRT_MULTI_HIT_MAX = 16
SRT_PATH_DEPTH_MAX = 8


class PathDesc(C.Structure):
    """srt_path_desc: segments per ray, the lower bound of a mirrored ray's interval, the per-object reflectance table as an address
    (a host array in the host form, a device pointer in the _device form; 0 = all 0)."""
    _fields_ = [("depth", C.c_uint32), ("bounce_t_min", C.c_float), ("reflectance", C.c_void_p)]


class PathOut(C.Structure):
    """srt_path_out: the per-segment arrays of srt_shade_paths (segment-major, depth x n rows), as addresses; 0 = not wanted."""
    _fields_ = [("hit_id", C.c_void_p), ("t", C.c_void_p), ("obj", C.c_void_p), ("rgb_linear", C.c_void_p), ("rays", C.c_void_p)]


SRT_SHADOW_SELF = 1


class ShadowRule(C.Structure):
    """srt_shadow_rule: a shadow ray blocks only inside the closed (t_min, t_max), in units of light - hit point (t = 1 is the light);
    flags: 0, or SRT_SHADOW_SELF = the hit object's own tree is walked too."""
    _fields_ = [("t_min", C.c_float), ("t_max", C.c_float), ("flags", C.c_uint32)]


def shadow_rule(shadow):
    """None, a ShadowRule, or (t_min, t_max, self_shadow) -> a ShadowRule, or None."""
    if shadow is None or isinstance(shadow, ShadowRule):
        return shadow
    t_min, t_max, self_shadow = shadow
    return ShadowRule(t_min, t_max, SRT_SHADOW_SELF if self_shadow else 0)


class Visibility(C.Structure):
    """srt_visibility: the object mask a walk of each ray KIND is made with -- segment 0, every later segment, every shadow ray.  Object k
    takes part in a walk with mask m iff (obj_mask[k] & m) != 0 (DeviceScene.set_object_masks; all ones until set)."""
    _fields_ = [("primary", C.c_uint32), ("bounce", C.c_uint32), ("shadow", C.c_uint32)]


def visibility(vis):
    """None, a Visibility, or (primary, bounce, shadow) -> a Visibility, or None."""
    if vis is None or isinstance(vis, Visibility):
        return vis
    primary, bounce, shadow = vis
    return Visibility(int(primary) & 0xFFFFFFFF, int(bounce) & 0xFFFFFFFF, int(shadow) & 0xFFFFFFFF)


class Refraction(C.Structure):
    """srt_refraction: the per-object table of the refracting path calls.  ior: n_objects floats (a host array's pointer in the host forms,
    a device pointer in the _device forms); object k transmits iff ior[k] > 0, else it mirrors.  flags: 0."""
    _fields_ = [("ior", C.c_void_p), ("flags", C.c_uint32)]


class FresnelOut(C.Structure):
    """srt_fresnel_out: the per-segment rows of the side rays of the _fresnel path calls (segment-major, depth x n rows, laid out as
    srt_path_out's hit_id, t and rgb_linear), as addresses; 0 = not wanted."""
    _fields_ = [("hit_id", C.c_void_p), ("t", C.c_void_p), ("rgb_linear", C.c_void_p), ("fresnel", C.c_void_p)]


class Fresnel(C.Structure):
    """srt_fresnel: the per-object table of the Fresnel split.  f0: n_objects floats, the reflectance at normal incidence (a host array's
    pointer in the host forms, a device pointer in the _device forms); object k splits iff ior[k] > 0 and f0[k] >= 0.  flags: 0.  out: the
    address of a FresnelOut, or 0."""
    _fields_ = [("f0", C.c_void_p), ("flags", C.c_uint32), ("out", C.POINTER(FresnelOut))]


# srt_fresnel_out's fields: name -> (numpy type, components per row)
FRESNEL_FIELDS = {"hit_id": (np.int32, 1), "t": (np.float32, 1), "rgb_linear": (np.float32, 3), "fresnel": (np.float32, 1)}

SRT_AO_DIRS_MAX = 1024
SRT_AO_SKIP_SELF = 1


class AoDesc(C.Structure):
    """srt_ao_desc: the direction table of an ambient-occlusion call as an address (n_dirs x 3 floats in the hit's local frame, z along the
    facing normal; a host array in the host forms, a device pointer in the _device forms), the closed interval every AO ray blocks in, and
    flags: 0, or SRT_AO_SKIP_SELF = the hit object's own tree is left out of the AO walks."""
    _fields_ = [("n_dirs", C.c_uint32), ("dirs", C.c_void_p), ("t_min", C.c_float), ("t_max", C.c_float), ("flags", C.c_uint32)]


class AoOut(C.Structure):
    """srt_ao_out: the arrays an ambient-occlusion call fills, as addresses; 0 = not wanted."""
    _fields_ = [("n_occluded", C.c_void_p), ("ao", C.c_void_p), ("occ_bits", C.c_void_p)]


# the fields of srt_ao_out: name -> dtype (n_occluded and ao: one entry a ray; occ_bits: (n_dirs + 31) // 32 words a ray)
AO_FIELDS = {"n_occluded": np.uint32, "ao": np.float32, "occ_bits": np.uint32}

SRT_AO_ROT_MAX = 64


class AoFrame(C.Structure):
    """srt_ao_frame: the rotation table of an ambient-occlusion frame call as an address (rot_h x rot_w x 2 floats (c, s), row-major; a host
    array in the host forms, a device pointer in the _device forms); 0, 0 and no address: no rotation."""
    _fields_ = [("rot_w", C.c_uint32), ("rot_h", C.c_uint32), ("rot", C.c_void_p)]


class AoFrameOut(C.Structure):
    """srt_ao_frame_out: the arrays an ambient-occlusion frame call fills, as addresses; 0 = not wanted."""
    _fields_ = [("n_occluded", C.c_void_p), ("ao", C.c_void_p), ("occ_bits", C.c_void_p), ("bent", C.c_void_p), ("ao8", C.c_void_p)]


# the fields of srt_ao_frame_out: name -> (dtype, entries per pixel; None: (n_dirs + 31) // 32 words)
AO_FRAME_FIELDS = {"n_occluded": (np.uint32, 1), "ao": (np.float32, 1), "occ_bits": (np.uint32, None), "bent": (np.float32, 3), "ao8": (np.uint8, 1)}

class PointOut(C.Structure):
    """srt_point_out: the arrays a closest-point query fills, as addresses (host arrays in the host form, device pointers in the _device
    form); 0 = not wanted."""
    _fields_ = [("tri", C.c_void_p), ("dist2", C.c_void_p), ("point", C.c_void_p), ("vw", C.c_void_p), ("region", C.c_void_p)]


# the fields of srt_point_out: name -> (dtype, entries per point)
POINT_FIELDS = {"tri": (np.int32, 1), "dist2": (np.float32, 1), "point": (np.float32, 3), "vw": (np.float32, 2), "region": (np.uint8, 1)}

# the fields of srt_path_out: name -> (dtype, floats or ints per ray and segment)
PATH_FIELDS = {"hit_id": (np.int32, 1), "t": (np.float32, 1), "obj": (np.int32, 1), "rgb_linear": (np.float32, 3), "rays": (np.float32, 6)}

# the fields of srt_surface_out: name -> (dtype, floats or ints per ray)
SURFACE_FIELDS = {"obj": (np.int32, 1), "point": (np.float32, 3), "normal": (np.float32, 3), "color": (np.float32, 3), "material": (np.float32, 3),
                  "bounce": (np.float32, 6)}


# every struct of include/srt.h: its name there -> its class here
STRUCTS = {"srt_scene_desc": SceneDesc, "srt_params": Params, "srt_stats": Stats, "srt_frame_geometry": FrameGeometry, "srt_refit_desc": RefitDesc,
           "srt_surface_out": SurfaceOut, "srt_path_desc": PathDesc, "srt_path_out": PathOut, "srt_shadow_rule": ShadowRule, "srt_visibility": Visibility,
           "srt_refraction": Refraction, "srt_fresnel_out": FresnelOut, "srt_fresnel": Fresnel, "srt_ao_desc": AoDesc, "srt_ao_out": AoOut,
           "srt_ao_frame": AoFrame, "srt_ao_frame_out": AoFrameOut}
# every struct of include/srt_points.h
POINT_STRUCTS = {"srt_point_out": PointOut}


class Sign(C.Structure):
    """srt_sign: the direction table of a signed-distance query (an address: host memory in the host form, device memory in the _device
    form; 0 with n_dirs 0 = the default table) and the vote's flags."""
    _fields_ = [("dirs", C.c_void_p), ("n_dirs", C.c_uint32), ("flags", C.c_uint32)]


class SignOut(C.Structure):
    """srt_sign_out: the arrays a signed-distance query fills, as addresses; 0 = not wanted."""
    _fields_ = [("sdist", C.c_void_p), ("inside", C.c_void_p), ("winding", C.c_void_p), ("crossings", C.c_void_p)]


# the fields of srt_sign_out: name -> (dtype, entries per point; None: n_dirs)
SIGN_FIELDS = {"sdist": (np.float32, 1), "inside": (np.uint8, 1), "winding": (np.int32, None), "crossings": (np.uint32, None)}
# every struct of include/srt_signed.h
SIGNED_STRUCTS = {"srt_sign": Sign, "srt_sign_out": SignOut}


class PointMultiOut(C.Structure):
    """srt_point_multi_out: the arrays a k-nearest-triangles query fills, as addresses (host arrays in the host forms, device pointers in
    the _device forms); 0 = not wanted."""
    _fields_ = [("n_within", C.c_void_p), ("n_found", C.c_void_p), ("tri", C.c_void_p), ("dist2", C.c_void_p), ("point", C.c_void_p), ("vw", C.c_void_p),
                ("region", C.c_void_p)]


# the fields of srt_point_multi_out: name -> (dtype, entries per point and column; None: one entry per point, no columns)
POINT_MULTI_FIELDS = {"n_within": (np.uint32, None), "n_found": (np.uint32, None), "tri": (np.int32, 1), "dist2": (np.float32, 1), "point": (np.float32, 3),
                      "vw": (np.float32, 2), "region": (np.uint8, 1)}
# every struct of include/srt_points_multi.h
POINT_MULTI_STRUCTS = {"srt_point_multi_out": PointMultiOut}


class SegmentOut(C.Structure):
    """srt_segment_out: the arrays a segment query fills, as addresses (host arrays in the host form, device pointers in the _device
    form); 0 = not wanted."""
    _fields_ = [("tri", C.c_void_p), ("dist2", C.c_void_p), ("s", C.c_void_p), ("point", C.c_void_p), ("vw", C.c_void_p), ("feature", C.c_void_p)]


# the fields of srt_segment_out: name -> (dtype, entries per segment)
SEGMENT_FIELDS = {"tri": (np.int32, 1), "dist2": (np.float32, 1), "s": (np.float32, 1), "point": (np.float32, 3), "vw": (np.float32, 2), "feature": (np.uint8, 1)}
# every struct of include/srt_segments.h
SEGMENT_STRUCTS = {"srt_segment_out": SegmentOut}


# ---- the prototypes of include/srt.h, in its order: name -> (restype, [argtypes]) ----
# srt_scene*, void* and every address that travels as an int (the d_* parameters, a stream, srt_render_async's outputs) are c_void_p;
# srt_scene** and T* const* are POINTER(c_void_p); a pointer to an srt_ struct is POINTER(its class); a scalar is its exact ctype.
_int, _u32, _f32, _vp = C.c_int, C.c_uint32, C.c_float, C.c_void_p
_vpp, _f64p = C.POINTER(C.c_void_p), C.POINTER(C.c_double)
_desc, _geom, _refit, _par, _stats = C.POINTER(SceneDesc), C.POINTER(FrameGeometry), C.POINTER(RefitDesc), C.POINTER(Params), C.POINTER(Stats)
_surf, _path, _seg, _rule, _vis = C.POINTER(SurfaceOut), C.POINTER(PathDesc), C.POINTER(PathOut), C.POINTER(ShadowRule), C.POINTER(Visibility)
_refr, _fres = C.POINTER(Refraction), C.POINTER(Fresnel)
_ao, _aout, _afr, _afout = C.POINTER(AoDesc), C.POINTER(AoOut), C.POINTER(AoFrame), C.POINTER(AoFrameOut)

PROTOTYPES = {
    "srt_params_default": (None, [_par, _u32, _u32]),
    "srt_light_staircase": (None, [_f32p, _u32, _f32p]),
    "srt_rows_owned": (_u32, [_par]),
    "srt_cols_owned": (_u32, [_par]),
    "srt_scene_create": (_int, [_int, _desc, _vpp]),
    "srt_scene_destroy": (_int, [_vp]),
    "srt_scene_share": (_int, [_vp, _vpp]),
    "srt_scene_update": (_int, [_vp, _desc, _vp]),
    "srt_scene_set_source": (_int, [_vp, _f32p, _f32p, _i32p]),
    "srt_scene_update_frame": (_int, [_vp, _geom, _vp]),
    "srt_scene_set_pose_source": (_int, [_vp, _f32p]),
    "srt_scene_pose": (_int, [_vp, _u32, _f32p, _f32p, _f32p, _vp]),
    "srt_scene_refit_prepare": (_int, [_vp, _u32, _u32p]),
    "srt_scene_refit_device": (_int, [_vp, _refit, _vp]),
    "srt_render_device": (_int, [_vp, _par, _vp, _vp, _vp, _vp, _vp]),
    "srt_render_device_batch": (_int, [_u32, _vpp, _par, _vp, _vpp, _vpp, _vpp, _vpp]),
    "srt_render": (_int, [_vp, _par, _i32p, _f32p, _f32p, _u8p, _stats]),
    "srt_render_async": (_int, [_vp, _par, _vp, _vp, _vp, _vp]),
    "srt_host_alloc": (_vp, [C.c_size_t]),
    "srt_host_free": (None, [_vp]),
    "srt_sync": (_int, [_vp, _stats]),
    "srt_trace_rays_device": (_int, [_vp, _u32, _vp, _u32, _vp, _vp, _vp, _vp]),
    "srt_trace_rays": (_int, [_vp, _u32, _f32p, _u32, _i32p, _f32p, _f32p, _stats]),
    "srt_occluded_device": (_int, [_vp, _u32, _vp, _vp, _vp, _vp]),
    "srt_occluded": (_int, [_vp, _u32, _f32p, _i32p, _u8p]),
    "srt_trace_rays_range_device": (_int, [_vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "srt_trace_rays_range": (_int, [_vp, _u32, _f32p, _f32p, _u32, _i32p, _f32p, _f32p, _stats]),
    "srt_occluded_range_device": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "srt_occluded_range": (_int, [_vp, _u32, _f32p, _f32p, _i32p, _u8p]),
    "srt_trace_rays_multi_device": (_int, [_vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "srt_trace_rays_multi": (_int, [_vp, _u32, _f32p, _f32p, _u32, _u32, _u32p, _i32p, _f32p, _f32p, _stats]),
    "srt_shade_rays_device": (_int, [_vp, _u32, _vp, _par, _vp, _vp, _vp, _vp, _vp]),
    "srt_shade_rays": (_int, [_vp, _u32, _f32p, _par, _i32p, _f32p, _f32p, _u8p, _stats]),
    "srt_shade_rays_range_device": (_int, [_vp, _u32, _vp, _vp, _par, _vp, _vp, _vp, _vp, _vp]),
    "srt_shade_rays_range": (_int, [_vp, _u32, _f32p, _f32p, _par, _i32p, _f32p, _f32p, _u8p, _stats]),
    "srt_surface_rays_device": (_int, [_vp, _u32, _vp, _vp, _u32, _vp, _vp, _vp, _surf]),
    "srt_surface_rays": (_int, [_vp, _u32, _f32p, _f32p, _u32, _i32p, _f32p, _surf, _stats]),
    "srt_surface_hits_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _surf]),
    "srt_surface_hits": (_int, [_vp, _u32, _f32p, _i32p, _f32p, _u32, _surf]),
    "srt_shade_paths_device": (_int, [_vp, _u32, _vp, _vp, _par, _path, _vp, _vp, _vp, _seg]),
    "srt_shade_paths": (_int, [_vp, _u32, _f32p, _f32p, _par, _path, _f32p, _u8p, _seg, _stats]),
    "srt_render_paths_device": (_int, [_vp, _par, _path, _vp, _vp, _vp, _seg]),
    "srt_render_paths": (_int, [_vp, _par, _path, _f32p, _u8p, _seg, _stats]),
}


def _path_family(form, base, after, new):
    """The four srt_{shade,render}_paths<form>{_device,} calls: those of the form `base` with one argument more, of type `new`, right
    after their argument of type `after` (the header: "the same, plus ...")."""
    for stem in ("srt_shade_paths", "srt_render_paths"):
        for suffix in ("_device", ""):
            restype, args = PROTOTYPES[stem + base + suffix]
            at = args.index(after) + 1
            PROTOTYPES[stem + form + suffix] = (restype, args[:at] + [new] + args[at:])


_path_family("_shadow", "", after=_path, new=_rule)         # ..., const srt_path_desc* path, const srt_shadow_rule* shadow, ...
PROTOTYPES.update({
    "srt_scene_set_object_masks": (_int, [_vp, _u32, _u32p, _vp]),
    "srt_trace_rays_masked_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "srt_trace_rays_masked": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _u32, _i32p, _f32p, _f32p, _stats]),
    "srt_occluded_masked_device": (_int, [_vp, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "srt_occluded_masked": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _i32p, _u8p]),
})
_path_family("_masked", "_shadow", after=_rule, new=_vis)   # ..., const srt_shadow_rule* shadow, const srt_visibility* vis, ...
_path_family("_refract", "_masked", after=_vis, new=_refr)  # ..., const srt_visibility* vis, const srt_refraction* refr, ...
_path_family("_fresnel", "_refract", after=_refr, new=_fres)  # ..., const srt_refraction* refr, const srt_fresnel* fres, ...
PROTOTYPES.update({
    "srt_ao_rays_device": (_int, [_vp, _u32, _vp, _vp, _u32, _ao, _vis, _vp, _vp, _vp, _aout]),
    "srt_ao_rays": (_int, [_vp, _u32, _f32p, _f32p, _u32, _ao, _vis, _i32p, _f32p, _aout, _stats]),
    "srt_ao_hits_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _ao, _vis, _vp, _aout]),
    "srt_ao_hits": (_int, [_vp, _u32, _f32p, _i32p, _f32p, _u32, _ao, _vis, _aout, _stats]),
    "srt_render_ao_device": (_int, [_vp, _par, _u32, _ao, _afr, _vis, _vp, _vp, _vp, _afout]),
    "srt_render_ao": (_int, [_vp, _par, _u32, _ao, _afr, _vis, _i32p, _f32p, _afout, _stats]),
    "srt_render_ao_hits_device": (_int, [_vp, _par, _vp, _vp, _u32, _ao, _afr, _vis, _vp, _afout]),
    "srt_render_ao_hits": (_int, [_vp, _par, _i32p, _f32p, _u32, _ao, _afr, _vis, _afout, _stats]),
    "srt_scene_device_bytes": (C.c_uint64, [_vp]),
    "srt_scene_pipeline": (C.c_char_p, [_vp]),
    "srt_scene_overlap_estimate": (C.c_double, [_vp]),
    "srt_kat_ray_aabb": (_int, [_int, _u32, _f32p, _f32p, _u8p, _u8p, _u8p, _u8p]),
    "srt_kat_ray_triangle": (_int, [_int, _u32, _f32p, _f32p, _f32p]),
    "srt_kat_ray_triangle_origin": (_int, [_int, _u32, _f32p, _f32p, _f32p]),
    "srt_kat_barycentric": (_int, [_int, _u32, _f32p, _f32p]),
    "srt_kat_phong": (_int, [_int, _u32, _f32p, _f32p]),
    "srt_kat_interp_normal": (_int, [_int, _u32, _f32p, _f32p]),
    "srt_kat_pow": (_int, [_int, _u32, _f32p, _f32p, _f32p, _f32p]),
    "srt_kat_tonemap": (_int, [_int, _u32, _f32p, _f32, _f32, _f32p, _i32p]),
    "srt_kat_tone_filter": (_int, [_int, _u32, _f32p, _f32, _f32, _i32p, _i32p, _u8p]),
    "srt_kat_tone_filter_sweep": (_int, [_int, _u32, _u32, _f32, _f32, _f64p]),
    "srt_debug_valu_rate": (_int, [_int, _u32, _f64p]),
    "srt_debug_scene_records": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32p, _f32p, _i32p]),
    "srt_debug_fail_host_allocs": (None, [_int]),
    "srt_strerror": (C.c_char_p, [_int]),
    "srt_last_hip_error": (_int, []),
    "srt_abi_version": (_u32, []),
})

# ---- the prototypes of include/srt_points.h, in its order, under the same rules ----
_pout = C.POINTER(PointOut)
POINT_PROTOTYPES = {
    "srt_closest_points_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _pout]),
    "srt_closest_points": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _u32, _pout, _stats]),
}

# ---- the prototypes of include/srt_nearest.h, in its order, under the same rules; SRT_NEAREST_K is the header's margin constant ----
NEAREST_K = 64      # SRT_NEAREST_K
NEAREST_PROTOTYPES = {
    "srt_nearest_points_device": POINT_PROTOTYPES["srt_closest_points_device"],
    "srt_nearest_points": POINT_PROTOTYPES["srt_closest_points"],
}

# ---- include/srt_signed.h: its constants, its default table (SRT_SIGN_DEFAULT_DIRS, float literals) and its prototypes, in its order ----
SIGN_MAX_DIRS = 16      # SRT_SIGN_MAX_DIRS
SIGN_PARITY = 1         # SRT_SIGN_PARITY
SIGN_DEFAULT_DIRS = np.array([[0.57, 0.31, 0.76], [-0.43, 0.81, -0.39], [0.29, -0.66, -0.69]], np.float32)
_sign, _sout = C.POINTER(Sign), C.POINTER(SignOut)
SIGNED_PROTOTYPES = {
    "srt_signed_points_device": (_int, [_vp, _u32, _vp, _vp, _vp, _sign, _u32, _vp, _pout, _sout]),
    "srt_signed_points": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _sign, _u32, _pout, _sout, _stats]),
}

# ---- include/srt_points_multi.h: its constant and its prototypes, in its order, under the same rules ----
POINT_MULTI_MAX = 16      # SRT_POINT_MULTI_MAX
_pmout = C.POINTER(PointMultiOut)
POINT_MULTI_PROTOTYPES = {
    "srt_closest_points_multi_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _u32, _vp, _pmout]),
    "srt_closest_points_multi": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _u32, _u32, _pmout, _stats]),
}
POINT_MULTI_PROTOTYPES.update({
    "srt_nearest_points_multi_device": POINT_MULTI_PROTOTYPES["srt_closest_points_multi_device"],
    "srt_nearest_points_multi": POINT_MULTI_PROTOTYPES["srt_closest_points_multi"],
})

# ---- include/srt_segments.h: its prototypes, in its order, under the same rules ----
_sgout = C.POINTER(SegmentOut)
SEGMENT_PROTOTYPES = {
    "srt_closest_segments_device": (_int, [_vp, _u32, _vp, _vp, _vp, _u32, _vp, _sgout]),
    "srt_closest_segments": (_int, [_vp, _u32, _f32p, _f32p, _u32p, _u32, _sgout, _stats]),
}


def _ptr(a, ty):
    return a.ctypes.data_as(ty) if a is not None else ty()


@dataclass
class FlatScene:
    """Host-side flat scene (numpy, C-contiguous).  Field names follow include/srt.h."""
    node_min: np.ndarray
    node_max: np.ndarray
    node_left: np.ndarray
    node_right: np.ndarray
    node_first: np.ndarray
    node_count: np.ndarray
    obj_root: np.ndarray
    tri_points: np.ndarray
    tri_obj: np.ndarray
    obj_color: np.ndarray
    obj_material: np.ndarray
    tri_tex: np.ndarray | None = None
    tri_texcoord: np.ndarray | None = None
    tri_normals: np.ndarray | None = None
    tex_rgb: np.ndarray | None = None
    tex_off: np.ndarray | None = None
    tex_w: np.ndarray | None = None
    tex_h: np.ndarray | None = None
    names: list = field(default_factory=list)

    _SPEC = {
        "node_min": np.float32, "node_max": np.float32,
        "node_left": np.int32, "node_right": np.int32, "node_first": np.int32, "node_count": np.int32,
        "obj_root": np.uint32, "tri_points": np.float32, "tri_obj": np.int32,
        "obj_color": np.float32, "obj_material": np.float32,
        "tri_tex": np.int32, "tri_texcoord": np.float32, "tri_normals": np.float32,
        "tex_rgb": np.uint8, "tex_off": np.uint64, "tex_w": np.uint32, "tex_h": np.uint32,
    }

    def __post_init__(self):
        for k, dt in self._SPEC.items():
            v = getattr(self, k)
            if v is not None:
                setattr(self, k, np.ascontiguousarray(v, dtype=dt))
        if self.tri_tex is None:
            self.tri_tex = np.full(self.n_tris, -1, np.int32)

    @property
    def n_objects(self):
        return int(self.obj_root.shape[0])

    @property
    def n_nodes(self):
        return int(self.node_left.shape[0])

    @property
    def n_tris(self):
        return int(self.tri_obj.shape[0])

    @property
    def n_textures(self):
        return 0 if self.tex_w is None else int(self.tex_w.shape[0])

    def desc(self) -> SceneDesc:
        """ctypes descriptor pointing into this object's arrays (keep `self` alive while in use)."""
        d = SceneDesc()
        d.n_objects, d.n_nodes, d.n_tris, d.n_textures = self.n_objects, self.n_nodes, self.n_tris, self.n_textures
        d.node_min, d.node_max = _ptr(self.node_min, _f32p), _ptr(self.node_max, _f32p)
        d.node_left, d.node_right = _ptr(self.node_left, _i32p), _ptr(self.node_right, _i32p)
        d.node_first, d.node_count = _ptr(self.node_first, _i32p), _ptr(self.node_count, _i32p)
        d.obj_root = _ptr(self.obj_root, _u32p)
        d.tri_points = _ptr(self.tri_points, _f32p)
        d.tri_obj, d.tri_tex = _ptr(self.tri_obj, _i32p), _ptr(self.tri_tex, _i32p)
        d.tri_texcoord, d.tri_normals = _ptr(self.tri_texcoord, _f32p), _ptr(self.tri_normals, _f32p)
        d.obj_color, d.obj_material = _ptr(self.obj_color, _f32p), _ptr(self.obj_material, _f32p)
        d.tex_rgb, d.tex_off = _ptr(self.tex_rgb, _u8p), _ptr(self.tex_off, _u64p)
        d.tex_w, d.tex_h = _ptr(self.tex_w, _u32p), _ptr(self.tex_h, _u32p)
        return d

    ARRAYS = tuple(_SPEC.keys())

    def to_npz_dict(self, prefix="scene_"):
        out = {prefix + k: getattr(self, k) for k in self.ARRAYS if getattr(self, k) is not None}
        out[prefix + "names"] = np.array(self.names, dtype="U")
        return out

    @classmethod
    def from_npz_dict(cls, z, prefix="scene_"):
        kw = {k: z[prefix + k] for k in cls.ARRAYS if (prefix + k) in z}
        names = [str(s) for s in z[prefix + "names"]] if (prefix + "names") in z else []
        return cls(names=names, **kw)


REFERENCE_BACKGROUND = (173, 216, 230)   # drawImage, simple_raytracer.cpp:476


def light_staircase(base, n):
    """softShadow's light table (simple_raytracer.cpp:363-383), accumulated in f32 like the reference.
    Pure data preparation for srt_params.light_pos (the C ABI's srt_light_staircase does the same)."""
    out = np.zeros((n, 3), np.float32)
    L = np.array(base[:3], np.float32)
    for i in range(n):
        out[i] = L
        L[i % 3] = np.float32(L[i % 3] + np.float32(3.0))
    return out


def make_params(width, height, lights, *, block_rows=None, block_first=0, block_stride=1, block_cols=0,
                focal=400.0, shadow_div=5.0, reinhard=0.5, gamma=1.1, background=REFERENCE_BACKGROUND,
                spp=1, flags=0, ray_matrix=None):
    """srt_params with the reference's literals; `lights` is an (n,3) f32 array kept alive on the
    returned object (attribute _lights)."""
    p = Params()
    p.width, p.height = int(width), int(height)
    p.block_rows = int(block_rows if block_rows else height)
    p.block_first, p.block_stride, p.block_cols = int(block_first), int(block_stride), int(block_cols)
    p.focal = focal
    lights = np.ascontiguousarray(np.asarray(lights, np.float32).reshape(-1, 3))
    p.n_lights = lights.shape[0]
    p.light_pos = _ptr(lights, _f32p)
    p._lights = lights
    p.shadow_div, p.reinhard, p.gamma = shadow_div, reinhard, gamma
    p.background[0], p.background[1], p.background[2], p.background[3] = background[0], background[1], background[2], 0
    p.spp, p.flags = spp, flags
    if ray_matrix is not None:      # camera mode (extension): 16 floats, column-major
        m = np.ascontiguousarray(np.asarray(ray_matrix, np.float32).reshape(16))
        p.ray_matrix = _ptr(m, _f32p)
        p._ray_matrix = m
    return p


def owned_pixels(width, height, block_rows, block_first, block_stride, block_cols=0):
    """Image pixel (flat index y * width + x) of every local output pixel of a call with these block params, as an int64 array
    [rows_local, cols_local]; -1 = padding.  Mirrors include/srt.h (srt_params.block_rows / block_cols)."""
    if not block_cols:
        ys = rows_owned(height, block_rows, block_first, block_stride)
        return ys[:, None] * width + np.arange(width, dtype=np.int64)[None, :]
    n_bx = (width + block_cols - 1) // block_cols
    wl = (n_bx + block_stride - 1) // block_stride * block_cols
    y = np.arange(height, dtype=np.int64)[:, None]
    xl = np.arange(wl, dtype=np.int64)[None, :]
    off = (block_first + block_stride - (y // block_rows) % block_stride) % block_stride
    x = ((xl // block_cols) * block_stride + off) * block_cols + xl % block_cols
    return np.where(x < width, y * width + x, -1)


def rows_owned(height, block_rows, block_first, block_stride):
    """Image rows (ascending, in local-row order) a call with these block params writes."""
    ys = []
    nblocks = (height + block_rows - 1) // block_rows
    for b in range(block_first, nblocks, block_stride):
        ys.extend(range(b * block_rows, min((b + 1) * block_rows, height)))
    return np.array(ys, np.int64)
