#!/usr/bin/env python3
"""A mirror floor from a ray query: render the K3 scene (bunny on its ground slab) in camera mode, build with numpy one reflected ray per
ground pixel from the caller's own triangle points, ask srt_shade_rays_range what colour comes back along each, mix the linear colours
and tone-map.  A reflected ray starts AT the hit point -- the origin is not moved, so the shadow origin o + d * t and Phong's view vector
are those of the true ray -- and its interval (T_MIN, +inf) keeps it off the slab it starts on.  The library has no recursion; the
caller composes it from this call.
Usage: python examples/mirror.py [out.bmp [width height [reflectance]]]     (needs a GPU)"""
import os, struct, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import abi, lib      # noqa: E402
import golden_util as gu                       # noqa: E402

GROUND = 0            # object 0 of the scene is the slab (cube.obj), object 1 the bunny
N_LIGHTS = 4
T_MIN = 1e-4          # in units of the reflected direction (as long as the primary one: (i, j, focal), some hundreds): about 1e-2 off the slab


def display_tone(lin, reinhard=0.5, gamma=1.1):
    """DISPLAY ONLY: the arithmetic of tests/tonemap_ref.py (tone_ref, quant_ref), copied -- c / (c + r) in float32, the power in
    float64 rounded once, int(c * 255) clamped.  The library's own tone map runs on the device; this one only shows the mixed colours."""
    c = np.asarray(lin, np.float32)
    with np.errstate(all="ignore"):
        ratio = c / (c + np.float32(reinhard))
        tone = np.power(ratio.astype(np.float64), np.float64(np.float32(gamma))).astype(np.float32)
        s = tone * np.float32(255.0)
        q = np.where(s > 0, s, 0).astype(np.float64)
    return np.floor(np.minimum(q, 255.0)).astype(np.uint8)


def write_bmp(path, rgb):
    """24-bit BMP, rows bottom-up, BGR, each row padded to 4 bytes."""
    h, w, _ = rgb.shape
    row = np.zeros((h, (w * 3 + 3) // 4 * 4), np.uint8)
    row[:, :w * 3] = rgb[::-1, :, ::-1].reshape(h, w * 3)
    with open(path, "wb") as f:
        f.write(b"BM" + struct.pack("<IHHI", 54 + row.size, 0, 0, 54))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, row.size, 2835, 2835, 0, 0))
        f.write(row.tobytes())


def main():
    a = sys.argv[1:]
    out = a[0] if a else "mirror.bmp"
    W, H = (int(a[1]), int(a[2])) if len(a) >= 3 else (640, 360)
    k = np.float32(a[3]) if len(a) >= 4 else np.float32(0.6)
    focal = np.float32(400.0 * W / 1920.0)
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    ds = lib.DeviceScene(flat)
    lights = abi.light_staircase(g.light, N_LIGHTS)
    # the frame, in camera mode with the identity matrix: rays leave the origin with direction (i, j, focal)
    eye = np.eye(4, dtype=np.float32).reshape(-1)
    frame = ds.render(abi.make_params(W, H, lights, focal=float(focal), ray_matrix=eye))
    hit, t, lin = frame["hit_id"].reshape(-1), frame["t"].reshape(-1), frame["rgb_linear"].reshape(-1, 3).copy()
    d = np.empty((H, W, 3), np.float32)
    d[..., 0] = (int(-W / 2) + np.arange(W)).astype(np.float32)[None, :]
    d[..., 1] = (int(-H / 2) + np.arange(H)).astype(np.float32)[:, None]
    d[..., 2] = focal
    d = d.reshape(-1, 3)
    ground = np.flatnonzero((hit >= 0) & (flat.tri_obj[np.maximum(hit, 0)] == GROUND))
    # one reflected ray per ground pixel, from the caller's own copy of the triangle points: r = d - 2 (d . n) n
    P = np.ascontiguousarray(flat.tri_points, np.float32).reshape(-1, 3, 4)[hit[ground]]
    p1, p2, p3 = (P[:, i, :3] / P[:, i, 3:4] for i in range(3))
    n = np.cross(p2 - p1, p3 - p1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    dg = d[ground]
    n = np.where(np.sum(n * dg, axis=1, keepdims=True) > 0, -n, n)                 # the side the ray arrives on
    point = dg * t[ground, None]
    r = dg - 2.0 * np.sum(dg * n, axis=1, keepdims=True) * n
    rays = np.ascontiguousarray(np.concatenate([point, r], axis=1), np.float32)      # from the hit point itself
    t_range = np.tile(np.float32([T_MIN, np.inf]), (rays.shape[0], 1))
    p = abi.make_params(1, 1, lights)                      # lights, literals, flags: the frame fields are ignored
    back = ds.shade_rays(rays, p, want=("hit_id", "rgb_linear"), t_range=t_range)
    seen = back["hit_id"] >= 0
    lin[ground[seen]] = (np.float32(1.0) - k) * lin[ground[seen]] + k * back["rgb_linear"][seen]
    rgb8 = display_tone(lin)
    rgb8[hit < 0] = np.array(abi.REFERENCE_BACKGROUND, np.uint8)
    write_bmp(out, rgb8.reshape(H, W, 3))
    print(f"{out}: {W}x{H}, {ground.size} ground pixels reflected, {int(seen.sum())} of them see the scene "
          f"({back['stats']['shadow_rays']} shadow rays), frame pipeline {ds.pipeline}")
    ds.close()


if __name__ == "__main__":
    main()
