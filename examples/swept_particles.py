#!/usr/bin/env python3
"""Particles that step THROUGH the bunny's ear, on torch device tensors: continuous collision for a step that is longer than the sheet is
thick.  Every particle starts a few units in front of a triangle of the ear and ends a few units behind it.  What a solver could ask
before: srt_closest_points_device at the END position with the particle's thickness -- the ear is behind the particle by then, and the
query finds nothing -- or a ray from A to B, which misses a near miss.  srt_closest_segments_device (include/srt_segments.h) takes the
step itself, a capsule of the particle's thickness: it finds the triangle the step crosses, the parameter s of the contact along the step
and the contact point, in one launch; the particles are then put back to where they touched.  A second batch passes BESIDE the ear, closer
than the thickness, without crossing anything: the segment query reports those too, with their distance.
Usage: python examples/swept_particles.py [particles [thickness [step]]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402


def main():
    a = sys.argv[1:]
    n = int(a[0]) if a else 100000
    thickness = float(a[1]) if len(a) > 1 else 0.25
    step = float(a[2]) if len(a) > 2 else 8.0
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    flat = gu.GoldenScene("ground_bunny").flat
    ds = lib.DeviceScene(flat)
    P = np.ascontiguousarray(flat.tri_points, np.float32)[..., :3]
    bunny, ground = P[flat.tri_obj == 1], P[flat.tri_obj == 0]
    # "up" is the axis along which the bunny stands off its slab; the ear: the triangles in the top eighth of the bunny along it
    off = bunny.reshape(-1, 3).mean(0) - ground.reshape(-1, 3).mean(0)
    axis = int(np.argmax(np.abs(off))); sign = float(np.sign(off[axis]))
    height = sign * bunny[..., axis].mean(1)
    ear = bunny[height >= height.min() + 0.875 * (height.max() - height.min())]
    nrm = np.cross(ear[:, 1] - ear[:, 0], ear[:, 2] - ear[:, 0])
    keep = np.linalg.norm(nrm, axis=1) > 0
    ear, nrm = ear[keep], nrm[keep] / np.linalg.norm(nrm[keep], axis=1, keepdims=True)
    d_c, d_n = torch.from_numpy(ear.mean(1).copy()).to(dev), torch.from_numpy(nrm.astype(np.float32)).to(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev); g.manual_seed(11)
        pick = torch.randint(0, d_c.shape[0], (n,), device=dev, generator=g)
        c, nn = d_c[pick], d_n[pick]
        # the first half steps through its triangle along the normal; the second half passes beside it, half a thickness off the surface
        through = torch.arange(n, device=dev) < n // 2
        tangent = torch.linalg.cross(nn, torch.roll(nn, 1, 1)); tangent = tangent / tangent.norm(dim=1, keepdim=True).clamp(min=1e-20)
        A = torch.where(through[:, None], c + nn * (0.5 * step), c + nn * (0.5 * thickness) - tangent * (0.5 * step))
        B = torch.where(through[:, None], c - nn * (0.5 * step), c + nn * (0.5 * thickness) + tangent * (0.5 * step))
        seg = torch.cat([A, B], 1).contiguous()
        rad = torch.full((n,), thickness, dtype=torch.float32, device=dev)
        # before: the point query at the end position
        end = B.contiguous()
        p_tri = torch.empty(n, dtype=torch.int32, device=dev)
        ds.closest_points_device(n, end.data_ptr(), radius=rad.data_ptr(), stream=side.cuda_stream, tri=p_tri.data_ptr())
        # the step itself
        tri, d2, s = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
        point, feature = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
        ds.closest_segments_device(n, seg.data_ptr(), radius=rad.data_ptr(), stream=side.cuda_stream, tri=tri.data_ptr(), dist2=d2.data_ptr(), s=s.data_ptr(),
                                   point=point.data_ptr(), feature=feature.data_ptr())
        found = tri >= 0
        contact = A + (B - A) * s[:, None]                                       # where on the step the particle touched, or came closest
        resolved = torch.where(found[:, None], contact, B)                      # (a solver would stop the particle there)
    side.synchronize()
    crossing = found & (feature == 5)
    assert bool((d2[crossing] == 0).all()) and bool((d2[found] <= thickness * thickness).all()) and bool(((s >= 0) & (s <= 1)).all())
    assert bool(found[through].all()), "a step along the normal through its own triangle's centroid crosses it"
    missed = found & (p_tri < 0)
    print(f"{n} particles of thickness {thickness}, steps of {step} at the bunny's ear ({ear.shape[0]} triangles): the point query at the end position finds "
          f"{int((p_tri >= 0).sum())}; the segment query finds {int(found.sum())} -- {int(crossing.sum())} crossings (median s {float(s[crossing].median()):.3f}) and "
          f"{int((found & ~crossing).sum())} near misses (median distance {float(torch.sqrt(d2[found & ~crossing]).median()) if bool((found & ~crossing).any()) else float('nan'):.3f}); "
          f"{int(missed.sum())} contacts the point query at the end missed; the particles were moved back by up to {float((resolved - B).norm(dim=1).max()):.2f}")
    ds.close()


if __name__ == "__main__":
    main()
