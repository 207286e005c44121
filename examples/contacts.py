#!/usr/bin/env python3
"""ALL contacts of a cloud of particles with the K3 scene (bunny on its ground slab), on torch device tensors: what a collision solver asks
before it resolves a step.  Particles are scattered in a shell around the bunny's surface; srt_closest_points_multi_device gives, in one
launch, every triangle within the particle's THICKNESS -- up to K of them, nearest first, with the contact point on each -- and n_within,
the full count, which tells a particle in a fold (more contacts than K) from one on a face.  The contact normals are made on the device
from the contact points; nothing but the summary comes back to the host.  For comparison the same particles go through
srt_nearest_points_multi_device without a radius: the K nearest faces of every particle, whatever their distance (include/srt_points_multi.h).
Usage: python examples/contacts.py [particles [thickness]]     (needs a GPU)"""
import os, sys
import numpy as np
import torch                                   # first: torch initialises HIP before the library does

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402

K = 8


def main():
    a = sys.argv[1:]
    n = int(a[0]) if a else 100000
    thickness = float(a[1]) if len(a) > 1 else 1.5
    dev = torch.device("cuda", 0); torch.zeros(1, device=dev)
    flat = gu.GoldenScene("ground_bunny").flat
    ds = lib.DeviceScene(flat)
    bunny = np.ascontiguousarray(flat.tri_points, np.float32)[flat.tri_obj == 1][..., :3]
    d_verts = torch.from_numpy(bunny.reshape(-1, 3).copy()).to(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        g = torch.Generator(device=dev); g.manual_seed(7)
        # particles: a vertex of the bunny, pushed up to three thicknesses away in a random direction
        pick = torch.randint(0, d_verts.shape[0], (n,), device=dev, generator=g)
        push = torch.randn((n, 3), device=dev, generator=g)
        push = push / push.norm(dim=1, keepdim=True) * (3.0 * thickness * torch.rand((n, 1), device=dev, generator=g))
        pts = (d_verts[pick] + push).contiguous()
        rad = torch.full((n,), thickness, dtype=torch.float32, device=dev)
        n_within, n_found = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        tri, d2 = torch.empty((n, K), dtype=torch.int32, device=dev), torch.empty((n, K), dtype=torch.float32, device=dev)
        point = torch.empty((n, K, 3), dtype=torch.float32, device=dev)
        ds.closest_points_multi_device(n, pts.data_ptr(), K, radius=rad.data_ptr(), stream=side.cuda_stream, n_within=n_within.data_ptr(), n_found=n_found.data_ptr(),
                                       tri=tri.data_ptr(), dist2=d2.data_ptr(), point=point.data_ptr())
        # per contact: the direction to push the particle along and how deep it is inside the thickness (empty columns: depth 0)
        filled = tri >= 0
        away = pts[:, None, :] - point
        depth = torch.where(filled, thickness - torch.sqrt(torch.where(filled, d2, torch.zeros_like(d2))), torch.zeros_like(d2))
        normal = away / away.norm(dim=2, keepdim=True).clamp(min=1e-20)
        correction = (normal * depth[..., None]).sum(1)                         # one Jacobi step of a position-based solver
        # the K nearest faces without a radius, for the same particles
        ntri, nd2 = torch.empty((n, K), dtype=torch.int32, device=dev), torch.empty((n, K), dtype=torch.float32, device=dev)
        ds.nearest_points_multi_device(n, pts.data_ptr(), K, stream=side.cuda_stream, tri=ntri.data_ptr(), dist2=nd2.data_ptr())
    side.synchronize()
    touching = n_found > 0
    assert bool((filled.sum(1) == n_found).all()) and bool((n_found == n_within.clamp(max=K)).all())
    assert bool((d2[filled] <= thickness * thickness).all()) and bool((d2[:, 1:] >= d2[:, :-1]).all())
    assert bool((ntri >= 0).all()) and bool((nd2[:, 1:] >= nd2[:, :-1]).all())
    # within the thickness the two calls agree on every filled column
    assert bool((ntri[filled] == tri[filled]).all()) and bool((nd2[filled] == d2[filled]).all())
    hist = torch.bincount(n_found.long(), minlength=K + 1).cpu().numpy()
    print(f"{n} particles around the bunny, thickness {thickness}: {int(touching.sum())} touch the scene, {int(n_found.sum())} contacts reported "
          f"({int(n_within.long().sum())} within the thickness; {int((n_within > K).sum())} particles have more than {K}); particles by contacts 0..{K}: {hist.tolist()}; "
          f"largest correction {float(correction.norm(dim=1).max()):.3f}; without a radius the {K}-th nearest face lies {float(torch.sqrt(nd2[:, K - 1]).median()):.2f} away (median)")
    ds.close()


if __name__ == "__main__":
    main()
