#!/usr/bin/env python3
"""Through the bunny with srt_trace_rays_multi: a batch of parallel rays through the bunny-and-ground scene, ONE call with k = 8.  Per
ray the hits come back nearest first; hits of the bunny pair up as (entry, exit), and the summed exit - entry is the thickness of bunny
the ray passes through, in units of the direction (the directions here have length 1).  Printed beside it: how many calls the chain of
srt_trace_rays_range calls with t_min = next float after the last hit needs for the same rows -- one per hit and one more to find the
end -- and how many hits that chain would step over because they share their t with the hit before them.
Usage: python examples/xray.py [rays]     (needs a GPU)"""
import os, sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from simple_raytracer_amd import lib           # noqa: E402
import golden_util as gu                       # noqa: E402

K = 8


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 12
    g = gu.GoldenScene("ground_bunny")
    flat = g.flat
    bunny = int(np.argmax(np.bincount(flat.tri_obj)))            # the object with the most triangles
    P = flat.tri_points[flat.tri_obj == bunny].reshape(-1, 3, 4)[..., :3].reshape(-1, 3)
    lo, hi = P.min(0), P.max(0)
    # parallel rays along +z from in front of the bunny, on a diagonal across its silhouette
    f = (np.arange(n) + 0.5) / n
    o = np.stack([lo[0] + f * (hi[0] - lo[0]), lo[1] + f * (hi[1] - lo[1]), np.full(n, lo[2] - 0.5 * (hi[2] - lo[2]))], axis=1)
    rays = np.concatenate([o, np.tile([0.0, 0.0, 1.0], (n, 1))], axis=1).astype(np.float32)
    ds = lib.DeviceScene(flat)
    r = ds.trace_rays_multi(rays, K, want=("n_hits", "hit_id", "t"))
    print(f"{n} rays through {g.name} ({flat.n_tris} triangles), one srt_trace_rays_multi call, k = {K}")
    print(f"{'ray':>3s} {'hits':>4s} {'thickness':>10s} {'chain calls':>11s} {'lost to ties':>12s}   (entry, exit) pairs on the bunny")
    calls = 0
    for i in range(n):
        m = min(int(r["n_hits"][i]), K)
        ids, t = r["hit_id"][i, :m], r["t"][i, :m]
        on = flat.tri_obj[ids] == bunny
        tb = t[on]
        pairs = [(float(tb[j]), float(tb[j + 1])) for j in range(0, len(tb) - 1, 2)]
        thick = sum(b - a for a, b in pairs)
        tied = int((t[1:] == t[:-1]).sum())                      # next_up(t) steps over these
        chain = (m - tied) + (1 if m < K else 0)                 # one range call per hit it finds, one more that finds nothing
        calls = max(calls, chain)
        note = "" if int(r["n_hits"][i]) <= K else f"   ({int(r['n_hits'][i])} hits in all: the row holds the nearest {K})"
        print(f"{i:3d} {int(r['n_hits'][i]):4d} {thick:10.4f} {chain:11d} {tied:12d}   " + " ".join(f"({a:.3f}, {b:.3f})" for a, b in pairs) + note)
    print(f"the chain needs {calls} calls of srt_trace_rays_range for this batch (every call a full walk of all {n} rays and a host round trip); this was 1")


if __name__ == "__main__":
    main()
