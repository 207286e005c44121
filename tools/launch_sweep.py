#!/usr/bin/env python3
"""What the render dispatcher of srt_hip.hip picks, case by case (GPU box): small frames over scenes x kernel selectors x light samples x
flags x camera mode x spp, as single calls and as srt_render_device_batch calls of three handles, the third with a frame of another size.
Every case is rendered twice on its handles (the second frame of a handle takes the heavy-quadrant lists where the pipeline has them) and
gives one line: the case, the return codes of the two calls, srt_scene_pipeline of each handle.  Calls that the argument checks refuse are
cases like any other.  The plain listing is 128,000 lines (10 MB), more than a file in the repository may hold, so what is printed is
the listing folded (cases with one answer that differ in one factor share a line that lists the factor's values; the order of lines
is that of the first case of each) and the SHA-256 of the plain lines; --plain prints the plain lines instead.  One process; stops at the first HIP error.  The listing of a tree is its dispatch table; two trees
launch the same kernels if the listings are equal and one run of each under the kernel trace,
    timeout -k 10 900 rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 tools/launch_sweep.py > listing.txt
    python3 tools/launch_sweep.py --trace OUT
gives the same digest (--trace reduces a trace to its ordered (kernel, grid, workgroup) list and the launches per kernel).  Under the
trace on an MI355X a scene takes 30 s (ground_bunny) to 310 s (soup200k), all five 2.6 M launches in about 10 minutes; profiles/launch_sweep.txt
holds the listing and the trace digests of commit d2aa044, one run per scene.  Every render kernel of the code object occurs in it but
k_shade_tile_batch<0>: a held batch with a scene whose shininess is no integer in [1, 64], and every scene here has such values.
Usage: python tools/launch_sweep.py [--scenes cube_ground,soup20k] [--sizes 64x48,203x117] [--plain]"""
import argparse, collections, copy, csv, glob, hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

# estimates 3.7, 11.7, 17.4, 214 and 478; main_nocats with vertex normals is 36.9 MB of records (over 32 MiB: whole tile rows per XCD), the soups 3.3 and 31.7 MB
SCENES = ("cube_ground", "ground_bunny", "main_nocats", "soup20k", "soup200k")
# (31 and 67 -- the one-wave workgroups of the trace kernel over tile spans without the in-flight hint, and the two-wave workgroups in
# their place -- came after the listing of profiles/launch_sweep.txt: its digests are those of this tuple without them)
SELECTORS = (0, 1, 2, 3, 4, 5, 6, 9, 10, 11, 12, 13, 17, 18, 20, 21, 22, 23, 24, 25, 27, 28, 29, 31, 35, 40, 41, 42, 43, 44, 45, 46, 47,
             53, 54, 55, 56, 57, 58, 62, 67, 99)
LIGHTS = (0, 1, 7, 8, 15, 16, 63, 64)


def reduce_trace(d):
    """The kernel trace under d as its ordered (kernel, grid, workgroup) list: digest, length, launches per kernel."""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, f"one *kernel_trace.csv expected under {d}: {files}"
    rows = []
    with open(files[0], newline="") as f:
        for r in csv.DictReader(f):
            name = r["Kernel_Name"].replace("void ", "").split("(")[0]
            rows.append((int(r["Dispatch_Id"]), name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ")))
    rows.sort()
    h = hashlib.sha256()
    per = collections.Counter()
    for _, name, grid, wg in rows:
        h.update(f"{name} {grid} {wg}\n".encode())
        per[name] += 1
    print(f"launches {len(rows)} sha256 {h.hexdigest()}")
    for name in sorted(per):
        print(f"{per[name]:9d} {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default=",".join(SCENES)); ap.add_argument("--sizes", default="64x48,203x117"); ap.add_argument("--trace"); ap.add_argument("--plain", action="store_true")
    a = ap.parse_args()
    if a.trace:
        return reduce_trace(a.trace)
    import numpy as np
    from simple_raytracer_amd import abi, build, host, lib
    import golden_util as gu
    import scenes as sc
    sizes = [tuple(int(x) for x in s.split("x")) for s in a.sizes.split(",")]
    modes = (("plain", 0), ("count", abi.SRT_FLAG_COUNT_WORK), ("in-flight", abi.SRT_FLAG_FRAMES_IN_FLIGHT), ("no-timing", abi.SRT_FLAG_NO_TIMING),
             ("smooth", abi.SRT_FLAG_SMOOTH_NORMALS))
    cam = np.array([np.cos(0.07), 0, -np.sin(0.07), 0, 0, 1, 0, 0, np.sin(0.07), 0, np.cos(0.07), 0, 3.0, -2.0, 10.0, 1.0], np.float32)      # a yaw and an origin

    def with_normals(flat):
        f = copy.copy(flat)
        P = f.tri_points[..., :3]
        nrm = P - P.reshape(-1, 3).mean(0)
        f.tri_normals = np.ascontiguousarray((nrm / np.maximum(np.linalg.norm(nrm, axis=2, keepdims=True), 1e-6)).reshape(-1, 9), np.float32)
        return f

    def call(f):
        try:
            f()
            return 0
        except lib.SrtError as e:
            if e.code == abi.SRT_ERR_DEVICE:
                print(f"HIP error: {e}", flush=True)
                sys.exit(1)
            return e.code

    def result(rc, handles):      # a refused call launches nothing and leaves the text of the handle's previous render
        return f"rc {rc[0]} {rc[1]} " + (" | ".join(d.pipeline for d in handles) if rc[1] == 0 else "-")

    def fold(rows):
        """Cases that differ in one factor only and gave the same answer become one line that lists that factor's values; factor after
        factor, innermost first.  Every line stands for the product of its lists, so the folded listing says what the plain one says."""
        rows = [(tuple((x,) for x in c), r) for c, r in rows]
        for axis in (5, 4, 6, 3, 2, 0, 1):
            merged = {}
            for c, r in rows:
                merged.setdefault((c[:axis], c[axis + 1:], r), []).extend(c[axis])
            rows = [(a + (tuple(v),) + b, r) for (a, b, r), v in merged.items()]
        return [(tuple(",".join(x) for x in c), r) for c, r in rows]

    digest = hashlib.sha256()
    for name in a.scenes.split(","):
        if name.startswith("soup"):
            build.build_host()
            recipe, meshes = sc.soup(int(name[4:-1]) * 1000)
            flat, light = with_normals(host.build_flat_scene(recipe, meshes)), np.array(recipe.light[:3], np.float32)
        else:
            g = gu.GoldenScene(name)
            flat, light = (g.flat if name == "cube_ground" else with_normals(g.flat)), g.light      # cube_ground: a scene without vertex normals
        ds = [lib.DeviceScene(flat)]
        ds += [ds[0].share(), ds[0].share()]
        print(f"# {name}: device_bytes {ds[0].device_bytes} overlap estimate {ds[0].overlap_estimate:.3f}", flush=True)
        lights = {L: abi.light_staircase(light, L) for L in LIGHTS}
        rows = []
        for (W, H), (W2, H2) in zip(sizes, sizes[1:] + sizes[:1]):
            for v in SELECTORS:
                for L in LIGHTS:
                    for mode, flags in modes:
                        for camera in (0, 1):
                            for spp in (1, 4):
                                kw = dict(flags=flags | (v << 8), spp=spp, ray_matrix=cam if camera else None)
                                case = (f"{W}x{H}", f"v{v}", f"L{L}", mode, f"cam{camera}", f"spp{spp}")
                                p = abi.make_params(W, H, lights[L], **kw)
                                rc = [call(lambda: ds[0].render_device(p)) for _ in range(2)]
                                call(ds[0].sync)
                                rows.append((case + ("single",), result(rc, ds[:1])))
                                fb = lib.FrameBatch(ds, [p, p, abi.make_params(W2, H2, lights[L], **kw)])
                                rc = [call(fb.render) for _ in range(2)]
                                for d in ds:
                                    call(d.sync)
                                rows.append((case + ("batch",), result(rc, ds)))
                print(f"{name} {W}x{H} v{v}", file=sys.stderr, flush=True)
        digest.update("".join(f"{name} {' '.join(c)}: {r}\n" for c, r in rows).encode())
        for c, r in (rows if a.plain else fold(rows)):
            print(f"{name} {' '.join(c)}: {r}")
        sys.stdout.flush()
        for d in ds:
            d.close()
    print(f"# sha256 of the plain listing (one line per case): {digest.hexdigest()}")


if __name__ == "__main__":
    main()
