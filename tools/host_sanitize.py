"""The loaders, the hierarchy builder and the flattener of the host mirror under AddressSanitizer and UBSan, on a machine without a GPU.

    python tools/host_sanitize.py [--jpeg N] [--image N] [--obj N] [--keep DIR]

Builds tools/host_sanitize_main.cpp with srt_host.cpp and srt_jpeg.cpp (g++ -fsanitize=address,undefined, no libsrt_hip: that half of
the mirror needs none), writes corrupt copies of small files into a temporary directory -- N mutants of each JPEG of
tests/golden/jpeg.npz (tests/mutants.py: what test_decoders_survive_corrupt_files feeds the shipped build), N of each of a handful of
PNG / BMP / PPM files, N line-level mutants of examples/assets/unit_cube.obj -- and runs the program over them once.  Exit status 0 =
the sanitizers had nothing to report.  Run by hand; loads nothing into Python; not for a GPU machine."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from mutants import mutate_bytes, mutate_lines                       # noqa: E402
from simple_raytracer_amd.build import HOST_CPU_SRCS                 # noqa: E402

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-O1"]


def build(out):
    cmd = ["g++"] + SANITIZE + ["-std=c++17", "-ffp-contract=off", "-pthread", "-o", out, os.path.join(ROOT, "tools", "host_sanitize_main.cpp")] + HOST_CPU_SRCS + ["-lz"]
    subprocess.run(cmd, check=True)
    needed = subprocess.run(["ldd", out], check=True, capture_output=True, text=True).stdout
    assert "libsrt_hip" not in needed and "libamdhip64" not in needed, needed


def small_images(d):
    """(file name, bytes) of small valid PNG / BMP / PPM files in the pixel formats their decoders know."""
    rng = np.random.default_rng(3)
    rgb = rng.integers(0, 256, (20, 32, 3), dtype=np.uint8)
    forms = [("rgb.png", Image.fromarray(rgb), {}), ("rgba.png", Image.fromarray(np.dstack([rgb, rgb[..., :1]])), {}),
             ("grey.png", Image.fromarray(rgb[..., 0]), {}), ("pal.png", Image.fromarray(rgb).quantize(16), {}),
             ("big.png", Image.fromarray(np.tile(rgb, (4, 4, 1))), {"compress_level": 9}),
             ("rgb.bmp", Image.fromarray(rgb[:, :31]), {}), ("pal.bmp", Image.fromarray(rgb).quantize(16), {}),
             ("rgb.ppm", Image.fromarray(rgb), {}), ("grey.pgm", Image.fromarray(rgb[..., 0]), {})]
    out = []
    for name, image, options in forms:
        image.save(os.path.join(d, name), **options)
        out.append((name, open(os.path.join(d, name), "rb").read()))
    return out


def crafted(images):
    """(file name, bytes): headers that declare what their files cannot hold -- each was a defect a sanitizer run of the loaders found."""
    files = dict(images)
    png, bmp = bytearray(files["rgb.png"]), files["rgb.bmp"]
    png[16:24] = b"\x00\x01\x00\x00\x7f\xff\xff\xff"                                   # IHDR: 65536 x (2^31 - 1) pixels in 2 kB
    return [("huge.png", bytes(png)), ("offset.bmp", bmp[:10] + b"\xff\xff\xff\xff" + bmp[14:]),      # pixel data 1 byte before the file
            ("height.bmp", bmp[:22] + b"\x00\x00\x00\x80" + bmp[26:])]                          # INT32_MIN rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--jpeg", type=int, default=1200, help="mutants of each of the 18 JPEG files")
    ap.add_argument("--image", type=int, default=1000, help="mutants of each of the 9 PNG / BMP / PPM files")
    ap.add_argument("--obj", type=int, default=4000, help="mutants of the unit cube's OBJ file")
    ap.add_argument("--keep", help="write the files here and keep them")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        d = args.keep or tmp
        os.makedirs(d, exist_ok=True)
        t0 = time.time()
        build(os.path.join(tmp, "host_sanitize"))
        t_build = time.time() - t0
        rng = np.random.default_rng(5)
        paths = []

        def put(name, data):
            paths.append(os.path.join(d, name))
            with open(paths[-1], "wb") as f:
                f.write(data)
        z = np.load(os.path.join(ROOT, "tests", "golden", "jpeg.npz"))
        for name in z["names"]:
            base = z[f"{name}_file"].tobytes()
            put(f"{name}.jpg", base)
            for i in range(args.jpeg):
                put(f"{name}_{i}.jpg", mutate_bytes(rng, base))
        images = small_images(d)
        for name, base in images:
            stem, ext = os.path.splitext(name)
            paths.append(os.path.join(d, name))
            for i in range(args.image):
                put(f"{stem}_{i}{ext}", mutate_bytes(rng, base))
        for name, data in crafted(images):
            put(name, data)
        cube = open(os.path.join(ROOT, "examples", "assets", "unit_cube.obj")).read()
        put("cube.obj", cube.encode())
        for i in range(args.obj):
            put(f"cube_{i}.obj", mutate_lines(rng, cube).encode())
        with open(os.path.join(d, "list.txt"), "w") as f:
            f.write("\n".join(paths) + "\n")
        print(f"{len(z['names'])} x {args.jpeg} JPEG, {len(images)} x {args.image} PNG / BMP / PPM, {args.obj} OBJ mutants, the {len(z['names']) + len(images) + 1} files themselves and 3 crafted headers", flush=True)
        t0 = time.time()
        rc = subprocess.run([os.path.join(tmp, "host_sanitize"), os.path.join(d, "list.txt")]).returncode
        print(f"build {t_build:.0f} s, run {time.time() - t0:.0f} s, exit status {rc}")
        return rc


if __name__ == "__main__":
    sys.exit(main())
