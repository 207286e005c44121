#!/usr/bin/env python3
"""Registers, scratch and LDS of every kernel in libsrt_hip.so (from the code object's metadata notes).
Usage: python tools/kernel_regs.py [substring ...]
       python tools/kernel_regs.py --digest     SHA-256 of the gfx950 code object's .text, .rodata (kernel descriptors) and metadata
                                                notes: equal digests before and after a host-only change = the kernels are untouched
                                                (the whole code object is not comparable: its symbol table carries a hash of the source)
       python tools/kernel_regs.py --digest --kernels [substring ...]
                                                one digest per kernel beside its registers: SHA-256 (first 16 hex digits) of the bytes
                                                of .text that the kernel's own symbol covers (address and size from the symbol table).
                                                A kernel that merely moves because an earlier one changed length keeps its digest:
                                                branches inside a kernel are relative; a pc-relative reference to something OUTSIDE the
                                                kernel would change it (the kernels that store lit pixels make one: the call
                                                of quant_tone_exact, srt_device.h; every other kernel is fully inlined).
       python tools/kernel_regs.py --compare OTHER.so [substring ...]
                                                the same per kernel for two builds side by side, OTHER.so first: identical or not,
                                                VGPR / SGPR / scratch / LDS / spills of both
       --lib PATH                               the library to read instead of simple_raytracer_amd/libsrt_hip.so"""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "simple_raytracer_amd", "libsrt_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
REGS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")


def code_object(lib, d):
    """The gfx950 code object of `lib`, unbundled into directory d."""
    co = f"{d}/k.co"
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", f"--input={lib}", f"--output={co}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=False, capture_output=True)
    if not os.path.exists(co) or os.path.getsize(co) == 0:
        # fat binary section: extract with objcopy
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={d}/fat.bin", lib], check=True)
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--unbundle", f"--input={d}/fat.bin", f"--output={co}",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], check=True)
    return co


def notes(co):
    return subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout


def section(co, sec, d):
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f"{sec}={d}/sec.bin", co, f"{d}/unused.co"], check=True)
    with open(f"{d}/sec.bin", "rb") as f:
        return f.read()


def kernel_rows(txt):
    """One dict per kernel of the metadata notes: mangled name, demangled name without arguments, registers."""
    cur = {}
    rows = []
    for line in txt.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == "name" and v.startswith(("_Z", "k_")) and "kd" not in v:
            cur["name"] = v
        if k in REGS + ("agpr_count",):
            cur[k] = v
        if k == "wavefront_size":
            if "name" in cur:
                rows.append(cur)
            cur = {}
    dem = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(rows, dem):
        r["short"] = n.replace("void ", "").split("(")[0]
    return rows


def kernel_digests(co, d):
    """mangled name -> digest of the kernel symbol's own bytes of .text"""
    text = section(co, ".text", d)
    hdr = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", "--wide", co], capture_output=True, text=True, check=True).stdout
    base = next(int(m.group(1), 16) for m in (re.search(r"\s\.text\s+PROGBITS\s+([0-9a-f]+)", l) for l in hdr.splitlines()) if m)
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC":
            lo = int(f[1], 16) - base
            out[f[7]] = hashlib.sha256(text[lo:lo + int(f[2])]).hexdigest()[:16]
    return out


def regs(r):
    return (f"vgpr {r.get('vgpr_count','?'):>4} sgpr {r.get('sgpr_count','?'):>4} scratch {r.get('private_segment_fixed_size','?'):>5} "
            f"lds {r.get('group_segment_fixed_size','?'):>6} spill {r.get('vgpr_spill_count','0')}")


def read(lib, d, want_digests):
    os.makedirs(d)
    co = code_object(lib, d)
    rows = kernel_rows(notes(co))
    dig = kernel_digests(co, d) if want_digests else {}
    for r in rows:
        r["digest"] = dig.get(r["name"], "?")
    return rows


def main():
    args = sys.argv[1:]
    lib, other = LIB, None
    for flag in ("--lib", "--compare"):
        if flag in args:
            i = args.index(flag)
            if flag == "--lib":
                lib = args[i + 1]
            else:
                other = args[i + 1]
            del args[i:i + 2]
    digest, per_kernel = "--digest" in args, "--kernels" in args
    pats = [a for a in args if a not in ("--digest", "--kernels")]
    keep = lambda n: not pats or any(p in n for p in pats)
    with tempfile.TemporaryDirectory() as d:
        if other:
            a, b = read(other, f"{d}/a", True), read(lib, f"{d}/b", True)
            bn = {r["name"]: r for r in b}
            same = 0
            print(f"# A = {other}\n# B = {lib}\n# digest: SHA-256 of the bytes of .text under the kernel's own symbol")
            for r in a:
                if not keep(r["short"]):
                    continue
                q = bn.pop(r["name"], None)
                if q is None:
                    print(f"{r['short']:90s} only in A  {regs(r)}")
                    continue
                ident = r["digest"] == q["digest"] and all(r.get(k) == q.get(k) for k in REGS)
                same += ident
                print(f"{r['short']:90s} {'identical' if ident else 'DIFFERENT'}  A: {regs(r)}  B: {regs(q)}")
            for q in bn.values():
                if keep(q["short"]):
                    print(f"{q['short']:90s} only in B  {regs(q)}")
            print(f"# {same} of {len(a)} kernels of A identical in B")
            return
        if digest and not per_kernel:
            os.makedirs(f"{d}/x")
            co = code_object(lib, f"{d}/x")
            for sec in (".text", ".rodata"):
                print(f"{sec:8s} {hashlib.sha256(section(co, sec, d)).hexdigest()}")
            print(f"{'notes':8s} {hashlib.sha256(notes(co).encode()).hexdigest()}")
            return
        for r in read(lib, f"{d}/x", digest):
            if keep(r["short"]):
                print(f"{r['short']:90s} " + (f"{r['digest']}  " if digest else "") + regs(r))


if __name__ == "__main__":
    main()
