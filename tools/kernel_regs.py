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
                                                VGPR / SGPR / scratch / LDS / spills of both.  "moved": same registers, same length,
                                                and nothing differs but the literal of the one pc-relative call named above (an
                                                s_add_u32 / s_addc_u32 literal behind an s_getpc_b64), in a kernel that lies behind
                                                one that changed length; counted apart from the identical ones
       --lib PATH                               the library to read instead of simple_raytracer_amd/libsrt_hip.so"""
import hashlib, os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "simple_raytracer_amd", "libsrt_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
GETPC_OP = 0x1C                           # s_getpc_b64 (SOP1) on gfx9 / gfx950
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


def kernel_digests(co, d, code=None):
    """mangled name -> digest of the kernel symbol's own bytes of .text (code: a dict that receives the bytes themselves)"""
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
            if code is not None:
                code[f[7]] = text[lo:lo + int(f[2])]
    return out


def regs(r):
    return (f"vgpr {r.get('vgpr_count','?'):>4} sgpr {r.get('sgpr_count','?'):>4} scratch {r.get('private_segment_fixed_size','?'):>5} "
            f"lds {r.get('group_segment_fixed_size','?'):>6} spill {r.get('vgpr_spill_count','0')}")


def read(lib, d, want_digests):
    os.makedirs(d)
    co = code_object(lib, d)
    rows = kernel_rows(notes(co))
    code = {}
    dig = kernel_digests(co, d, code) if want_digests else {}
    for r in rows:
        r["digest"] = dig.get(r["name"], "?")
        r["code"] = code.get(r["name"], b"")
    return rows


def moved_only(x, y):
    """Two kernels' bytes: equal length, and every dword that differs is the 32-bit literal of an s_add_u32 / s_addc_u32 that follows an
    s_getpc_b64 within two instructions -- the pc-relative address of a call -- and at most two dwords differ.  Anything else is a change."""
    if len(x) != len(y):
        return False
    dw = lambda b, i: int.from_bytes(b[4 * i:4 * i + 4], "little")
    diff = [i for i in range(len(x) // 4) if dw(x, i) != dw(y, i)]
    for i in diff:
        op = dw(x, i - 1) if i else 0
        # SOP2: bits 31:30 = 10, op 29:23 (0 s_add_u32, 4 s_addc_u32), a source operand of 255 = a literal follows
        add_lit = i and op == dw(y, i - 1) and op >> 30 == 2 and (op >> 23) & 0x7F in (0, 4) and 255 in (op & 0xFF, (op >> 8) & 0xFF)
        # SOP1 s_getpc_b64: 0xBE80 in bits 31:16 with the opcode in 15:8
        getpc = any(k >= 0 and dw(x, k) & 0xFF80FF00 == 0xBE800000 | GETPC_OP << 8 for k in range(i - 5, i - 1))
        if not (add_lit and getpc):
            return False
    return 0 < len(diff) <= 2


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
            same = moved = 0
            print(f"# A = {other}\n# B = {lib}\n# digest: SHA-256 of the bytes of .text under the kernel's own symbol")
            for r in a:
                if not keep(r["short"]):
                    continue
                q = bn.pop(r["name"], None)
                if q is None:
                    print(f"{r['short']:90s} only in A  {regs(r)}")
                    continue
                regs_same = all(r.get(k) == q.get(k) for k in REGS)
                ident = r["digest"] == q["digest"] and regs_same
                mov = not ident and regs_same and moved_only(r["code"], q["code"])
                same += ident
                moved += mov
                print(f"{r['short']:90s} {'identical' if ident else 'moved    ' if mov else 'DIFFERENT'}  A: {regs(r)}  B: {regs(q)}")
            for q in bn.values():
                if keep(q["short"]):
                    print(f"{q['short']:90s} only in B  {regs(q)}")
            print(f"# {same} of {len(a)} kernels of A identical in B" + (f", {moved} more moved only" if moved else ""))
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
