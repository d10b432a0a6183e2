#!/usr/bin/env python3
"""Per-kernel register / spill / occupancy table of the HIP engine (cross-compiles for gfx950; no GPU needed).

    python tools/kernel_resources.py [extra hipcc flags, e.g. -DMGPU_RECIP_MINWAVES=5] [--filter substr]
    python tools/kernel_resources.py --isa-digest [--root OTHER_CHECKOUT] [...]

--isa-digest adds, per kernel symbol, a digest of its device assembly (the text between the kernel's label and its
.Lfunc_end, without comments, .file / .ident / .loc lines and with the per-function numbers of local labels removed, so
that a kernel that merely moved inside or between translation units keeps its digest).  The table is then sorted by
mangled symbol over the union of the translation units, one line per symbol: two such tables (say of a parent commit and
of a branch, --root) compare with diff.  A symbol emitted by more than one unit shows every distinct digest it got.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ("mgpu_engine.hip", "mgpu_launch.hip", "mgpu_lanes.hip", "mgpu_windows.hip", "mgpu_replicas.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fopenmp", "-Rpass-analysis=kernel-resource-usage"]
KEYS = [("vgpr", r"VGPRs"), ("agpr", r"AGPRs"), ("sgpr", r"SGPRs"), ("spillV", r"VGPRs? Spill"), ("spillS", r"SGPRs? Spill"),
        ("scratch", r"ScratchSize \[bytes/lane\]"), ("occ", r"Occupancy \[waves/SIMD\]"), ("lds", r"LDS Size \[bytes/block\]")]


def compile_unit(src, workdir, extra, digest):
    """-> (the compiler's remarks, the device assembly or None)"""
    out = os.path.join(workdir, os.path.basename(src) + (".s" if digest else ".o"))
    mode = ["--offload-device-only", "-S"] if digest else ["-c"]
    p = subprocess.run(["hipcc"] + FLAGS + mode + [src, "-o", out] + extra, capture_output=True, text=True, cwd=workdir)
    if p.returncode != 0:
        sys.exit(p.stderr[-4000:])
    asm = None
    if digest:
        with open(out) as fh:
            asm = fh.read()
    return p.stderr, asm


def resources(remarks):
    """mangled symbol -> the resource columns"""
    table = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", remarks)[1:]:
        vals = []
        for label, k in KEYS:
            m = re.search(k + r": (\d+)", b)
            vals.append(f"{label} {m.group(1) if m else '?':>4s}")
        table[b.split("\n")[0].split()[0]] = "  ".join(vals)
    return table


def isa_digests(asm):
    """kernel symbol -> sha256 (first 16 hex digits) of its code"""
    lines = [ln.split(";")[0].strip() for ln in asm.splitlines()]
    digests = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M):
        start = lines.index(sym + ":")
        h = hashlib.sha256()
        for s in lines[start + 1:]:
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith((".file", ".ident", ".loc", ".cfi_")):
                continue
            h.update(re.sub(r"\.L([A-Za-z_]+?)\d+_(\d+)", r".L\1_\2", s).encode() + b"\n")
        digests[sym] = h.hexdigest()[:16]
    return digests


def short_name(demangled):
    return re.sub(r"\(.*", "", demangled).replace("void ", "").replace("mgpu::", "")


def main():
    args = sys.argv[1:]
    flt, root = None, ROOT
    digest = "--isa-digest" in args
    if digest:
        args.remove("--isa-digest")
    if "--filter" in args:
        i = args.index("--filter")
        flt = args[i + 1]
        del args[i:i + 2]
    if "--root" in args:
        i = args.index("--root")
        root = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    srcs = [os.path.join(root, "maniac_mc_amd", "csrc", f) for f in UNITS]
    srcs = [s for s in srcs if os.path.exists(s)]          # (--root of a checkout from before a unit was added)
    with tempfile.TemporaryDirectory() as d, ThreadPoolExecutor(max_workers=len(srcs)) as pool:
        built = list(pool.map(lambda s: compile_unit(s, d, args, digest), srcs))
    rows = []            # (mangled symbol, resource columns), in the units' order
    isa = {}             # mangled symbol -> its distinct digests
    for remarks, asm in built:
        rows += resources(remarks).items()
        for sym, dg in (isa_digests(asm) if digest else {}).items():
            if dg not in isa.setdefault(sym, []):
                isa[sym].append(dg)
    if digest:
        rows = sorted(set(r for r in rows if r[0] in isa))
    dem = subprocess.run(["c++filt"] + [r[0] for r in rows], capture_output=True, text=True).stdout.splitlines()
    for (sym, cols), name in zip(rows, dem):
        name = short_name(name)
        if flt and flt not in name:
            continue
        if digest:
            print(f"{name:70s} isa {'/'.join(isa[sym])}  {cols}  {sym}")
        else:
            print(f"{name:62s} {cols}")


if __name__ == "__main__":
    main()
