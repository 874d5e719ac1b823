#!/usr/bin/env python3
"""Print the device-code manifest of a source tree: for every csrc/*.hip unit, compiled device-only for gfx950 with the build's flags,
one line per FUNC symbol of the code object (``unit func name size digest-of-its-bytes``) and one per kernel with the compiler's
resource report (VGPRs, SGPRs, scratch, occupancy, LDS).  Two trees hold the same kernels with the same machine code exactly when
``diff`` finds their manifests equal, which is how a host-side refactor of the launch code is checked without a GPU:

    python tools/kernel_manifest.py [--root TREE] [--jobs N] > manifest.txt
    python tools/kernel_manifest.py --summary < manifest.txt      # per-unit kernel counts and total device code size

The tool lists symbol names, sizes, a digest of each function's bytes (the order of the functions inside a code object follows the
order of instantiation and may differ between two such trees; their bytes do not) and the resource remarks; it decodes no
instruction of any kernel."""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
READELF = os.environ.get("LLVM_READELF", "/opt/rocm/llvm/bin/llvm-readelf")
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "--no-gpu-bundle-output", "-O3", "-std=c++17", "-ffp-contract=off",
         "-Rpass-analysis=kernel-resource-usage", "-c"]
REMARK = re.compile(r": remark:\s+(.*?)(?: \[-Rpass-analysis=kernel-resource-usage\])?$")


def unit_manifest(src: str, tmp: str) -> list:
    unit = os.path.basename(src)[:-4]
    obj = os.path.join(tmp, unit + ".co")
    out = subprocess.run([HIPCC] + FLAGS + [src, "-o", obj], capture_output=True, text=True)
    if out.returncode:
        sys.stderr.write(out.stderr[-4000:])
        raise SystemExit(f"{unit}: device compile failed")
    lines, data, text = [], open(obj, "rb").read(), None
    for row in subprocess.run([READELF, "-SW", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        f = row.replace("[", " ").replace("]", " ").split()
        if len(f) > 5 and f[1] == ".text":
            text = (int(f[3], 16), int(f[4], 16))   # address, file offset
    if text is None:
        raise SystemExit(f"{unit}: no .text section in the section table of {obj}")
    for row in subprocess.run([READELF, "-sW", obj], capture_output=True, text=True, check=True).stdout.splitlines():
        f = row.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            at, size = int(f[1], 16) - text[0] + text[1], int(f[2], 0)
            lines.append(f"{unit} func {f[7]} {size} {hashlib.sha1(data[at:at + size]).hexdigest()[:16]}")
    name, fields = None, []
    for row in out.stderr.splitlines() + ["end: remark: Function Name: "]:
        m = REMARK.search(row)
        if not m:
            continue
        if m.group(1).startswith("Function Name:"):
            if name:
                lines.append(f"{unit} resources {name} " + "; ".join(fields))
            name, fields = m.group(1).split(":", 1)[1].strip(), []
        else:
            fields.append(" ".join(m.group(1).split()))
    return sorted(set(lines))   # (a shared code object lists each symbol in .symtab and .dynsym)


def summary(rows) -> None:
    units, total = {}, 0
    for row in rows:
        f = row.split()
        if len(f) == 5 and f[1] == "func":
            n, size = units.get(f[0], (0, 0))
            units[f[0]] = (n + 1, size + int(f[3]))
            total += int(f[3])
    for unit in sorted(units):
        print(f"{unit:28s} {units[unit][0]:5d} functions {units[unit][1]:10d} bytes")
    print(f"{'total':28s} {sum(n for n, _ in units.values()):5d} functions {total:10d} bytes")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--units", nargs="*", help="unit names (ptb_views ...); default: all")
    ap.add_argument("--summary", action="store_true", help="read a manifest on stdin, print per-unit counts and total size")
    args = ap.parse_args()
    if args.summary:
        return summary(sys.stdin)
    srcs = sorted(glob.glob(os.path.join(args.root, "pytorch_toolbelt_amd", "csrc", "*.hip")))
    if args.units:
        srcs = [s for s in srcs if os.path.basename(s)[:-4] in args.units]
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=args.jobs) as pool:
        for lines in pool.map(lambda s: unit_manifest(s, tmp), srcs):
            print("\n".join(lines))


if __name__ == "__main__":
    main()
