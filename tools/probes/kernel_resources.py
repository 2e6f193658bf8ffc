#!/usr/bin/env python3
"""Per-kernel resource table from hipcc's ``-Rpass-analysis=kernel-resource-usage`` remarks.

    hipcc <the flags of csrc/build.py> -Rpass-analysis=kernel-resource-usage -c csrc/gemm_skinny.hip \
        -o /tmp/a.o 2> a.remarks
    python tools/probes/kernel_resources.py a.remarks [b.remarks ...] > table.txt

One line per kernel, sorted, keyed by kernel family and template arguments (not by source file or
line, so two trees whose wrappers moved or were renamed can be diffed). The fp8 one-tile wrapper
of older trees (``skinny_gemm_fp8_kernel<P, E, NW, U>``) is written as today's
``skinny_gemm_kernel<P, E, NW, U, 1>``.
"""
import re
import shutil
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]",
          "Occupancy [waves/SIMD]"]


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def key(name):
    name = name.replace("(anonymous namespace)::", "")
    name = re.sub(r"^void ", "", name)
    m = re.match(r"([\w:]+)(<[^(]*>)?\(", name)
    fam, targs = m.group(1), [a.strip() for a in (m.group(2) or "<>")[1:-1].split(",") if a.strip()]
    if fam == "skinny_gemm_fp8_kernel":
        fam, targs = "skinny_gemm_kernel", targs + ["1"]
    elif fam == "skinny_gemm_kernel" and len(targs) == 4:
        targs = targs + ["0"]
    return fam + ("<" + ", ".join(targs) + ">" if targs else "")


def main(paths):
    rows, cur = {}, None
    for p in paths:
        for line in open(p):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = rows.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([^:]+): (\S+) \[-Rpass", line)
            if m and cur is not None:
                cur[m.group(1)] = m.group(2)
    names = list(rows)
    table = sorted((key(d), rows[n]) for n, d in zip(names, demangle(names)))
    print("# kernel | " + " | ".join(FIELDS))
    for k, r in table:
        print(k + " | " + " | ".join(r.get(f, "?") for f in FIELDS))
    print(f"# {len(table)} kernels")


if __name__ == "__main__":
    main(sys.argv[1:])
