#!/usr/bin/env python3
"""Compare two device-assembly files (hipcc <Makefile flags> --cuda-device-only -S) kernel by kernel: the same set of kernel symbols, and per
symbol identical instruction text, kernel descriptor (.amdhsa_* lines) and metadata entry (register / spill counts, LDS and scratch sizes, arguments).
Only the order of the kernels in the file may differ: local labels (.LBB<k>_<n>, .Lfunc_end<k>) carry the kernel's position k in the file, which is
dropped before comparing, as are the assembler's comments (they repeat those labels).  A host-side refactor must leave this at "identical".

    python tools/compare_device_asm.py parent/gemm_conv.s pr/gemm_conv.s [more pairs ...]

Exit status 0 when every pair is identical, 1 otherwise."""
import re
import sys


def split(path):
    """-> {symbol: (body, descriptor)}, {symbol: metadata entry} of the kernels in one .s file."""
    text = re.sub(r"\.L(BB|func_begin|func_end|tmp)\d+", r".L\1", open(path).read())
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    funcs, cur, name = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m and m.group(1) in kernels and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            cur.append(line.split(";")[0].rstrip())
            if re.match(r"^\s*\.end_amdhsa_kernel", line):
                funcs[name] = "\n".join(cur)
                cur = None
    meta = {}
    m = re.search(r"^amdhsa\.kernels:\n(.*?)^amdhsa\.", text, re.M | re.S)
    for entry in re.split(r"^  - ", m.group(1) if m else "", flags=re.M)[1:]:
        sym = re.search(r"\.name:\s+(\S+)", entry)
        meta[sym.group(1)] = entry
    return funcs, meta


def compare(a, b):
    (fa, ma), (fb, mb) = split(a), split(b)
    bad = []
    for what, x, y in (("kernel", fa, fb), ("metadata", ma, mb)):
        bad += [f"{what} only in {a}: {s}" for s in sorted(set(x) - set(y))]
        bad += [f"{what} only in {b}: {s}" for s in sorted(set(y) - set(x))]
        bad += [f"{what} differs: {s}" for s in sorted(set(x) & set(y)) if x[s] != y[s]]
    if set(fa) != set(ma):
        bad.append(f"{a}: kernels and metadata entries do not match up")
    print(f"{a} vs {b}: {len(fa)} / {len(fb)} kernels, " + ("identical" if not bad else f"{len(bad)} differences"))
    for line in bad:
        print("   ", line)
    return not bad


if __name__ == "__main__":
    if len(sys.argv) < 3 or len(sys.argv) % 2 == 0:
        sys.exit(__doc__)
    sys.exit(0 if all([compare(x, y) for x, y in zip(sys.argv[1::2], sys.argv[2::2])]) else 1)
