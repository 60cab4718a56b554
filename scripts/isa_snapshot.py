#!/usr/bin/env python3
"""Device assembly of every translation unit of the default build, for an exact before/after diff.

    python scripts/isa_snapshot.py OUTDIR

Every unit of build._units(()) is compiled with the library's own flags plus `--cuda-device-only -S`
into OUTDIR/<object name>.s, and the lines that carry the per-compilation `__hip_cuid_<hash>` symbol
are dropped.  The output has no line information, so two trees whose kernels are the same machine
code give byte-identical directories: `diff -r` of two snapshots is an exact test of a refactor
(a moved definition, a folded switch, a split header).  No GPU is needed; at most 16 compilers run.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robustgrape_amd import build  # noqa: E402


def snapshot(unit, outdir):
    src, extra, obj = unit
    out = os.path.join(outdir, os.path.splitext(os.path.basename(obj))[0] + ".s")
    cmd = [build.HIPCC] + build.FLAGS + extra + ["--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    with open(out) as fh:
        lines = [ln for ln in fh if "__hip_cuid_" not in ln]
    with open(out, "w") as fh:
        fh.writelines(lines)
    return out, sum(ln.lstrip().startswith(".amdhsa_kernel ") for ln in lines)


def main(argv):
    if len(argv) != 2:
        sys.exit(__doc__)
    outdir = argv[1]
    os.makedirs(outdir, exist_ok=True)
    units = build._units(())[1]
    jobs = max(1, min(len(units), int(os.environ.get("MAX_JOBS", os.cpu_count() or 4)), 16))
    with ThreadPoolExecutor(jobs) as pool:
        for out, nk in pool.map(lambda u: snapshot(u, outdir), units):
            print(f"{os.path.basename(out)}: {nk} kernels", flush=True)
    print(f"{len(units)} units -> {outdir}")


if __name__ == "__main__":
    main(sys.argv)
