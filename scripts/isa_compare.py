#!/usr/bin/env python3
"""Compare two snapshots of scripts/isa_snapshot.py kernel by kernel.

    python scripts/isa_compare.py DIR_A DIR_B

`diff -r` of two snapshots is the exact test, and it applies as long as both trees emit the same
functions in the same order.  Removing a kernel, or instantiating the same kernels in another order,
renumbers the local labels (`.LBB<function index>_<block>`, `.Lfunc_end<index>`) and reorders the file.
This compares what is left when that is taken out; it is looser than `diff -r` in exactly these ways:

- per unit, every function's text (code, `.amdhsa_kernel` block, resource `.set` lines) is compared under
  its symbol name, with the function index of local labels normalised and runs of blanks squeezed;
- everything from the first `;` of a line on is dropped as an assembler comment (the register names in
  `; implicit-def` notes vary).  The compiler's output has no `;` inside string data today (kernels hold no
  `.ascii` / `.asciz` strings); a line that did would be cut there and compared only up to it;
- the metadata entries are compared as a set, one per kernel;
- the lines outside any function (file header, trailer, constants) are compared as a multiset, except the
  section switches around a function and the end padding of the plain `.text` section (GLUE below), which
  exist only while a non-template kernel lives in that section.

Prints the functions only one side has and those that differ; exit status 0 when nothing common differs.
"""
from __future__ import annotations

import os
import re
import sys

BEGIN = re.compile(r"; -- Begin function (\S+)")
# not compared outside the functions (see above)
GLUE = {" .text", " .p2align 8", ' .section .AMDGPU.csdata,"",@progbits', " .p2alignl 6, 3212836864",
        " .fill 256, 4, 3212836864"}
LABEL = re.compile(r"BB\d+_|\.L(func_end|func_begin|JTI|tmp)\d+")


def norm(line):
    line = LABEL.sub(lambda m: "BBN_" if m.group(1) is None else ".L" + m.group(1) + "N", line)
    line = line.split(";", 1)[0]  # assembler comments are not code (the register names of `implicit-def` notes vary)
    return re.sub(r"\s+", " ", line).rstrip()


def split(path):
    """{function: its lines}, {metadata kernel entry}, [everything else]"""
    funcs, meta, rest = {}, set(), []
    cur = rest
    lines = open(path).read().split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        if ln.startswith("\t.section\t.text.") and i + 1 < len(lines) and BEGIN.search(lines[i + 1]):
            cur = funcs.setdefault(BEGIN.search(lines[i + 1]).group(1), [])
        elif BEGIN.search(ln) and not (i and lines[i - 1].startswith("\t.section\t.text.")):
            cur = funcs.setdefault(BEGIN.search(ln).group(1), [])
        elif ln.startswith("\t.amdgpu_metadata"):
            j = lines.index("\t.end_amdgpu_metadata", i)
            entry = []  # one per kernel: from its `  - .` line to the next one or to the next top-level key
            for m in lines[i + 1:j] + ["end:"]:
                if (m.startswith("  - .") or not m.startswith(" ")) and entry:
                    meta.add("\n".join(entry))
                    entry = []
                if m.startswith("  - .") or entry:
                    entry.append(m)
            i = j
            cur = rest
        cur.append(norm(ln))
        if ln.startswith("; COMPUTE_PGM_RSRC3_GFX90A:TG_SPLIT"):  # the last line of a kernel's own text
            cur = rest
        i += 1
    return funcs, meta, rest


def main(a, b):
    bad = 0
    units = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    for u in units:
        pa, pb = os.path.join(a, u), os.path.join(b, u)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{u}: only in {a if os.path.exists(pa) else b}")
            bad += 1
            continue
        fa, ma, ra = split(pa)
        fb, mb, rb = split(pb)
        differ = sorted(k for k in fa.keys() & fb.keys() if fa[k] != fb[k])
        print(f"{u}: {len(fa)} / {len(fb)} functions, {len(fa.keys() & fb.keys()) - len(differ)} identical")
        for k in sorted(fa.keys() - fb.keys()):
            print(f"  only in A: {k}")
        for k in sorted(fb.keys() - fa.keys()):
            print(f"  only in B: {k}")
        for k in differ:
            print(f"  DIFFERS: {k}")
        if len(ma ^ mb) != len(fa.keys() ^ fb.keys()):  # one metadata entry per kernel only one side has
            print(f"  METADATA differs beyond the removed kernels ({len(ma - mb)} / {len(mb - ma)} entries)")
            bad += 1
        if sorted(x for x in ra if x not in GLUE) != sorted(x for x in rb if x not in GLUE):
            print("  text outside functions differs")
            bad += 1
        bad += len(differ)
    print("identical otherwise" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
