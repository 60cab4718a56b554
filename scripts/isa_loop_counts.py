#!/usr/bin/env python3
"""Instruction counts of the basic blocks of one kernel in a device assembly file (scripts/isa_snapshot.py, or
hipcc --cuda-device-only -S with the unit's flags): per block the VALU, scalar, LDS, vector-memory and
scalar-memory instructions, the F64 FMA / MUL / ADD among the VALU, and the branch targets, so that a
loop body -- a block, or a chain of blocks, that branches back to itself -- can be read off and summed.

    python scripts/isa_loop_counts.py walk.s 'k_walk_fwd_mILi3ELb1ELb1ELb1E' [min VALU per block to print]
"""
import re
import sys


def blocks(path, key):
    """[(label, [instruction lines])] of the first function whose mangled name contains key"""
    out, cur, inside = [], None, False
    with open(path) as fh:
        for ln in fh:
            s = ln.strip()
            m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
            if m and not s.startswith(".L") and not inside and key in m.group(1) and s.startswith("_Z"):
                inside, cur = True, (m.group(1), [])
                out.append(cur)
                continue
            if not inside:
                continue
            if s.startswith(".Lfunc_end"):
                break
            if m:
                cur = (m.group(1), [])
                out.append(cur)
            elif s and not s.startswith((".", ";")):
                cur[1].append(s.split(";")[0].strip())
    return out


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith(("s_load", "s_buffer_load")):
        return "smem"
    return "salu"


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    floor = int(argv[3]) if len(argv) > 3 else 0
    bl = blocks(argv[1], argv[2])
    if not bl:
        sys.exit("no function matches " + argv[2])
    print(bl[0][0])
    for label, ins in bl:
        n = {"valu": 0, "salu": 0, "lds": 0, "vmem": 0, "smem": 0}
        f64 = {"fma": 0, "mul": 0, "add": 0}
        targets = []
        for i in ins:
            n[classify(i)] += 1
            op = i.split()[0]
            for k in f64:
                if re.match(r"v_(%s|%sc|%sak|%sk)_f64" % (k, k, k, k), op) or (k == "fma" and op.startswith("v_fmac_f64")):
                    f64[k] += 1
            if op.startswith(("s_cbranch", "s_branch")):
                targets.append(i.split()[-1])
        if n["valu"] >= floor:
            print((f"{label:>12}: valu {n['valu']:4d} (f64 fma {f64['fma']:3d} mul {f64['mul']:3d} add {f64['add']:3d}) "
                   f"salu {n['salu']:3d} lds {n['lds']:2d} vmem {n['vmem']:2d} smem {n['smem']:2d} -> {' '.join(targets)}").rstrip())


if __name__ == "__main__":
    main(sys.argv)
