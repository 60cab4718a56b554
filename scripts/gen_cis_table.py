#!/usr/bin/env python3
"""Writes robustgrape_amd/csrc/grape_cis_table.hpp: (cos, sin)(2 pi k / 128), k = 0 .. 127, correctly rounded
doubles as hex-float literals (grape_cis::cis_tab's table).  The values come from Taylor series in 70-digit
decimal arithmetic; entries at multiples of pi / 2 are written as exact 0 and +-1.

    python scripts/gen_cis_table.py            # rewrite the header
    python scripts/gen_cis_table.py --check    # exit 1 if the committed header differs
"""
import os
import sys
from decimal import Decimal, getcontext

N = 128
getcontext().prec = 70
PI = Decimal("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899862803")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robustgrape_amd", "csrc",
                   "grape_cis_table.hpp")


def _series(x, first, n0):
    """sum of the alternating Taylor series with first term `first`, next factorial index n0 (sin: x, 2; cos: 1, 1)"""
    term, total, n, x2 = first, first, n0, x * x
    while abs(term) > Decimal(10) ** -68:
        term = -term * x2 / (n * (n + 1))
        total += term
        n += 2
    return total


def entry(k):
    """(cos, sin)(2 pi k / N) as doubles; the argument is folded into [0, pi / 2) first"""
    q, r = divmod(k, N // 4)       # quadrant, position inside it
    if r == 0:
        c, s = Decimal(1), Decimal(0)
    else:
        x = 2 * PI * r / N
        c, s = _series(x, Decimal(1), 1), _series(x, x, 2)
    for _ in range(q):             # rotate by pi / 2
        c, s = -s, c
    return float(c) + 0.0, float(s) + 0.0  # (+ 0.0: no negative zeros)


def render():
    lines = [
        "// grape_cis_table.hpp -- (cos, sin)(2 pi k / 128), k = 0 .. 127, correctly rounded: the table of",
        "// grape_cis::cis_tab (grape_cis.hpp).  Written by scripts/gen_cis_table.py; do not edit by hand.",
        "#pragma once",
        "",
        "#define GRAPE_CIS_TABLE_ENTRIES \\",
    ]
    rows = []
    for k in range(N):
        c, s = entry(k)
        rows.append("    {%s, %s}" % (c.hex(), s.hex()))
    lines.append(", \\\n".join(rows))
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv:
        with open(OUT) as fh:
            sys.exit(0 if fh.read() == text else 1)
    with open(OUT, "w") as fh:
        fh.write(text)
