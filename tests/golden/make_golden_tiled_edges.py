"""Generate tests/golden/tiled_edges.npz: the slow cases of tests/test_gpu_tiled_edges.py (above 81 levels, or
more than about ten steps) from the CPU oracle and the exact (longdouble) forward difference.

Run from the repo root:  python tests/golden/make_golden_tiled_edges.py
Per case of tests/problems.py tiled_edge_case the fixture holds x, F, F_dx (oracle/grape_oracle.py), F_exact,
F_dx_exact (oracle/grape_exact.py) and the case parameters (d, N_t, np): a few KB of numbers, no matrices.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import grape_exact as E  # noqa: E402
from oracle import grape_oracle as O  # noqa: E402
from tests import problems as Pm  # noqa: E402

CASES = ["proj113", "seam23"]


def main():
    out = {"names": np.array(CASES)}
    for name in CASES:
        fp, x, nparam = Pm.tiled_edge_case(name)
        up = fp.unitary_problem
        F, Fdx, _, _ = O.calculate_fidelity_and_derivatives(fp, x)
        Fe, Fdxe = E.fidelity_and_gradient(fp, x, nparam=nparam)
        out[f"params_{name}"] = np.array([up.ndim, up.ntimes, nparam], dtype=np.int64)
        out[f"x_{name}"], out[f"F_{name}"], out[f"F_dx_{name}"] = x, np.float64(F), np.asarray(Fdx)
        out[f"F_exact_{name}"], out[f"F_dx_exact_{name}"] = np.float64(Fe), np.asarray(Fdxe)
        se = np.max(np.abs(Fdxe))
        print(f"{name} (d, N_t, np) = {(up.ndim, up.ntimes, nparam)}: F {F:.12f}  oracle - exact "
              f"{np.max(np.abs(Fdx - Fdxe)):.2e} = {np.max(np.abs(Fdx - Fdxe)) / (0.5 * (1e-6 * se + 1e-9)):.2f} of half the "
              f"tier at max |F_dx| = {se:.2e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "tiled_edges.npz"), **out)
    print("wrote tiled_edges.npz")


if __name__ == "__main__":
    main()
