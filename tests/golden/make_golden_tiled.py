"""Generate tests/golden/tiled.npz: the tiled engine's slow cases (64 < d <= 128) from the CPU oracle
and the exact (longdouble) forward difference.

Run from the repo root:  python tests/golden/make_golden_tiled.py
Per case (d, N_t, scale, phase) of the C5 family (robustgrape_amd/synthetic.py) the fixture holds
x, F, F_dx (oracle/grape_oracle.py), F_exact, F_dx_exact (oracle/grape_exact.py) and the case
parameters: a few KB of numbers, no matrices.  5-75 s of CPU per case and evaluator.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import grape_exact as E  # noqa: E402
from oracle import grape_oracle as O  # noqa: E402
from robustgrape_amd import synthetic as S  # noqa: E402

# every padded size (80, 96, 112, 128), P != d and P = d, one chunk remainder each way (N_t = 19, 7),
# Taylor 8 (scale 0.05), one squaring (scale 2.0: |A|_1 = 1.42), the x_add target (phase)
CASES = [(80, 7, 0.3, False), (81, 5, 1.0, False), (96, 4, 0.05, False), (112, 2, 2.0, False),
         (128, 3, 1.0, True), (128, 19, 1.0, False)]


def problem(d, ntimes, scale, phase):
    """(fidelity problem, x) of a case: x = dense_x(N_t, seed 300 + N_t), x_add = 0.3 appended for phase."""
    x = S.dense_x(ntimes, seed=300 + ntimes)
    if phase:
        return S.dense_error_problem(d, ntimes, rank=16, scale=scale, nerr=0, phase=True), np.concatenate([x, [0.3]])
    return S.dense_problem(d, ntimes, rank=16, scale=scale), x


def main():
    out = {"cases": np.array([[d, nt, int(ph)] for d, nt, _, ph in CASES], dtype=np.int64),
           "scales": np.array([sc for _, _, sc, _ in CASES])}
    for i, (d, nt, sc, ph) in enumerate(CASES):
        fp, x = problem(d, nt, sc, ph)
        F, Fdx, _, _ = O.calculate_fidelity_and_derivatives(fp, x)
        Fe, Fdxe = E.fidelity_and_gradient(fp, x, nparam=2)
        out[f"x{i}"], out[f"F{i}"], out[f"F_dx{i}"] = x, np.float64(F), np.asarray(Fdx)
        out[f"F_exact{i}"], out[f"F_dx_exact{i}"] = np.float64(Fe), np.asarray(Fdxe)
        print(f"case {i} {(d, nt, sc, ph)}: F {F:.12f}  oracle - exact {np.max(np.abs(Fdx - Fdxe)):.2e} of "
              f"{np.max(np.abs(Fdxe)):.2e}", flush=True)
    np.savez_compressed(os.path.join(HERE, "tiled.npz"), **out)
    print("wrote tiled.npz")


if __name__ == "__main__":
    main()
