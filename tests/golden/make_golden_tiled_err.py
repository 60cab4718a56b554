"""Generate tests/golden/tiled_err.npz: the tiled engine's error-source cases (64 < d <= 128, GRAPE_OPT_TILED_ERR)
from the CPU oracle and the exact (longdouble) evaluator.

Run from the repo root:  python tests/golden/make_golden_tiled_err.py [--live]
Per case (d, N_t, ne, phase, scale) of the C5 family with error sources (robustgrape_amd/synthetic.py
dense_error_problem) the fixture holds x and the four outputs of oracle/grape_oracle.py and of
oracle/grape_exact.py (fidelity_and_derivatives): a few KB of numbers, no matrices.  Each case prints the
oracle's own distance from the exact value against half the tier of tests/test_gpu_tiled_err.py: a case is
kept only where that distance is at most 0.75 of it.  --live also measures the two cases that the test runs
live (they are not stored).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import grape_exact as E  # noqa: E402
from oracle import grape_oracle as O  # noqa: E402
from robustgrape_amd import synthetic as S  # noqa: E402

LIVE = [(65, 1, 1, False, 1.0), (65, 5, 2, True, 1.0)]
# the user's size with a last chunk of one step; P = d, four full tiles, the x_add target; weights in the first
# tile only, Taylor 8; one squaring shared by every variant of a step; and the evaluation that the slab-seam test
# puts on the seam (d = 65, N_t = 7).  The fourth case was meant at scale 2.0, where the oracle's F_dx sits at 0.92
# of half the tier (1.5: 0.94); at 1.75 it is 0.40, |A|_1 = 0.88 .. 1.28: steps with one squaring and steps with none.
CASES = [(81, 7, 1, False, 1.0), (128, 3, 2, True, 1.0), (113, 4, 1, False, 0.05), (96, 6, 2, False, 1.75),
         (65, 7, 1, False, 1.0)]


def problem(d, ntimes, nerr, phase, scale):
    """(fidelity problem, x) of a case: x = dense_x(N_t, seed 500 + N_t), x_add = 0.7 appended for phase."""
    x = S.dense_x(ntimes, seed=500 + ntimes)
    fp = S.dense_error_problem(d, ntimes, rank=16, scale=scale, nerr=nerr, phase=phase)
    return fp, (np.concatenate([x, [0.7]]) if phase else x)


def evaluate(case):
    fp, x = problem(*case)
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    exact = E.fidelity_and_derivatives(fp, x, nparam=2)
    ref = [np.asarray(a, dtype=np.float64) for a in ref]
    exact = [np.asarray(a, dtype=np.float64) for a in exact]
    half = [0.5e-12, 0.5 * (1e-6 * np.max(np.abs(exact[1])) + 1e-9), 0.5 * (1e-6 * np.max(np.abs(exact[2])) + 1e-7),
            0.5 * (1e-5 * np.max(np.abs(exact[3])) + 1e-7)]
    dist = [float(np.max(np.abs(r - e))) for r, e in zip(ref, exact)]
    print(f"case {case}: oracle - exact / half tier: " +
          ", ".join(f"{n} {a:.2e} / {h:.2e} ({a / h:.2f})" for n, a, h in zip(("F", "F_dx", "F_d2err", "F_d2err_dx"), dist, half)),
          flush=True)
    return x, ref, exact


def main():
    if "--live" in sys.argv:
        for case in LIVE:
            evaluate(case)
    out = {"cases": np.array([[d, nt, ne, int(ph)] for d, nt, ne, ph, _ in CASES], dtype=np.int64),
           "scales": np.array([sc for *_, sc in CASES])}
    names = ("F", "F_dx", "F_d2err", "F_d2err_dx")
    for i, case in enumerate(CASES):
        x, ref, exact = evaluate(case)
        out[f"x{i}"] = x
        for n, r, e in zip(names, ref, exact):
            out[f"{n}{i}"], out[f"{n}_exact{i}"] = r, e
    np.savez_compressed(os.path.join(HERE, "tiled_err.npz"), **out)
    print("wrote tiled_err.npz")


if __name__ == "__main__":
    main()
