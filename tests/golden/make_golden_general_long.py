"""Generate tests/golden/general_long.npz: the reference of the k_u_fid_contract test past its grid cap
(tests/test_gpu_unitary_wrap.py, case table tests/unitary_wrap_cases.py): the d = 5 symmetric problem with both
error sources at N_t = 5500, 16 500 items of N_t np (1 + ne) against the kernel's 16 384 resident waves.

Run from the repo root:  python tests/golden/make_golden_general_long.py   (about 25 s of CPU)

H0 is Hermitian, so the longdouble evaluator applies (oracle/grape_exact.py fidelity_and_derivatives, 11 s); the
double oracle (oracle/grape_oracle.py, 12 s) enters only through its distance from it.  The fixture holds
    F, F_dx, F_d2err, F_d2err_dx     the longdouble values, cast to double
    noise_<output>                    max|oracle - exact| per output: the checker's own noise at this length
    x_sample                          x[::50] of tests/problems.py random_x(5500, 5500), which the test regenerates
    params                            (N_t, seed, stride)
-- about 140 KB; the full x and both references would be twice that.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import grape_exact as E  # noqa: E402
from oracle import grape_oracle as O  # noqa: E402
from tests import unitary_wrap_cases as W  # noqa: E402


def main():
    fp, x = W.long_problem(), W.long_x()
    exact = E.fidelity_and_derivatives(fp, x)
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    out = {"params": np.array([W.LONG_NT, W.LONG_SEED, W.LONG_X_STRIDE], dtype=np.int64),
           "x_sample": x[::W.LONG_X_STRIDE].copy()}
    for name, a, b in zip(W.LONG_OUTPUTS, exact, ref):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        out[name] = a
        out["noise_" + name] = np.float64(np.max(np.abs(a - b)))
        print(f"{name}: max|oracle - exact| {out['noise_' + name]:.2e} at scale {np.max(np.abs(a)):.2e}", flush=True)
    path = os.path.join(HERE, "general_long.npz")
    np.savez_compressed(path, **out)
    print(f"wrote general_long.npz ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
