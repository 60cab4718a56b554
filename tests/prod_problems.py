"""Problem builders of the product-coefficient tests (tests/test_prod_cpu.py, tests/test_gpu_prod.py):
operator bases whose terms carry Factors (include/grape.h GRAPE_OP_FACTOR) -- amplitude x phase drives,
a control entering twice, a global scale on x_add, a step-index envelope.

Every builder returns the operator-basis problem.  The CPU oracle calls such an object as a closure and
sees the factors; oracle/grape_exact.py reads `.terms` and knows nothing of factors, so it is always
handed `closures(fp)`, never the operator-basis object."""
from __future__ import annotations

import math

import numpy as np

from robustgrape_amd import rydberg as R
from robustgrape_amd.operators import (FN_CIS, FN_COS, FN_SIN, VAR_TSTEP, VAR_X, VAR_XADD, Factor,
                                       OperatorBasisHamiltonian, OperatorBasisTarget, Term)
from robustgrape_amd.types import ErrorSource, FidelityRobustGRAPEProblem, UnitaryRobustGRAPEProblem
from tests import problems as P

NPARAM = 2  # x[0, k] the amplitude Omega_k, x[1, k] the phase phi_k


def closures(fp):
    """The closure form for oracle/grape_exact.py and the closure-table path."""
    return P.as_closures(fp)


def prod_x(ntimes, seed, nadd=1):
    """Amplitudes 0.5 + U[0, 1), phases 2 pi U, x_add = 2 pi U: x[p + k * 2] = control p at step k."""
    rng = np.random.default_rng(seed)
    xm = np.empty((ntimes, NPARAM))
    xm[:, 0] = 0.5 + rng.uniform(size=ntimes)
    xm[:, 1] = 2 * math.pi * rng.uniform(size=ntimes)
    return np.concatenate([xm.ravel(), 2 * math.pi * rng.uniform(size=nadd)])


def sym_problem(ntimes, t0=3.0, errors=()):
    """d = 5 symmetric blockaded CZ driven by Omega_k (cos phi_k Hc + sin phi_k Hs); errors: subset of
    {'amp', 'freq'}, 'amp' the relative amplitude error of the shaped drive (a product as well)."""
    H0 = R.rydberg_symmetric_blockaded_operator_basis(param=1, amplitude_param=0)
    errs = [ErrorSource(R.symmetric_amplitude_error(param=1, amplitude_param=0) if e == "amp"
                        else R.symmetric_frequency_error()) for e in errors]
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=5, H0=H0, nb_additional_param=1, error_sources=errs)
    return FidelityRobustGRAPEProblem(up, P.W_SYM, R.cz_symmetric_target())


def full9_problem(ntimes, t0=3.0, B=10.0):
    """d = 9 rydberg_hamiltonian_full with both Rabi frequencies scaled by the amplitude control."""
    H0 = R.rydberg_full_operator_basis(1.0, 1.0, 0.0, 0.0, B, param=1, amplitude_param=0)
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=9, H0=H0, nb_additional_param=1)
    return FidelityRobustGRAPEProblem(up, P.W_FULL9, R.cz_full_target())


def _hermitian(d, rng):
    A = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    A = (A + A.conj().T) / 2
    return A / np.abs(A).sum(axis=0).max()  # |A|_1 = 1


def _phase_target(d, rng):
    """Q (I - e_0 e_0^T) + cis(x_add[0]) Q e_0 e_0^T for a random unitary Q."""
    Q, _ = np.linalg.qr(rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    P0 = np.zeros((d, d))
    P0[0, 0] = 1.0
    return OperatorBasisTarget([Term(Q @ (np.eye(d) - P0)), Term(Q @ P0, var=VAR_XADD, index=0, func=FN_CIS)])


def many_terms_problem(ntimes=3, t0=3.0, nterms=8, d=4):
    """More operator terms than the builders cache (kCachedTerms = 6): `nterms` random Hermitian operators,
    |H_i|_1 = 1, each with a factor: 0.6 x0 cos(x1 + i) H_i for even i, 0.3 x0 sin(0.7 x1 - i) H_i for odd i
    (a strong pulse: the oracle's u / eps noise stays well inside the F_dx tier)."""
    rng = np.random.default_rng(97)
    terms = []
    for i in range(nterms):
        fac = (Factor(VAR_X, 0, scale=0.6 if i % 2 == 0 else 0.3),)
        terms.append(Term(_hermitian(d, rng), var=VAR_X, index=1, func=FN_COS if i % 2 == 0 else FN_SIN,
                          a=1.0 if i % 2 == 0 else 0.7, b=float(i if i % 2 == 0 else -i), factors=fac))
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=d, H0=OperatorBasisHamiltonian(terms),
                                   nb_additional_param=1)
    return FidelityRobustGRAPEProblem(up, np.diag([1.0, 1.0, 0.5, 0.0]), _phase_target(d, rng))


def twice_problem(ntimes=9, t0=1.8, d=4):
    """Both scalars on one control, x0 cos(x0) H_0, and a term with two factors that reads x_add,
    x_add[1] x0 cos(x1) H_1, plus a plain sin(x1) H_2: nadd = 2 (x_add[0] the target's phase)."""
    rng = np.random.default_rng(98)
    H = [_hermitian(d, rng) for _ in range(3)]
    terms = [Term(H[0], var=VAR_X, index=0, func=FN_COS, scale=0.6, factors=(Factor(VAR_X, 0),)),
             Term(H[1], var=VAR_X, index=1, func=FN_COS, scale=0.5,
                  factors=(Factor(VAR_XADD, 1), Factor(VAR_X, 0))),
             Term(H[2], var=VAR_X, index=1, func=FN_SIN, scale=0.4)]
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=d, H0=OperatorBasisHamiltonian(terms),
                                   nb_additional_param=2)
    return FidelityRobustGRAPEProblem(up, np.diag([1.0, 1.0, 0.5, 0.0]), _phase_target(d, rng))


def twice_x(ntimes, seed):
    """prod_x with x_add = (2 pi U, 0.5 + U): the second entry is the global scale of twice_problem."""
    x = prod_x(ntimes, seed, nadd=2)
    x[-1] = 0.5 + np.random.default_rng(seed + 1000).uniform()
    return x


def envelope_problem(ntimes=11, t0=5.0):
    """A step-index factor: sin(pi (k - 1/2) / N_t) x0 (cos x1 Hc + sin x1 Hs) on the d = 5 model."""
    base = R.rydberg_symmetric_blockaded_operator_basis(param=1, amplitude_param=0)
    env = Factor(VAR_TSTEP, 0, FN_SIN, a=math.pi / ntimes, b=-0.5 * math.pi / ntimes)
    terms = [Term(op=t.op, var=t.var, index=t.index, func=t.func, a=t.a, b=t.b, scale=t.scale,
                  factors=(env,) + t.factors) for t in base.terms]
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=5, H0=OperatorBasisHamiltonian(terms),
                                   nb_additional_param=1)
    return FidelityRobustGRAPEProblem(up, P.W_SYM, R.cz_symmetric_target())


def wide_problem(d, ntimes=4):
    """A product problem at d levels for the refusals above GRAPE_MAX_SMALL_DIM (never evaluated)."""
    rng = np.random.default_rng(d)
    terms = [Term(_hermitian(d, rng), var=VAR_X, index=1, func=FN_COS, factors=(Factor(VAR_X, 0),)),
             Term(_hermitian(d, rng), var=VAR_X, index=1, func=FN_SIN, factors=(Factor(VAR_X, 0),))]
    up = UnitaryRobustGRAPEProblem(t0=1.0, ntimes=ntimes, ndim=d, H0=OperatorBasisHamiltonian(terms),
                                   nb_additional_param=1)
    W = np.zeros(d)
    W[:4] = 1.0
    return FidelityRobustGRAPEProblem(up, np.diag(W), OperatorBasisTarget([Term(np.eye(d, dtype=np.complex128))]))

