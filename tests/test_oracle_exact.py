"""The extended-precision evaluator (oracle/grape_exact.py) against the double oracle and the
reference's known answer (CPU).  grape_exact restates the same formulas as oracle/grape_oracle.py
(UnitaryCalculations.jl:44-151, FidelityCalculations.jl:19-119) in longdouble, so the two agree to
the oracle's own rounding noise: F to 1e-14, the eps forward differences to ~u / eps of their
scale, the eps2 mixed stencils to ~u / eps2^2."""
import numpy as np

from tests import problems as P


def test_exact_matches_oracle_within_its_noise():
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    for fp, nt in ((P.sym_problem(12), 12), (P.full9_problem(20), 20)):
        x = P.random_x(nt, 31)
        F, g = E.fidelity_and_gradient(fp, x)
        F0, g0 = O.calculate_fidelity_and_derivatives(fp, x)[:2]
        assert abs(F - F0) < 1e-14
        assert np.max(np.abs(g - g0)) < 1e-6 * np.max(np.abs(g0)) + 1e-9
        # the error-free form of the general evaluator: the same computation, products grouped differently
        Fa, ga, d2, d2dx = E.fidelity_and_derivatives(fp, x)
        assert abs(Fa - F) < 1e-16 and np.max(np.abs(ga - g)) < 1e-15 * np.max(np.abs(g)) and d2.shape == (0,)


def test_exact_error_path_matches_oracle_within_its_noise():
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    fp = P.sym_problem(8, errors=("amp", "freq"))
    x = P.random_x(8, 5)
    ex = E.fidelity_and_derivatives(fp, x)
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    assert abs(ex[0] - ref[0]) < 1e-14
    assert np.max(np.abs(ex[1] - ref[1])) < 1e-6 * np.max(np.abs(ref[1])) + 1e-9
    assert np.max(np.abs(ex[2] - ref[2])) < 1e-6 * np.max(np.abs(ref[2])) + 1e-9
    assert np.max(np.abs(ex[3] - ref[3])) < 1e-4 * np.max(np.abs(ref[3])) + 1e-6


def test_exact_reproduces_the_evered_known_answer():
    """runtests.jl:115-165: F > 0.9999 for the published time-optimal pulse (the restatement value
    0.999996184760959)."""
    from oracle import grape_exact as E
    F, g = E.fidelity_and_gradient(P.sym_problem(1000), P.evered_pulse(1000))
    assert F > 0.9999 and abs(F - 0.999996184760959) < 1e-12


def test_sensitivities_and_xadd_are_the_full_evaluators_rows():
    """grape_exact.sensitivities_and_xadd (only the nominal and eps error propagators) returns
    fidelity_and_derivatives' own F, F_d2err and x_add rows of F_d2err_dx (tests/xadd_pin.py uses it)."""
    import numpy as np
    from oracle import grape_exact as E
    from tests import problems as P
    for fp, x in ((P.sym_problem(7, errors=("amp", "freq")), P.random_x(7, 11)),
                  (P.full9_problem(5, nerr=4), P.random_x(5, 12, small=True))):
        F, _, d2, d2dx = E.fidelity_and_derivatives(fp, x)
        F1, d21, add = E.sensitivities_and_xadd(fp, x)
        assert F1 == F and np.array_equal(d21, d2) and np.array_equal(add, d2dx[len(x) - 1:])
    import pytest
    with pytest.raises(ValueError):
        E.sensitivities_and_xadd(P.xadd_err_problem(5, 3), P.xadd_x(3, 1))


def test_exact_refuses_a_non_hermitian_h0():
    """grape_exact takes C_k^-1 = C_k^dagger.  Given a -i Gamma / 2 decay term it used to return an "exact"
    F_dx 4.7e-4 from the oracle on a scale of 0.037 and an F_d2err 85 % off, without complaint (N_t = 300,
    gamma = 0.4 on levels 3 and 4): it refuses such an H0 now, in every evaluator."""
    import pytest
    from oracle import grape_exact as E
    fp = P.with_decay(P.sym_problem(300, errors=("amp", "freq")), 0.4, (3, 4))
    x = P.random_x(300, 41)
    with pytest.raises(ValueError, match="Hermitian"):
        E.fidelity_and_derivatives(fp, x)
    with pytest.raises(ValueError, match="Hermitian"):
        E.sensitivities_and_xadd(fp, x)
    for device in (True, False):  # operator basis (longdouble coefficients) and closure (double)
        with pytest.raises(ValueError, match="Hermitian"):
            E.fidelity_and_gradient(P.with_decay(P.sym_problem(300, device=device), 0.4, (3, 4), device), x)
    # a non-Hermitian error generator over a Hermitian H0 leaves the chain unitary but not H0 + Herror
    from robustgrape_amd.operators import OperatorBasisError, Term
    from robustgrape_amd.types import ErrorSource
    base = P.sym_problem(6)
    decay = np.diag([0.0, 0.0, 0.0, 1.0, 1.0]).astype(complex)
    errs = (ErrorSource(OperatorBasisError([Term(decay, scale=-0.5j)])),)
    with pytest.raises(ValueError, match="Herror_0"):
        E.fidelity_and_derivatives(base.replace(unitary_problem=base.unitary_problem.replace(error_sources=errs)),
                                   P.random_x(6, 42))


def test_exact_accepts_a_hermitian_sum_of_non_hermitian_terms():
    """Complex-coefficient split terms (each term non-Hermitian, the sum e^{i alpha} U + h.c. Hermitian) stay
    in scope: the guard looks at the step's H0, not at its terms."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd import synthetic as S
    from tests.test_gpu_dense import _split_terms_problem
    d, nt = 13, 3
    fp = _split_terms_problem(d, nt)
    x = S.dense_x(nt, seed=803)
    F, g = E.fidelity_and_gradient(fp, x, nparam=2)
    F0, g0 = O.calculate_fidelity_and_derivatives(fp, x)[:2]
    # the oracle's forward difference of quantities of order 1 carries u / eps = 2.2e-8 of rounding (it sits
    # 3e-9 from exact here, on this problem and on the unsplit one alike)
    assert abs(F - F0) < 1e-14 and np.max(np.abs(g - g0)) < 1e-6 * np.max(np.abs(g0)) + 2.2e-8
