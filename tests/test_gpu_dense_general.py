"""Non-Hermitian generators at 13..64 levels: the dense engine's pivoted exponential
(grape_dense.hpp gj_solve_pivot, k_dexp<true> / k_dexp_raw<true>) and the general path over it
(GRAPE_OPT_GENERAL_H0 above 12 levels), against the CPU oracle.

Tolerances:
  exp(A)       the tiers of tests/test_gpu_dense.py: relative max-entry error <= 1e-13 max(1, |A|_1),
               1e-12 max(1, |A|_1) where the device takes Pade 13 (m from the unbalanced 1-norm).
  F            1e-12 absolute
  F_dx         tests/problems.py fd_tier (nparam = 2), plus the oracle-to-C++-port spread where the
               port is built, capped at the tier itself (tests/test_gpu_dense.py _cpu_spread)
  F_d2err      1e-6 fd_factor max|ref| + 1e-7
  F_d2err_dx   1e-5 fd_factor max|ref| + 1e-7
"""
import functools

import numpy as np
import pytest

from robustgrape_amd import synthetic as S
from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
T2, T2_ABS = 1e-6, 1e-7
T3, T3_ABS = 1e-5, 1e-7
NORMS = (0.2, 0.9, 1.5, 4.0, 30.0)  # Taylor, Taylor, Pade 9, Pade 13 (s = 0), Pade 13 (s = 3)
HIST = {3: 0, 5: 1, 7: 2, 9: 3, 13: 4}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _norm1(A):
    return float(np.abs(A).sum(axis=0).max())


def _expm(A, general=True):
    """exp of a stack of row-major matrices through the C ABI; returns (E, stats)."""
    from robustgrape_amd import _capi
    d = A.shape[-1]
    Acm = np.ascontiguousarray(A.transpose(0, 2, 1))  # column-major per matrix
    E = np.empty_like(Acm)
    stats = (_capi.ctypes.c_int * 5)()
    fn = _capi.lib().grape_expm_batch_general if general else _capi.lib().grape_expm_batch
    _capi.check(fn(0, d, len(A), _capi.dptr(Acm), _capi.dptr(E), stats))
    return E.transpose(0, 2, 1), list(stats)


def _device_m(A):
    from oracle import grape_oracle as O
    return O.pade_degree(_norm1(A))[0]


def _tol(A):
    return (1e-12 if _device_m(A) == 13 else 1e-13) * max(1.0, _norm1(A))


def _expect_stats(As):
    expect = [0] * 5
    for a in As:
        expect[HIST[_device_m(a)]] += 1
    return expect


def _family(kind, d, norm, rng):
    G = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    if kind == "decay":  # skew-Hermitian plus a negative real diagonal on ~30 % of the levels
        A = -1j * (G + G.conj().T) / 2
        lv = rng.choice(d, size=max(1, int(round(0.3 * d))), replace=False)
        A[lv, lv] -= rng.uniform(0.5, 2.0, size=len(lv)) * np.sqrt(d)
    else:  # Ginibre: no symmetry
        A = G
    return A / _norm1(A) * norm


@pytest.mark.parametrize("kind", ["decay", "ginibre"])
@pytest.mark.parametrize("d", [13, 34, 64])
def test_general_expm_matches_oracle(d, kind):
    from oracle import grape_oracle as O
    from tests.parity_log import record
    rng = np.random.default_rng(2000 + d + (0 if kind == "decay" else 100))
    A = np.stack([_family(kind, d, nm, rng) for nm in NORMS])
    E, stats = _expm(A)
    for j, nm in enumerate(NORMS):
        ref = O.julia_exp(A[j])
        rel = float(np.max(np.abs(E[j] - ref)) / np.max(np.abs(ref)))
        tol = _tol(A[j])
        record(f"general_expm_{kind}_d{d}_n{nm}", "exp", rel, 1.0, tol)
        print(f"general_expm {kind} d={d} |A|_1={nm}: rel {rel:.2e} tol {tol:.1e}")
        assert rel <= tol, (kind, d, nm, rel, tol)
    assert stats == _expect_stats(A)


def _interchange(d, ginibre=0.0):
    """A[i, i+h] = 4.9 e^{i phi_i}, A[i+h, i] = -(pi^2 / 4.9) e^{-i phi_i}: A^2 = -pi^2 I on each pair, so
    the even part of Pade 13 vanishes there, diag(V - U) ~ 1e-15 c0 and the pivot of column i is row
    i + h (another 16-row tile at d = 34, 64): an elimination without interchanges is wrong by 0.13-0.28."""
    rng = np.random.default_rng(3000 + d)
    h = d // 2
    A = np.zeros((d, d), complex)
    phi = rng.uniform(0, 2 * np.pi, size=h)
    for i in range(h):
        A[i, i + h] = 4.9 * np.exp(1j * phi[i])
        A[i + h, i] = -(np.pi ** 2 / 4.9) * np.exp(-1j * phi[i])
    if ginibre:
        A = A + ginibre / d * (rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d)))
    return A


@pytest.mark.parametrize("ginibre", [0.0, 0.01])
@pytest.mark.parametrize("d", [13, 34, 64])
def test_general_expm_needs_row_interchanges(d, ginibre):
    from oracle import grape_oracle as O
    from tests.parity_log import record
    A = _interchange(d, ginibre)
    assert _device_m(A) == 13
    ref = O.julia_exp(A)
    E, stats = _expm(A[None])
    rel = float(np.max(np.abs(E[0] - ref)) / np.max(np.abs(ref)))
    tol = 1e-12 * _norm1(A)
    record(f"general_expm_interchange_d{d}_g{ginibre}", "exp", rel, 1.0, tol)
    print(f"interchange d={d} ginibre={ginibre}: rel {rel:.2e} tol {tol:.1e}")
    assert rel <= tol, (d, ginibre, rel, tol)
    assert stats == [0, 0, 0, 0, 1]


def _skew_hermitian(d, norm, rng):  # the inputs of tests/test_gpu_dense.py's exponential test
    H = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    H = (H + H.conj().T) / 2
    return -1j * H / np.abs(H).sum(axis=0).max() * norm


@pytest.mark.parametrize("d", [13, 24, 64])
def test_general_expm_agrees_with_the_hermitian_kernel(d):
    from tests.parity_log import record
    rng = np.random.default_rng(1000 + d)
    norms = (0.01, 0.04, 0.2, 0.6, 0.8, 0.9, 1.5, 4.0, 30.0)
    A = np.stack([_skew_hermitian(d, nm, rng) for nm in norms])
    Eg, sg = _expm(A, general=True)
    Eh, sh = _expm(A, general=False)
    for j, nm in enumerate(norms):
        rel = float(np.max(np.abs(Eg[j] - Eh[j])) / np.max(np.abs(Eh[j])))
        tol = _tol(A[j])
        record(f"general_vs_hermitian_expm_d{d}_n{nm}", "exp", rel, 1.0, tol)
        assert rel <= tol, (d, nm, rel, tol)
    assert sg == sh == _expect_stats(A)


# ---------------------------------------------------------------------------------------------
# plans
# ---------------------------------------------------------------------------------------------
def _base(d, nt, nerr, phase, scale):
    if nerr == 0 and not phase:
        return S.dense_problem(d, nt, rank=min(16, d - 3), scale=scale)
    return S.dense_error_problem(d, nt, rank=min(16, d - 3), scale=scale, nerr=nerr, phase=phase)


def _decay(d, nt, nerr, phase, scale, device):
    return P.with_decay(_base(d, nt, nerr, phase, scale), 0.4, (1, d // 2, d - 1), device)


def _x(nt, phase, seed):
    x = S.dense_x(nt, seed=seed)
    return np.concatenate([x, [0.7]]) if phase else x


@functools.lru_cache(maxsize=None)
def _oracle(d, nt, nerr, phase, scale):
    """(x, reference outputs, F without the decay) of one decay case, evaluated once."""
    from oracle import grape_oracle as O
    x = _x(nt, phase, 800 + nt)
    ref = O.calculate_fidelity_and_derivatives(_decay(d, nt, nerr, phase, scale, False), x)
    F_plain = O.calculate_fidelity_and_derivatives(_base(d, nt, nerr, phase, scale), x)[0]
    return x, ref, F_plain


def _spread(fp, x, ref_Fdx):
    """The checker's own noise: oracle against the C++ port, 0 when the port is not built."""
    try:
        from oracle.cref import cref
        if not cref.available():
            return 0.0
        return float(np.max(np.abs(np.asarray(cref.fidelity_grad(fp, x)[1]) - np.asarray(ref_Fdx))))
    except Exception:
        return 0.0


def _check(got, ref, label, ne, fp, x, spread=0.0):
    from tests.parity_log import record
    f = P.fd_factor(fp, x, nparam=2)
    t, ta = P.fd_tier(fp, x, nparam=2)
    eF = float(np.max(np.abs(np.asarray(got[0]) - ref[0])))
    record(label, "F", eF, 1.0, T1)
    print(label, "F", f"{eF:.2e}")
    assert eF <= T1, (label, eF)
    tiers = [("F_dx", t, ta), ("F_d2err", T2 * f, T2_ABS), ("F_d2err_dx", T3 * f, T3_ABS)]
    for n, (name, rel, ab) in enumerate(tiers, start=1):
        if n > 1 and ne == 0:
            break
        a, b = np.asarray(got[n]), np.asarray(ref[n])
        err, scale = float(np.max(np.abs(a - b))), float(np.max(np.abs(b)))
        tol = rel * scale + ab
        if n == 1:
            tol += min(spread, tol)
        record(label, name, err, scale, tol)
        print(label, name, f"err {err:.2e} scale {scale:.2e} tol {tol:.2e}")
        assert err <= tol, (label, name, err, scale, tol)


CASES = [(13, 1, 0, False, 2.0), (16, 5, 2, True, 1.0), (27, 9, 1, False, 2.0), (40, 4, 2, False, 4.0),
         (64, 3, 0, False, 12.0)]


@pytest.mark.parametrize("d,nt,nerr,phase,scale", CASES)
def test_decay_plans_match_live_oracle(d, nt, nerr, phase, scale):
    """The public function with no option: the default plan is refused (UNSUPPORTED) and served by
    the general path with the pivoted exponential."""
    from robustgrape_amd import calculate_fidelity_and_derivatives
    x, ref, F_plain = _oracle(d, nt, nerr, phase, scale)
    fpo = _decay(d, nt, nerr, phase, scale, False)
    if scale >= 8.0:
        assert P.max_step_norm(fpo, x, 2) > 5.4  # reaches a squaring
    assert abs(ref[0] - F_plain) > 1e-4  # the decay is visible
    got = calculate_fidelity_and_derivatives(_decay(d, nt, nerr, phase, scale, True), x)
    _check(got, ref, f"dense_general_d{d}_nt{nt}_ne{nerr}", nerr, fpo, x, _spread(fpo, x, ref[1]))


def test_non_hermitian_error_generator_with_hermitian_h0():
    """The problem tests/test_gpu_dense.py sees refused by default, served with the option."""
    from oracle import grape_oracle as O
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0, OperatorBasisError, Term
    from robustgrape_amd.types import ErrorSource
    fp0 = S.dense_problem(20, 4)
    decay = np.diag([0.0] * 19 + [1.0]).astype(complex)
    errs = (ErrorSource(OperatorBasisError([Term(decay, scale=-0.5j)])),)
    fp = fp0.replace(unitary_problem=fp0.unitary_problem.replace(error_sources=errs))
    x = S.dense_x(4, seed=811)
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    plan = GrapePlan(fp, nparam=2, max_batch=1, options=OPT_GENERAL_H0)
    try:
        F, Fdx, Fd2, Fd2dx = plan.fidelity_grad(x[None, :])
    finally:
        plan.close()
    _check((F[0], Fdx[0], Fd2[0], Fd2dx[0]), ref, "dense_general_nonherm_error", 1, fp, x)


def test_decay_closures_above_12_levels():
    from robustgrape_amd import calculate_fidelity_and_derivatives
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    case = CASES[1]
    x, ref, _ = _oracle(*case)
    fpo = _decay(*case, False)
    fpc = P.as_closures(_decay(*case, True))
    plan = GrapePlan(fpc, nparam=2, max_batch=1, options=OPT_GENERAL_H0)
    try:
        assert plan.tables
        F, Fdx, Fd2, Fd2dx = plan.fidelity_grad(x[None, :])
    finally:
        plan.close()
    _check((F[0], Fdx[0], Fd2[0], Fd2dx[0]), ref, "dense_general_closures_plan", 2, fpo, x)
    got = calculate_fidelity_and_derivatives(fpc, x)
    _check(got, ref, "dense_general_closures_public", 2, fpo, x)


def test_decay_unitary_derivatives_and_interaction_operators_above_12_levels():
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_interaction_error_operators, calculate_unitary_and_derivatives
    d, nt = 16, 5
    x = _x(nt, False, 830)
    upo = _decay(d, nt, 2, False, 1.0, False).unitary_problem
    upd = _decay(d, nt, 2, False, 1.0, True).unitary_problem
    ref = O.calculate_unitary_and_derivatives(upo, x)
    got = calculate_unitary_and_derivatives(upd, x)
    assert np.max(np.abs(got[0] - ref[0])) <= T1
    assert abs(abs(np.linalg.det(ref[0])) - 1.0) > 1e-3  # not unitary
    fac = P.tensor_factor(_decay(d, nt, 2, False, 1.0, False), x, nparam=2)
    for n, (tol, atol) in ((1, (T2 * fac, T2_ABS)), (2, (T2 * fac, T2_ABS)), (3, (T2 * fac, T2_ABS)),
                           (4, (T3 * fac, T3_ABS)), (5, (T3 * fac, T3_ABS))):
        a, b = np.asarray(got[n]), np.asarray(ref[n])
        assert a.shape == b.shape, (n, a.shape, b.shape)
        if b.size:
            assert np.max(np.abs(a - b)) <= tol * np.max(np.abs(b)) + atol, (n, np.max(np.abs(a - b)))
    Oref = O.calculate_interaction_error_operators(upo, x)
    Og = calculate_interaction_error_operators(upd, x)
    assert np.max(np.abs(Og - Oref)) <= 1e-7 * np.max(np.abs(Oref))


def test_decay_batches_are_single_calls_above_12_levels():
    """A batch is the single evaluations, bit for bit; ragged chunks of the plan."""
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    nt = 6
    fp = P.with_decay(S.dense_problem(20, nt), 0.4, (1, 10, 19))
    X = np.stack([S.dense_x(nt, seed=840 + s) for s in range(5)])
    plan = GrapePlan(fp, nparam=2, max_batch=2, options=OPT_GENERAL_H0)
    try:
        F, Fdx, _, _ = plan.fidelity_grad(X)
        for b in range(5):
            Fs, gs, _, _ = plan.fidelity_grad(X[b:b + 1])
            assert Fs[0] == F[b] and np.array_equal(gs[0], Fdx[b])
    finally:
        plan.close()


def test_general_option_on_a_hermitian_dense_problem_matches_the_fused_path():
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    nt = 7
    fp = S.dense_error_problem(24, nt)
    X = np.stack([S.dense_x(nt, seed=850 + s) for s in range(2)])
    outs = []
    for opts in (0, OPT_GENERAL_H0):
        plan = GrapePlan(fp, nparam=2, max_batch=2, options=opts)
        try:
            outs.append(plan.fidelity_grad(X))
        finally:
            plan.close()
    for b in range(len(X)):
        _check(tuple(o[b] for o in outs[1]), tuple(o[b] for o in outs[0]), f"dense_general_vs_fused_{b}", 2, fp, X[b])
