"""The materialised-derivative kernels (robustgrape_amd/csrc/grape_unitary.hip) where a workgroup takes more
than one item: above 12 levels the launches are capped at kResident = 256 workgroups striding over the items
with their tiles in global scratch, and k_u_fid_contract caps its grid at 16 384 waves at every size.  Every
other test of these kernels stays below both counts, so its loops run once.  The cases (and the item counts
they reach) are in tests/unitary_wrap_cases.py; tests/test_unitary_wrap_cases_cpu.py checks the counts.

References: oracle/grape_oracle.py evaluated live (under 2 s each), except the 5500-step case, whose longdouble
reference (oracle/grape_exact.py) is the fixture tests/golden/general_long.npz.

Tolerances (the tiers of the neighbouring files):
  U                      1e-12 max(1, max|ref|)
  U_dx, U_dx_add, U_derr 1e-6 max(1, max|ref|);  U_derr_dx, U_derr_dx_add 1e-5 max(1, max|ref|)
                         (tests/test_gpu_dense.py test_dense_unitary_derivatives_match_oracle; general H0:
                         tests/problems.py tensor_factor, as tests/test_gpu_dense_general.py)
  interaction operators, expectation values, fidelity response   1e-6 max|ref| + 1e-7
  F, F_dx, F_d2err, F_d2err_dx   tests/test_gpu_dense_general.py _check (1e-12; fd_tier; 1e-6 / 1e-5 fd_factor
                         max|ref| + 1e-7; the oracle-to-C++-port spread on F_dx where the port is built)
"""
import functools
import os

import numpy as np
import pytest

from tests import problems as P
from tests import unitary_wrap_cases as W

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T1 = 1e-12
T2, T2_ABS = 1e-6, 1e-7
T3, T3_ABS = 1e-5, 1e-7
TENSORS = ["U", "U_dx", "U_dx_add", "U_derr", "U_derr_dx", "U_derr_dx_add"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _close(got, ref, label, name, rel=T2, ab=T2_ABS):
    from tests.parity_log import record
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (label, name, got.shape, ref.shape)
    err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
    tol = rel * scale + ab
    record(label, name, err, scale, tol)
    print(f"{label} {name}: err {err:.2e} scale {scale:.2e} tol {tol:.2e}")
    assert err <= tol, (label, name, err, scale, tol)


def _assert_tensors(out, ref, label, factor=1.0):
    """The six outputs of calculate_unitary_and_derivatives at 1e-12, T2, T2, T2, T3, T3, each times
    max(1, max|ref|) (tests/test_gpu_dense.py); factor: tests/problems.py tensor_factor for a general H0."""
    from tests.parity_log import record
    for name, a, r, t in zip(TENSORS, out, ref, [T1, T2 * factor, T2 * factor, T2 * factor, T3 * factor, T3 * factor]):
        assert a.shape == r.shape, name
        if r.size == 0:
            continue
        err, scale = float(np.max(np.abs(a - r))), float(np.max(np.abs(r)))
        tol = t * max(1.0, scale)
        record(label, name, err, scale, tol)
        print(f"{label} {name}: err {err:.2e} scale {scale:.2e} tol {tol:.2e}")
        assert err <= tol, (label, name, err, scale)


# ---------------------------------------------------------------- materialised tensors, Hermitian H0
@pytest.mark.parametrize("d,nt,nerr,phase", list(W.TENSOR_CASES))
def test_unitary_derivatives_match_oracle_past_the_resident_grid(d, nt, nerr, phase):
    """calculate_unitary_and_derivatives at 280 / 528 / 260 k_u_vmats items and 280 / 288 / 260 k_u_assemble
    items (256 workgroups: the scratch tiles are reused from one item to the next, k_u_assemble's `continue`
    branch is followed by another item, its sU tile outlives the first); the (16, 48) case runs k_u_reduce over
    five outputs; (64, 6, 2 errors, phase) is d = 64 with error sources and an additional parameter."""
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_unitary_and_derivatives
    up, x = W.tensor_case(d, nt, nerr, phase)
    ref = O.calculate_unitary_and_derivatives(up, x)
    out = calculate_unitary_and_derivatives(up, x)
    _assert_tensors(out, ref, f"wrap_tensors_d{d}_nt{nt}_ne{nerr}")


# ---------------------------------------------------------------- analysis entry points
FREQS = np.linspace(0.0, 1.0, 3)


@functools.lru_cache(maxsize=None)
def _analysis_ref():
    from oracle import grape_oracle as O
    fp, x = W.analysis_problem(), W.analysis_x()
    return (O.calculate_interaction_error_operators(fp.unitary_problem, x), O.calculate_expectation_values(fp, x),
            O.calculate_fidelity_response(fp, x, FREQS))


@pytest.mark.parametrize("closures", [False, True], ids=["operator-basis", "closures"])
def test_analysis_entry_points_match_oracle_past_the_resident_grid(closures):
    """280 items of k_u_interaction (operator basis) / k_u_interaction_table (closures): the (k, e) decoding of
    a second item, and k_u_expect with a general projector at d = 20."""
    from robustgrape_amd import analysis as A
    fp, x = W.analysis_problem(), W.analysis_x()
    if closures:
        fp = P.as_closures(fp)
    Oref, ev0, r0 = _analysis_ref()
    label = "wrap_analysis_" + ("closures" if closures else "basis")
    _close(A.calculate_interaction_error_operators(fp.unitary_problem, x), Oref, label, "O")
    _close(A.calculate_expectation_values(fp, x), ev0, label, "expectation")
    _close(A.calculate_fidelity_response(fp, x, FREQS), r0, label, "response")


def _check_fidelity(got, ref, label, ne, fp, x):
    from tests.test_gpu_dense_general import _check, _spread
    _check(got, ref, label, ne, fp, x, _spread(fp, x, ref[1]))


def test_decay_analysis_and_fidelity_match_oracle_with_260_inverses():
    """Non-Hermitian H0 at d = 13, N_t = 260: k_u_inverse strides (its pivot state is per item), and
    k_u_interaction reads C_k^-1 from it; the fidelity of the same problem takes the general path with 1300
    k_u_vmats and 1040 k_u_assemble items."""
    from oracle import grape_oracle as O
    from robustgrape_amd import analysis as A
    from robustgrape_amd import calculate_fidelity_and_derivatives
    fp, x = W.decay_problem(), W.decay_x()
    up = fp.unitary_problem
    _close(A.calculate_interaction_error_operators(up, x), O.calculate_interaction_error_operators(up, x),
           "wrap_decay", "O")
    _close(A.calculate_expectation_values(fp, x), O.calculate_expectation_values(fp, x), "wrap_decay", "expectation")
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    F_plain = O.calculate_fidelity_and_derivatives(W.decay_problem(decay=False), x)[0]
    assert abs(ref[0] - F_plain) > 1e-4, (ref[0], F_plain)  # the decay is visible
    _check_fidelity(calculate_fidelity_and_derivatives(fp, x), ref, "wrap_decay_fidelity", 1, fp, x)


# ---------------------------------------------------------------- general-H0 fidelity, every kernel wrapping
def test_general_fidelity_matches_oracle_with_four_items_per_workgroup():
    """d = 13, N_t = 90, two error sources, an additional parameter, decay: 990 k_u_vmats items and 540
    k_u_assemble items through enqueue_general.  Then a batch of two different x on one plan of two equals
    the two single calls on it bit for bit: the single-evaluation workspace is reused after a wrapped pass."""
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_fidelity_and_derivatives
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    fp, x = W.general_problem(), W.general_x()
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    _check_fidelity(calculate_fidelity_and_derivatives(fp, x), ref, "wrap_general", 2, fp, x)
    X = np.stack([x, W.general_x(seed=1991)])
    assert np.max(np.abs(X[0] - X[1])) > 0.1
    plan = GrapePlan(fp, nparam=W.NP, max_batch=2, options=OPT_GENERAL_H0)
    try:
        batch = plan.fidelity_grad(X)
        singles = [plan.fidelity_grad(X[b:b + 1]) for b in range(2)]
    finally:
        plan.close()
    for b in range(2):
        for a, s in zip(batch, singles[b]):
            assert np.array_equal(a[b], s[0])
    _check_fidelity(tuple(a[0] for a in batch), ref, "wrap_general_plan", 2, fp, x)
    assert abs(batch[0][0] - batch[0][1]) > 1e-6  # two evaluations, not one twice


# ---------------------------------------------------------------- k_u_fid_contract past 4096 x 4 waves
def test_fid_contract_past_its_grid_cap_matches_the_longdouble_reference():
    """The d = 5 symmetric problem with both error sources at N_t = 5500 on the general path (forced on a
    Hermitian H0, as tests/test_gpu_general_h0.py does): 16 500 items for k_u_fid_contract's 16 384 waves, so
    the second error source's rows at steps k >= 5384 are written by a wave's second trip.  They are asserted
    on their own as well as with the whole arrays.

    Reference: the longdouble evaluation (tests/golden/general_long.npz), not the double oracle, which at this
    length is itself further from it than the bare T2 / T3 tiers allow.  Bound per output: the tier of
    tests/test_gpu_general_h0.py (1e-12; fd_tier; 1e-6 max|ref| + 1e-7; 1e-5 max|ref| + 1e-7) plus
    LONG_NOISE_MULTIPLE times the recorded max|oracle - exact| of that output -- a second correct double
    implementation sits about as far from exact as the oracle does.  Every bound is below 1e-2 of the output's
    scale (asserted): a skipped or stale item is off by about the scale.

    Measured on an MI355X (max|device - exact|; the oracle's own max|oracle - exact|; scale; bare tier):
        F            1.8e-14    3.5e-13    0.59      1.0e-12
        F_dx         9.1e-10    9.1e-10    7.6e-2    8.6e-9    (both at the x_add entry: the target's difference)
        F_d2err      4.6e-9     7.8e-9     1.5e-2    1.1e-7
        F_d2err_dx   3.8e-8     5.5e-9     1.8e-3    1.2e-7
        its tail     2.8e-11               3.6e-5    (rows k >= 5384 of the second error source)
    With this pulse the device is inside the bare tier in every output (by 3x in F_d2err_dx, the closest), so the
    smallest multiple that leaves headroom is taken: LONG_NOISE_MULTIPLE = 1, the checker's noise counted once.
    """
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    from tests.parity_log import record
    g = dict(np.load(os.path.join(GOLDEN, "general_long.npz"), allow_pickle=False))
    fp, x = W.long_problem(), W.long_x()
    assert np.array_equal(g["x_sample"], x[::W.LONG_X_STRIDE])
    plan = GrapePlan(fp, nparam=1, max_batch=1, options=OPT_GENERAL_H0)
    try:
        out = plan.fidelity_grad(x[None, :])
    finally:
        plan.close()
    got = {name: np.asarray(a[0]) for name, a in zip(W.LONG_OUTPUTS, out)}
    bounds = W.long_bounds(g, fp, x)
    rows, e = W.long_tail_rows()
    checks = [(name, got[name], g[name]) for name in W.LONG_OUTPUTS]
    checks.append(("F_d2err_dx", got["F_d2err_dx"][rows, e], g["F_d2err_dx"][rows, e]))
    failures = []
    for n, (name, a, r) in enumerate(checks):
        label = "wrap_long" + ("_tail" if n == len(W.LONG_OUTPUTS) else "")
        bound = bounds[name][0]
        err, scale = float(np.max(np.abs(a - r))), float(np.max(np.abs(r)))
        record(label, name, err, scale, bound)
        print(f"{label} {name}: device - exact {err:.2e}  oracle - exact {float(g['noise_' + name]):.2e}  "
              f"scale {scale:.2e}  bound {bound:.2e}")
        assert bound < 1e-2 * scale, (label, name, bound, scale)
        if not err <= bound:
            failures.append((label, name, err, bound))
    assert not failures, failures


# ---------------------------------------------------------------- a singular chain is reported, the plan recovers
@pytest.mark.parametrize("d", W.SING_DIMS)
def test_singular_chain_is_reported_and_the_plan_recovers(d):
    """A level whose decay the hot control drives to an exact zero of C_k (tests/unitary_wrap_cases.py): each
    public entry point reports GRAPE_ERR_SINGULAR from k_u_inverse's status bit (a defined error return, as
    Julia's inv throws), and the same cached plan then serves a cool control at the usual tiers: the sticky
    status word was cleared.  d = 5: LDS tiles; d = 13: scratch tiles over the pivoted dense exponential."""
    from oracle import grape_oracle as O
    from robustgrape_amd import (_capi, calculate_fidelity_and_derivatives, calculate_interaction_error_operators,
                                 calculate_unitary_and_derivatives)
    from robustgrape_amd.engine import fidelity_wrapper, get_plan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    fp = W.singular_problem(d)
    up = fp.unitary_problem
    hot, cool = W.singular_x(True), W.singular_x(False)
    singular = r"SINGULAR.*propagator chain"
    label = f"wrap_singular_d{d}"
    # fidelity
    with pytest.raises(_capi.GrapeError, match=singular):
        calculate_fidelity_and_derivatives(fp, hot)
    plan = get_plan(fp, W.NP)
    assert plan.options & OPT_GENERAL_H0 or d <= 12  # (d <= 12: the C side selects the general path itself)
    handle = plan.handle.value
    ref = O.calculate_fidelity_and_derivatives(fp, cool)
    _check_fidelity(calculate_fidelity_and_derivatives(fp, cool), ref, label, 1, fp, cool)
    assert get_plan(fp, W.NP) is plan and plan.handle.value == handle
    # materialised tensors and interaction operators: the plan of the wrapped unitary problem
    with pytest.raises(_capi.GrapeError, match=singular):
        calculate_unitary_and_derivatives(up, hot)
    uplan = get_plan(fidelity_wrapper(up), W.NP)
    uhandle = uplan.handle.value
    with pytest.raises(_capi.GrapeError, match=singular):
        calculate_interaction_error_operators(up, hot)
    got = calculate_unitary_and_derivatives(up, cool)
    tref = O.calculate_unitary_and_derivatives(up, cool)
    # the tensors' tier of this file: U_derr sums N_t = 20 forward differences, each with the oracle's own
    # u / eps = 2e-8 of rounding per entry of order 1, on a scale of 0.01
    _assert_tensors(got, tref, label, P.tensor_factor(fp, cool, nparam=W.NP))
    with pytest.raises(_capi.GrapeError, match=singular):
        calculate_unitary_and_derivatives(up, hot)
    _close(calculate_interaction_error_operators(up, cool), O.calculate_interaction_error_operators(up, cool),
           label, "O")
    assert get_plan(fidelity_wrapper(up), W.NP) is uplan and uplan.handle.value == uhandle


@pytest.mark.parametrize("d", W.SING_DIMS)
def test_a_deeply_decayed_chain_is_still_inverted(d):
    """The same problem with the control hot for 12 steps only: the cut-off level's entry of C_k stops at
    5e-217, a normal double with a finite reciprocal, and the oracle (LAPACK getrf / getri) evaluates every
    entry point.  k_u_inverse formed 1 / pivot as conj(pivot) / |pivot|^2, whose denominator underflows to 0
    below 1.5e-154: the row became inf / NaN, the elimination spread it over the whole inverse, and every
    output came back NaN with no status bit set.  The reciprocal is scaled now; this pins it."""
    from oracle import grape_oracle as O
    from robustgrape_amd import (calculate_fidelity_and_derivatives, calculate_interaction_error_operators,
                                 calculate_unitary_and_derivatives)
    fp = W.singular_problem(d)
    up = fp.unitary_problem
    x = W.singular_x(False, deep=True)
    label = f"wrap_deep_d{d}"
    got = calculate_fidelity_and_derivatives(fp, x)
    assert all(np.all(np.isfinite(a)) for a in got)
    _check_fidelity(got, O.calculate_fidelity_and_derivatives(fp, x), label, 1, fp, x)
    _assert_tensors(calculate_unitary_and_derivatives(up, x), O.calculate_unitary_and_derivatives(up, x), label,
                    P.tensor_factor(fp, x, nparam=W.NP))
    _close(calculate_interaction_error_operators(up, x), O.calculate_interaction_error_operators(up, x), label, "O")
