"""General projectors on the paths and with the patterns tests/test_gpu_projector.py leaves out
(tests/projector_cases.py: the generators, the case table, why dense_projector cannot tell B from B^dagger).

  a. the small engine's whole-matrix heads k_proj_fid / k_proj_err (no sectors) at d = 2, 3, 7, 8, 12 with
     np = 2, and at d = 5, 9 with H0 reading x_add (the tgt_part branch);
  b. the same heads on the dense engine's register-file images, d = 13 .. 64 (k_dmc / k_dmce downstream);
  c. k_u_fid_head on Hermitian problems (GRAPE_OPT_GENERAL_H0 forced), LDS tiles (d = 9) and global-scratch
     tiles (d = 16), against the oracle, the longdouble evaluation and the default path;
  d. k_u_fid_head with a decay term, d = 9, 16, 40, and with non-0/1 diagonal weights;
  e. closure plans: the per-evaluation target table at b = 1 and on a ragged remainder;
  f. batches are the single calls, bit for bit;
  g. calculate_expectation_values (k_u_expect's general branch) and calculate_fidelity_response.

Tiers (unchanged from the files named): F 1e-12.  Hermitian problems as tests/test_gpu_dense.py _assert_fid:
F_dx against oracle/grape_exact.py at 1e-6 max|exact| + 1e-9 where it covers the problem, and against the
oracle at the same tier plus the oracle's own distance from exact (an H0 reading x_add is covered for F and
F_dx by fidelity_and_gradient_xadd); F_d2err at 1e-6 max|ref| + 1e-7, F_d2err_dx at 1e-5 max|ref| + 1e-7, against
the oracle and, where the evaluator has them, against exact.  Decay problems, which the evaluator does not
cover, against the oracle as tests/test_gpu_dense_general.py _check (tests/problems.py fd_tier / fd_factor)."""
import numpy as np
import pytest

from tests import problems as P
from tests import projector_cases as PC
from tests.projector_cases import T1, T2, T2_ABS, T2_FLOOR, T3, T3_ABS

pytestmark = pytest.mark.gpu
BY_GROUP = {g: [c.name for c in PC.CASES.values() if c.group == g] for g in "abcd"}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(c, X, max_batch=1, fp=None, options=None, profile=False):
    """(outputs, sectors(), kernel_times() or None, the plan's options) of a fresh plan over the rows of X."""
    from robustgrape_amd.engine import GrapePlan
    plan = GrapePlan(PC.problem(c) if fp is None else fp, nparam=PC.nparam(c), max_batch=max_batch,
                     options=c.options if options is None else options)
    try:
        if profile:
            plan.set_profiling(True)
        out = plan.fidelity_grad(np.atleast_2d(X))
        return out, plan.sectors(), plan.kernel_times() if profile else None, plan.options
    finally:
        plan.close()


def _row(out, b=0):
    return tuple(o[b] for o in out)


def _rec(label, name, err, scale, tol):
    from tests.parity_log import record
    record(label, name, err, scale, tol)
    print(f"{label} {name}: err {err:.2e} scale {scale:.2e} tol {tol:.2e}")


def _dist(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b))), float(np.max(np.abs(b)))


def _check_hermitian(label, got, ref, exact, ne):
    """tests/test_gpu_dense.py's _assert_fid and _assert_err, with the sensitivities against exact too where the
    evaluator has them.  (That file's stand-in where no exact evaluation exists, the spread between the oracle
    and the C++ port, does not apply here: the port takes diagonal projectors only.)"""
    err = abs(float(got[0]) - ref[0])
    _rec(label, "F", err, 1.0, T1)
    assert err <= T1, (label, got[0], ref[0])
    noise = _dist(ref[1], exact[1])[0]   # the oracle's own distance from exact
    err, scale = _dist(got[1], exact[1])
    _rec(label + "_vs_exact", "F_dx", err, scale, T2 * scale + T2_FLOOR)
    assert err <= T2 * scale + T2_FLOOR, (label, "F_dx vs exact", err, scale)
    err, scale = _dist(got[1], ref[1])
    _rec(label, "F_dx", err, scale, T2 * scale + T2_FLOOR + noise)
    assert err <= T2 * scale + T2_FLOOR + noise, (label, "F_dx", err, scale, noise)
    if not ne:
        return
    for against, tag in ((ref, ""), (exact, "_vs_exact")):
        if against[2] is None:   # H0 reads x_add: the evaluator has F and F_dx only
            continue
        for n, (name, rel, ab) in ((2, ("F_d2err", T2, T2_ABS)), (3, ("F_d2err_dx", T3, T3_ABS))):
            err, scale = _dist(got[n], against[n])
            _rec(label + tag, name, err, scale, rel * scale + ab)
            assert err <= rel * scale + ab, (label + tag, name, err, scale)


def _check_tiers(label, got, ref, ne, fp, x, nparam, scaled=True):
    """Two uses.  Decay cases against the oracle (scaled): tests/test_gpu_dense_general.py's _check without its
    oracle-to-C++-port spread (the port takes diagonal projectors only) -- the F_dx tier of tests/problems.py
    fd_tier, F_d2err and F_d2err_dx at T2 / T3 times fd_factor.  The general path against the default path of a
    Hermitian problem (scaled=False): tests/test_gpu_general_h0.py's _check as
    test_general_path_on_a_hermitian_problem_matches_the_fused_path calls it -- fd_tier for F_dx, F_d2err and
    F_d2err_dx at the flat T2 / T3."""
    f = P.fd_factor(fp, x, nparam=nparam) if scaled else 1.0
    t, ta = P.fd_tier(fp, x, nparam=nparam)
    err = float(np.max(np.abs(np.asarray(got[0]) - ref[0])))
    _rec(label, "F", err, 1.0, T1)
    assert err <= T1, (label, err)
    for n, (name, rel, ab) in enumerate([("F_dx", t, ta), ("F_d2err", T2 * f, T2_ABS), ("F_d2err_dx", T3 * f, T3_ABS)], 1):
        if n > 1 and ne == 0:
            break
        err, scale = _dist(got[n], ref[n])
        tol = rel * scale + ab
        _rec(label, name, err, scale, tol)
        assert err <= tol, (label, name, err, scale, tol)


def _against_references(c, got, label=None, x=None, ref=None, exact=None):
    """One evaluation of case c against its references (the table's control vector unless x, ref and, for a
    Hermitian case, exact are given)."""
    if x is None:
        x, ref, exact = PC.reference(c.name)
    label = label or f"projpaths_{c.name}"
    if c.decay:
        _check_tiers(label, got, ref, c.nerr, PC.problem(c, device=False), x, PC.nparam(c))
    else:
        _check_hermitian(label, got, ref, exact, c.nerr)
    assert np.asarray(got[1]).shape == (len(x),) and np.asarray(got[3]).shape == (len(x), c.nerr)


# --------------------------------------------------------------------------------------------- a, b
@pytest.mark.parametrize("name", BY_GROUP["a"])
def test_whole_matrix_small_engine(name):
    c = PC.CASES[name]
    x, ref, exact = PC.reference(name)
    out, sectors, _, _ = _run(c, x)
    assert sectors == ((c.d, 1),), sectors   # no sectors: k_proj_fid / k_proj_err, not the sector heads
    _against_references(c, _row(out))
    if c.builder == "xadd":   # H0 reads x_add: the heads' target part goes through tgt_part
        assert np.max(np.abs(ref[1][-2:])) > 1e-6 and np.max(np.abs(ref[3][-2:])) > 1e-6


@pytest.mark.parametrize("name", BY_GROUP["b"])
def test_dense_engine(name):
    c = PC.CASES[name]
    x, ref, exact = PC.reference(name)
    out, _, kt, _ = _run(c, x, profile=True)
    print({k: v[1] for k, v in kt.items() if v[1]})
    assert kt["k_dexp"][1] > 0 and kt["k_dmc"][1] > 0 and kt["k_expm"][1] == 0, kt   # the dense engine ran
    _against_references(c, _row(out))
    if c.builder == "dense_xadd":
        assert abs(ref[1][-1]) > 1e-6   # the H0 part of F_dx_add is not empty


# --------------------------------------------------------------------------------------------- c, d
@pytest.mark.parametrize("name", BY_GROUP["c"])
def test_general_path_on_hermitian_problems(name):
    """k_u_fid_head with non-symmetric P.PA / P.PB where the longdouble evaluator and the fused path still
    apply: against the oracle (and exact), and against the default plan of the same problem."""
    from robustgrape_amd.operators import OPT_GENERAL_H0
    c = PC.CASES[name]
    x, ref, exact = PC.reference(name)
    out, _, _, options = _run(c, x)
    assert options & OPT_GENERAL_H0
    _against_references(c, _row(out))
    fused, _, _, fopts = _run(c, x, options=0)
    assert not (fopts & OPT_GENERAL_H0)
    _check_tiers(f"projpaths_{name}_vs_fused", _row(out), _row(fused), c.nerr, PC.problem(c), x, PC.nparam(c),
                 scaled=False)
    up = PC.problem(c).unitary_problem
    if name == "general9_xadd":   # the (e, q) indexing of U_derr_dx_add needs both above one
        assert up.nb_additional_param == 2 and len(up.error_sources) == 2
        assert np.min(np.abs(ref[3][-1])) > 1e-3   # F_d2err_dx_add[q = 1, :] is not noise


@pytest.mark.parametrize("name", BY_GROUP["d"])
def test_general_path_with_decay(name):
    from robustgrape_amd.operators import OPT_GENERAL_H0
    c = PC.CASES[name]
    x, ref, _ = PC.reference(name)
    assert abs(ref[0] - PC.fidelity_without_decay(name)) > 1e-4   # the decay is visible
    out, _, _, options = _run(c, x)
    assert options & OPT_GENERAL_H0
    _against_references(c, _row(out))
    if c.proj == "weighted":   # really the diagonal specialisation, with weights that are not 0 / 1
        W = PC.projector(c)
        assert np.array_equal(W, np.diag(np.diag(W))) and 0.5 in np.diag(W)


# --------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("name", ["xadd9_whole", "decay16_ne2"])
def test_closure_plans_read_the_target_table_of_their_evaluation(name):
    """Three evaluations through a closure plan of two: the host-evaluated target table U0tab is read at
    b = 1 and on the ragged remainder (k_proj_fid / k_proj_err build_target; k_u_fid_head's fid::target)."""
    from oracle import grape_oracle as O
    from robustgrape_amd.engine import GrapePlan
    c = PC.CASES[name]
    fpc = P.as_closures(PC.problem(c))
    X = PC.batch_controls(c, 3)
    assert len({tuple(r[-1:]) for r in X}) == 3   # the targets differ from row to row
    plan = GrapePlan(fpc, nparam=PC.nparam(c), max_batch=2, options=c.options)
    try:
        assert plan.tables and plan.max_batch == 2
        if not c.decay:
            assert plan.sectors() == ((c.d, 1),)
        out = plan.fidelity_grad(X)
    finally:
        plan.close()
    fpo = PC.problem(c, device=False)
    for b in range(3):
        if b == 0:
            _, ref, exact = PC.reference(name)
        else:
            ref, exact = O.calculate_fidelity_and_derivatives(fpo, X[b]), PC.exact_outputs(c, X[b])
        _against_references(c, _row(out, b), f"projpaths_{name}_closures_{b}", X[b], ref, exact)


# --------------------------------------------------------------------------------------------- f
@pytest.mark.parametrize("name", ["dense17_ne2", "dims12_ne2", "decay16_ne2"])
def test_batches_are_the_single_calls(name):
    """Five evaluations through a plan of two (2 + 2 + 1): the per-evaluation scratch, image and output
    offsets of the general heads at b > 0; rows 0, 3 and 4 are the single calls, bit for bit."""
    from robustgrape_amd.engine import GrapePlan
    c = PC.CASES[name]
    assert c.nerr == 2
    X = PC.batch_controls(c, 5)
    plan = GrapePlan(PC.problem(c), nparam=PC.nparam(c), max_batch=2, options=c.options)
    try:
        out = plan.fidelity_grad(X)
        for b in (0, 3, 4):
            one = plan.fidelity_grad(X[b:b + 1])
            for q, (a, s) in enumerate(zip(_row(out, b), _row(one))):
                assert np.array_equal(a, s), (name, b, q)
    finally:
        plan.close()
    x, ref, exact = PC.reference(name)   # and row 0 is the case's own evaluation
    _against_references(c, _row(out, 0), f"projpaths_{name}_batch_0")
    assert not np.array_equal(out[1][0], out[1][3])


# --------------------------------------------------------------------------------------------- g
@pytest.mark.parametrize("name", ["general16_ne2", "decay9_xadd", "decay16_ne2"])
def test_analysis_entry_points(name):
    """tr(P0 O) of k_u_expect's general branch and the fidelity response at three frequencies, at
    tests/test_gpu_analysis.py's tolerances.  On a Hermitian plan O is Hermitian and P0 real, so tr(P0 O) and
    tr(P0 O^T) have the same real part; with a decay term they differ, below and above 12 levels."""
    from oracle import grape_oracle as O
    from robustgrape_amd import analysis as A
    c = PC.CASES[name]
    fp, fo, x = PC.problem(c), PC.problem(c, device=False), PC.control(c)
    ev0 = O.calculate_expectation_values(fo, x)
    ev = A.calculate_expectation_values(fp, x)
    assert ev.shape == ev0.shape == (c.nt, c.nerr)
    err, scale = _dist(ev, ev0)
    _rec(f"projpaths_{name}", "expectation", err, scale, 1e-7 * max(1.0, scale))
    assert err <= 1e-7 * max(1.0, scale)
    w = np.array([0.0, 0.3, 1.7])
    r0 = O.calculate_fidelity_response(fo, x, w)
    r = A.calculate_fidelity_response(fp, x, w)
    assert r.shape == r0.shape == (3, c.nerr)
    err, scale = _dist(r, r0)
    _rec(f"projpaths_{name}", "response", err, scale, 1e-6 * max(1.0, scale))
    assert err <= 1e-6 * max(1.0, scale)
    if c.decay:   # the transposed contraction would be another number, far outside the tolerance above
        up = fo.unitary_problem
        cums = np.cumsum(O.calculate_interaction_error_operators(up, x), axis=2)
        P0 = PC.projector(c)
        swapped = up.t0 / up.ntimes * np.real(np.einsum("ij,ijke->ke", P0, cums) - np.einsum("ij,jike->ke", P0, cums)) / np.trace(P0)
        assert np.max(np.abs(swapped)) > 1e-3
