"""The small engine's exponential (d = 2 .. 12: grape_device.hpp's row groups; k_expm, k_expm_table, k_expm_grad,
k_expm_high, k_grad_high, k_expm_raw) at every size, degree, branch and wave seam.  The cases and the conditions
that make them bite are in tests/small_expm_cases.py, pinned on the CPU by tests/test_small_expm_cases_cpu.py; the
reference of exp is oracle.grape_exact.exp_ld (longdouble Taylor 40).  No input here is non-finite: the degree
choice's behaviour at +inf and NaN is checked on the host only (tests/test_pade_degree_cpu.py).

Tolerances:
  exp(A)       T0 as tests/test_gpu_dense_general.py and tests/test_gpu_tiled_edges.py state it: relative max-entry
               error <= 1e-13 max(1, |A|_1), 1e-12 max(1, |A|_1) where the degree is 13
  U            one hot step: T0 of that step's matrix; every step hot (contractions: |E_k|_2 <= 1, so errors do not
               grow through the product): the sum over the steps of T0 times max|E_k|, absolute
  F            1e-12 absolute
  F_dx         tests/problems.py fd_tier (nparam = 2); without error sources also against oracle.grape_exact's
               forward difference: no farther from it than the tier plus the oracle's own distance
  F_d2err      1e-6 fd_factor max|ref| + 1e-7
  F_d2err_dx   1e-5 fd_factor max|ref| + 1e-7; the x_add rows by tests/xadd_pin.py
"""
import functools

import numpy as np
import pytest

from tests import problems as P
from tests import small_expm_cases as C

pytestmark = pytest.mark.gpu
T1 = 1e-12
T2, T2_ABS = 1e-6, 1e-7
T3, T3_ABS = 1e-5, 1e-7


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _expm(mats, general=False):
    """exp of row-major matrices through the C ABI into a buffer pre-filled with NaN; returns (E, stats)."""
    from robustgrape_amd import _capi
    A = np.stack(mats)
    d = A.shape[-1]
    Acm = np.ascontiguousarray(A.transpose(0, 2, 1))  # column-major per matrix
    E = np.full_like(Acm, complex(np.nan, np.nan))
    stats = (_capi.ctypes.c_int * 5)()
    fn = _capi.lib().grape_expm_batch_general if general else _capi.lib().grape_expm_batch
    _capi.check(fn(0, d, len(A), _capi.dptr(Acm), _capi.dptr(E), stats))
    return E.transpose(0, 2, 1), list(stats)


# --- grape_expm_batch / grape_expm_batch_general ---------------------------------------------------------------
@pytest.mark.parametrize("d", C.DIMS)
def test_every_case_against_exp_ld(d):
    """All cases of the size in one batch (28 matrices: every wave mixes the shortcut, the in-kernel degrees and
    parked items) against exp_ld at T0; the zero matrix gives exactly I, the imaginary diagonal an off-diagonal of
    exactly 0; stats is the expected histogram, a diagonal input counting in slot 0."""
    from tests.parity_log import record
    names = [n for n, _ in C.cases(d)]
    mats = [A for _, A in C.cases(d)]
    refs = C.references(d)
    E, stats = _expm(mats)
    assert not np.any(np.isnan(E.real)) and not np.any(np.isnan(E.imag))
    worst = {}
    for j, name in enumerate(names):
        rel, tol = C.rel_err(E[j], refs[name]), C.tol(mats[j])
        record(f"small_expm_d{d}_{name}", "exp", rel, 1.0, tol)
        print(f"small expm d={d} {name} |A|_1={C.norm1(mats[j])!r} m,s={C.degree(mats[j])}: rel {rel:.2e} tol {tol:.1e}")
        fam = "diagonal" if name.startswith("diag") or name == "zero" else name.rstrip("0123456789.")
        worst[fam] = max(worst.get(fam, 0.0), rel / tol)
        assert rel <= tol, (d, name, rel, tol)
    print(f"small expm d={d} worst error / tier by family:", {k: round(v, 4) for k, v in worst.items()})
    z = E[names.index("zero")]
    assert np.array_equal(z.real, np.eye(d)) and not np.any(z.imag)
    di = E[names.index("diag_imag")]
    assert not np.any(di - np.diag(np.diag(di)))
    assert stats == C.histogram(mats), (stats, C.histogram(mats))
    # the shortcut is in the histogram's first slot: the three diagonal inputs and the cases of degree 3
    assert stats[0] == 3 + sum(1 for A in mats if C.degree(A)[0] == 3)


@pytest.mark.parametrize("d", C.DIMS)
def test_threshold_degrees_follow_the_norm_read_back(d):
    """One threshold case per call: stats names the degree the kernel took, which follows from the 1-norm in the
    kernel's own summation order (on the threshold: the lower degree; one double above: the higher)."""
    from oracle import grape_oracle as O
    for t in C.THRESHOLDS:
        A = C.case_map(d)[f"on{t}"]
        _, stats = _expm([A])
        want = [0] * 5
        want[C.SLOT[O.pade_degree(C.norm1(A))[0]]] = 1
        assert stats == want, (d, t, C.norm1(A), stats)


@pytest.mark.parametrize("d,slot", [(12, 0), (13, 4), (65, 4)])
def test_stats_slot_of_a_large_norm_diagonal_matrix_per_engine(d, slot):
    """include/grape.h: a diagonal matrix counts in the first slot on the small engine (the shortcut), by its
    1-norm on the dense and tiled engines (no shortcut).  A = 6 i diag(+-1): skew-Hermitian, |A|_1 = 6 > 5.4."""
    A = np.diag(6j * np.where(np.arange(d) % 2, -1.0, 1.0))
    E, stats = _expm([A])
    want = [0] * 5
    want[slot] = 1
    assert stats == want, (d, stats)
    assert C.rel_err(E[0], np.diag(np.exp(np.diag(A)))) <= C.T0_PADE13 * 6.0


@pytest.mark.parametrize("d", C.DIMS)
def test_general_entry_point_is_the_same_kernel(d):
    mats = [A for _, A in C.cases(d)]
    E0, s0 = _expm(mats)
    E1, s1 = _expm(mats, general=True)
    assert np.array_equal(E0, E1) and s0 == s1


@functools.lru_cache(maxsize=None)
def _singles(d, names):
    """Each case in a batch of one."""
    out = {}
    for n in names:
        E, _ = _expm([C.case_map(d)[n]])
        out[n] = E[0]
    return out


@pytest.mark.parametrize("d", C.DIMS)
def test_wave_seams(d):
    """Batches of 1, GPW - 1, GPW, GPW + 1 and 3 GPW + 2 matrices cycled from ten cases that alternate diagonal,
    low-norm, interchange and norm-30 items: every item is bitwise its value from a batch of one, and nothing of
    the NaN-filled output is left unwritten (GPW = 64 / d groups share a wave; the lanes past GPW d belong to none)."""
    names = C.seam_names(d)
    single = _singles(d, names)
    refs = C.references(d)
    for n in names:
        assert C.rel_err(single[n], refs[n]) <= C.tol(C.case_map(d)[n]), (d, n)
    g = C.gpw(d)
    for n in (1, g - 1, g, g + 1, 3 * g + 2):
        pick = [names[i % len(names)] for i in range(n)]
        E, stats = _expm([C.case_map(d)[p] for p in pick])
        assert not np.any(np.isnan(E.real)) and not np.any(np.isnan(E.imag)), (d, n)
        bad = [i for i in range(n) if not np.array_equal(E[i], single[pick[i]])]
        assert not bad, (d, n, bad[:10])
        assert stats == C.histogram([C.case_map(d)[p] for p in pick]), (d, n, stats)


@pytest.mark.parametrize("d", [2, 7, 12])
def test_k_expm_high_strides_over_the_parked_list(d):
    """64 GPW + 3 items that all park (2 051, 579 and 323 matrices, cycled from five cases): k_expm_high's 64
    workgroups take a second trip over the list, with a ragged tail.  Every item is bitwise its first occurrence,
    the first five meet the reference, stats is the cycled list's histogram."""
    names = C.parked_names(d)
    n = 64 * C.gpw(d) + 3
    assert n == {2: 2051, 7: 579, 12: 323}[d]
    pick = [names[i % 5] for i in range(n)]
    E, stats = _expm([C.case_map(d)[p] for p in pick])
    refs = C.references(d)
    for j in range(5):
        rel, tol = C.rel_err(E[j], refs[names[j]]), C.tol(C.case_map(d)[names[j]])
        assert rel <= tol, (d, names[j], rel, tol)
    bad = [i for i in range(5, n) if not np.array_equal(E[i], E[i % 5])]
    assert not bad, (d, bad[:10])
    assert stats == C.histogram([C.case_map(d)[p] for p in pick])
    assert stats[0] == stats[1] == 0


# --- the pipeline's own exponentials, through U --------------------------------------------------------------
HOT = ("interchange0.0", "ginibre0.2", "ginibre0.01", "decay1.5", "decay30.0", "diag_decay", "on0.25", "rankone5.3")
ALL_HOT = ("decay0.2", "decay0.6", "decay1.5", "decay4.0")


def probe_problem(d, mats, steps, device):
    """(unitary problem, x) whose step k has A_k = -i dt H_k = mats[steps[k]] exactly (A_k = 0 where steps[k] is
    None): N_t = len(steps), t0 = N_t so dt = 1, one control per matrix, H0(nt, x) = sum_p x[p] (i mats[p]) with
    x[k, p] = 1 where steps[k] == p and 0 elsewhere (a product by 1 or 0 and sums with 0: exact; a step of zeros
    is the zero matrix and takes the shortcut to an exact identity).  The term kinds have no gate on the step
    index, so the controls are the gate, for the operator basis (device = True: k_expm, k_expm_lane at d <= 3) and
    for the same function as a plain closure (device = False: the host table, k_expm_table)."""
    from robustgrape_amd.operators import FN_LINEAR, VAR_X, OperatorBasisHamiltonian, Term
    from robustgrape_amd.types import UnitaryRobustGRAPEProblem
    basis = OperatorBasisHamiltonian([Term(1j * np.asarray(M), var=VAR_X, index=p, func=FN_LINEAR)
                                      for p, M in enumerate(mats)])
    H0 = basis if device else (lambda t, x, xa: basis(t, x, xa))
    nt = len(steps)
    x = np.zeros((nt, len(mats)))
    for k, p in enumerate(steps):
        if p is not None:
            x[k, p] = 1.0
    return UnitaryRobustGRAPEProblem(t0=float(nt), ntimes=nt, ndim=d, H0=H0, nb_additional_param=0), x.reshape(-1)


@functools.lru_cache(maxsize=None)
def _one_hot_problems(d):
    """One problem per form, shared by every layout of the size: the plan is created once."""
    mats = [C.case_map(d)[n] for n in HOT]
    nt = C.gpw(d) + 2
    return {dev: probe_problem(d, mats, [None] * nt, dev)[0] for dev in (True, False)}


@pytest.mark.parametrize("device", [True, False], ids=["basis", "closure"])
@pytest.mark.parametrize("d", C.DIMS)
def test_pipeline_one_hot_step(d, device):
    """N_t = GPW + 2 steps, all zero (the shortcut: exact identities) except step j in {0, GPW - 1, GPW, N_t - 1}:
    U must meet exp_ld of that one matrix at its T0 tier.  Hot matrices: row interchanges, ginibre at 0.2 (Taylor
    12 in the pipeline, where k_expm_raw runs Pade 5) and 0.01 (Taylor 6), decay at 1.5 and 30 (parked: k_expm_high
    writes row-major into the slot it read column-major), the decay diagonal, the norm on 0.25 (Taylor 12 at the
    top of its range, chosen on the |re| + |im| bound, which is the norm itself there) and the rank-one matrix whose
    A^13 is as large as its norm allows."""
    from robustgrape_amd import calculate_unitary_and_derivatives
    from tests.parity_log import record
    g = C.gpw(d)
    nt = g + 2
    up = _one_hot_problems(d)[device]
    refs = C.references(d)
    for p, name in enumerate(HOT):
        M = C.case_map(d)[name]
        for j in sorted({0, g - 1, g, nt - 1}):
            x = np.zeros((nt, len(HOT)))
            x[j, p] = 1.0
            U = np.asarray(calculate_unitary_and_derivatives(up, x.reshape(-1))[0])
            rel, tol = C.rel_err(U, refs[name]), C.tol(M)
            record(f"small_expm_onehot_{'basis' if device else 'closure'}_d{d}_{name}_j{j}", "U", rel, 1.0, tol)
            assert rel <= tol, (d, device, name, j, rel, tol)
    x = np.zeros(nt * len(HOT))
    U = np.asarray(calculate_unitary_and_derivatives(up, x)[0])
    assert np.array_equal(U.real, np.eye(d)) and not np.any(U.imag)  # every step the shortcut: exactly I


@pytest.mark.parametrize("device", [True, False], ids=["basis", "closure"])
@pytest.mark.parametrize("d", C.DIMS)
def test_pipeline_every_step_hot(d, device):
    """N_t = GPW + 2 steps cycling decay-family matrices of norms 0.2 / 0.6 / 1.5 / 4.0 (Taylor 12, Pade 7, 9, 13 in
    one wave) against the ordered longdouble product of the steps' exp_ld."""
    from oracle import grape_exact as X
    from robustgrape_amd import calculate_unitary_and_derivatives
    from tests.parity_log import record
    mats = [C.case_map(d)[n] for n in ALL_HOT]
    nt = C.gpw(d) + 2
    steps = [k % len(mats) for k in range(nt)]
    up, x = probe_problem(d, mats, steps, device)
    El = [X.exp_ld(M.astype(np.clongdouble)) for M in mats]
    for M, E in zip(mats, El):
        assert np.linalg.norm(np.asarray(E, np.complex128), 2) <= 1.0 + 1e-14  # a contraction
    ref = np.eye(d, dtype=np.clongdouble)
    for k in steps:
        ref = El[k] @ ref  # C_k = E_k C_{k-1}
    ref = np.asarray(ref, np.complex128)
    tol = sum(C.tol(mats[k]) * float(np.max(np.abs(El[k]))) for k in steps)
    U = np.asarray(calculate_unitary_and_derivatives(up, x)[0])
    err = float(np.max(np.abs(U - ref)))
    record(f"small_expm_allhot_{'basis' if device else 'closure'}_d{d}", "U", err, float(np.max(np.abs(ref))), tol)
    print(f"all hot d={d} {'basis' if device else 'closure'}: err {err:.2e} tol {tol:.2e} max|U| {np.max(np.abs(ref)):.2e}")
    assert err <= tol, (d, device, err, tol)


# --- fidelity and gradient with parked steps at every size --------------------------------------------------
BANDS = ((0.25, 0.95, 0.6), (0.95, 2.1, 1.5), (2.1, 5.4, 3.5), (5.4, 10.8, 8.0))  # (lo, hi], aimed at


@pytest.mark.parametrize("nerr", [0, 2])
@pytest.mark.parametrize("band", range(len(BANDS)))
@pytest.mark.parametrize("d", C.DIMS)
def test_parked_steps_fidelity_and_gradient(d, band, nerr):
    """tests/test_gpu_dims.py's random problems with the step norm scaled into each of Pade 7, 9, 13 and 13 with
    one squaring, whole matrices (GRAPE_OPT_NO_SECTORS), N_t = 7: without error sources k_expm_grad parks for
    k_grad_high, with two k_expm<ERR> parks for k_expm_high and the error path follows."""
    from oracle import grape_exact as X
    from oracle import grape_oracle as O
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_SECTORS
    from tests.parity_log import record
    from tests.test_gpu_dims import random_problem
    from tests.xadd_pin import check_xadd, exact_rows
    nt = 7
    lo, hi, aim = BANDS[band]
    rng = np.random.default_rng(d * 100 + band * 10 + nerr)
    x = np.concatenate([rng.uniform(-1, 1, size=2 * nt), [rng.uniform(0, 2 * np.pi)]])
    scale = aim / P.max_step_norm(random_problem(d, nt, nerr, False), x, 2)
    fpo, fpd = random_problem(d, nt, nerr, False, scale=scale), random_problem(d, nt, nerr, True, scale=scale)
    norm = P.max_step_norm(fpo, x, 2)
    assert lo < norm <= hi, (norm, lo, hi)
    ref = O.calculate_fidelity_and_derivatives(fpo, x)
    plan = GrapePlan(fpd, nparam=2, max_batch=1, options=OPT_NO_SECTORS)
    try:
        got = [np.asarray(a)[0] for a in plan.fidelity_grad(x[None, :])]
    finally:
        plan.close()
    label = f"small_expm_parked_d{d}_band{band}_ne{nerr}"
    f = P.fd_factor(fpo, x, nparam=2)
    t, ta = P.fd_tier(fpo, x, nparam=2)
    eF = abs(float(got[0]) - ref[0])
    record(label, "F", eF, 1.0, T1)
    assert eF <= T1, (label, eF)
    g0 = np.asarray(ref[1])
    err, sc = float(np.max(np.abs(got[1] - g0))), float(np.max(np.abs(g0)))
    record(label, "F_dx", err, sc, t * sc + ta)
    print(label, f"|A|_1 {norm:.3f} F {eF:.1e} F_dx {err:.2e} / {sc:.2e} tol {t * sc + ta:.2e}")
    assert err <= t * sc + ta, (label, "F_dx", err, sc)
    nmain = len(x) - 1
    if nerr == 0:
        ex = np.asarray(X.fidelity_and_gradient(fpd, x, nparam=2)[1], np.float64)
        own = float(np.max(np.abs(g0 - ex)))  # the oracle's own distance from the exact forward difference
        e, s = float(np.max(np.abs(got[1] - ex))), float(np.max(np.abs(ex)))
        record(label + "_vs_exact", "F_dx", e, s, t * s + ta + own)
        assert e <= t * s + ta + own, (label, "F_dx vs exact", e, own)
        return
    d20, d2dx0 = np.asarray(ref[2]), np.asarray(ref[3])
    e2, s2 = float(np.max(np.abs(got[2] - d20))), float(np.max(np.abs(d20)))
    record(label, "F_d2err", e2, s2, T2 * f * s2 + T2_ABS)
    assert e2 <= T2 * f * s2 + T2_ABS, (label, "F_d2err", e2, s2)
    e3, s3 = float(np.max(np.abs(got[3][:nmain] - d2dx0[:nmain]))), float(np.max(np.abs(d2dx0[:nmain])))
    record(label, "F_d2err_dx", e3, s3, T3 * f * s3 + T3_ABS)
    assert e3 <= T3 * f * s3 + T3_ABS, (label, "F_d2err_dx", e3, s3)
    check_xadd(label, got[3], d2dx0, nmain, exact_rows(fpd, x, 2), rel=T3 * f, ab=T3_ABS * f)
