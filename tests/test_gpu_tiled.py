"""GPU parity of the tiled (MFMA, matrices in HBM) engine, 64 < d <= 128, through the
C ABI: its exponential against the oracle's restatement of Julia's exp!, the fidelity and the control
gradient against the CPU oracle and the exact (longdouble) forward difference -- live at d = 65, from
the committed fixture tests/golden/tiled.npz (tests/golden/make_golden_tiled.py) for the slow cases.

Tolerances: the dense suite's own tiers (header of tests/test_gpu_dense.py)
  T0  exp(A)   <= 1e-13 relative x max(1, |A|_1); 1e-12 x max(1, |A|_1) where Julia takes Pade 13;
               unitarity 1e-12 x max(1, |A|_1)
  T1  F        <= 1e-12 absolute
  T2  F_dx     device - exact  <= 1e-6 max|exact| + 1e-9
               device - oracle <= 1e-6 max|oracle| + 1e-9 + |oracle - exact|
and, so that the oracle's own distance stays an honest part of the bound, each case asserts that the oracle
alone sits within half the device-vs-exact tier.
"""
import functools
import os

import numpy as np
import pytest

from robustgrape_amd import synthetic as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T1 = 1e-12
T2, T2_FLOOR = 1e-6, 1e-9


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _problem(d, ntimes, scale, phase):
    x = S.dense_x(ntimes, seed=300 + ntimes)
    if phase:
        return S.dense_error_problem(d, ntimes, rank=16, scale=scale, nerr=0, phase=True), np.concatenate([x, [0.3]])
    return S.dense_problem(d, ntimes, rank=16, scale=scale), x


def _assert_fid(test, F, Fdx, ref_F, ref_Fdx, exact_F, exact_Fdx):
    from tests.parity_log import record
    ref_Fdx, exact_Fdx = np.asarray(ref_Fdx), np.asarray(exact_Fdx)
    ef = abs(F - ref_F)
    record(test, "F", ef, 1.0, T1)
    print(f"{test}: F err {ef:.3e}")
    assert ef <= T1, (F, ref_F)
    se = float(np.max(np.abs(exact_Fdx)))
    tier = T2 * se + T2_FLOOR
    noise = float(np.max(np.abs(ref_Fdx - exact_Fdx)))
    record(test + "_oracle_vs_exact", "F_dx", noise, se, 0.5 * tier)
    ee = float(np.max(np.abs(Fdx - exact_Fdx)))
    record(test + "_vs_exact", "F_dx", ee, se, tier)
    err, scale = float(np.max(np.abs(Fdx - ref_Fdx))), float(np.max(np.abs(ref_Fdx)))
    tol = T2 * scale + T2_FLOOR + noise
    record(test, "F_dx", err, scale, tol)
    print(f"{test}: F_dx vs exact {ee:.3e} (tier {tier:.2e}), vs oracle {err:.3e} (tol {tol:.2e}), "
          f"oracle vs exact {noise:.2e}")
    assert noise <= 0.5 * tier, ("oracle vs exact", noise, tier)
    assert ee <= tier, ("vs exact", ee, se)
    assert err <= tol, (err, scale, noise)


def _skew_hermitian(d, norm, rng):
    H = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    H = (H + H.conj().T) / 2
    return -1j * H / np.abs(H).sum(axis=0).max() * norm


@pytest.mark.parametrize("d", [65, 96, 128])
def test_tiled_expm_matches_oracle_every_degree_and_squaring_count(d):
    from oracle import grape_oracle as O
    from robustgrape_amd import _capi
    from tests.parity_log import record
    rng = np.random.default_rng(1000 + d)
    norms = (0.01, 0.04, 0.2, 0.6, 0.8, 0.9, 1.5, 4.0, 30.0)  # Taylor 8 / 8 / 12 / 16 / 16 / 20, then s = 1, 3, 5
    A = np.stack([_skew_hermitian(d, nm, rng) for nm in norms])
    refs, ms = [], []
    for a in A:
        st = {}
        refs.append(O.julia_exp(a, st))
        ms.append(list(st)[0][0])
    Acm = np.ascontiguousarray(A.transpose(0, 2, 1))  # column-major per matrix
    E = np.full_like(Acm, np.nan)
    stats = (_capi.ctypes.c_int * 5)()
    _capi.check(_capi.lib().grape_expm_batch(0, d, len(A), _capi.dptr(Acm), _capi.dptr(E), stats))
    E = E.transpose(0, 2, 1)
    for j, nm in enumerate(norms):
        rel = np.max(np.abs(E[j] - refs[j])) / np.max(np.abs(refs[j]))
        tol = (1e-12 if ms[j] == 13 else 1e-13) * max(1.0, nm)
        uni = np.max(np.abs(E[j].conj().T @ E[j] - np.eye(d)))
        record(f"tiled_expm_d{d}_norm{nm}", "exp", rel, 1.0, tol)
        print(f"tiled expm d={d} |A|_1={nm}: rel {rel:.2e} (tol {tol:.1e}), unitarity {uni:.2e}")
        assert rel <= tol, (d, nm, ms[j], rel)
        assert uni < 1e-12 * max(1.0, nm), (d, nm, uni)
    hist = {3: 0, 5: 1, 7: 2, 9: 3, 13: 4}
    expect = [0] * 5
    for m in ms:
        expect[hist[m]] += 1
    assert list(stats) == expect


@pytest.mark.parametrize("d,ntimes,scale,phase", [(65, 1, 1.0, False), (65, 3, 1.0, True)])
def test_tiled_fidelity_gradient_matches_live_oracle_and_exact(d, ntimes, scale, phase):
    """One step (no prefix product, one chunk) and the x_add target at the first tiled size (P = 80)."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_fidelity_and_derivatives
    fp, x = _problem(d, ntimes, scale, phase)
    F0, g0, _, _ = O.calculate_fidelity_and_derivatives(fp, x)
    Fe, ge = E.fidelity_and_gradient(fp, x, nparam=2)
    F, g, d2, d2dx = calculate_fidelity_and_derivatives(fp, x)
    _assert_fid(f"tiled_live_d{d}_nt{ntimes}", F, g, F0, g0, Fe, ge)
    assert d2.shape == (0,) and d2dx.shape == (len(x), 0)


@functools.lru_cache(maxsize=1)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "tiled.npz"), allow_pickle=False))


@pytest.mark.parametrize("case", range(6))
def test_tiled_matches_golden(case):
    """Every padded size (80, 96, 112, 128), P != d and P = d, chunk remainders (N_t = 19, 7), Taylor 8
    (scale 0.05), one squaring (scale 2.0: |A|_1 = 1.42), the x_add target (case 4)."""
    from robustgrape_amd import calculate_fidelity_and_derivatives
    g = _golden()
    d, ntimes, phase = (int(v) for v in g["cases"][case])
    fp, x = _problem(d, ntimes, float(g["scales"][case]), bool(phase))
    assert np.array_equal(x, g[f"x{case}"])
    F, Fdx, _, _ = calculate_fidelity_and_derivatives(fp, x)
    _assert_fid(f"tiled_golden_d{d}_nt{ntimes}", F, Fdx, float(g[f"F{case}"]), g[f"F_dx{case}"],
                float(g[f"F_exact{case}"]), g[f"F_dx_exact{case}"])


def test_the_user_level_call_at_81_levels():
    """Four three-level atoms (3^4 = 81 levels) through the public function."""
    from robustgrape_amd import calculate_fidelity_and_derivatives
    F, Fdx, _, _ = calculate_fidelity_and_derivatives(S.dense_problem(81, 5, rank=16), S.dense_x(5, seed=305))
    assert abs(F - float(_golden()["F1"])) <= T1 and abs(F - 0.015365) < 1e-6 and Fdx.shape == (10,)


def test_tiled_batch_equals_single():
    """Deterministic kernels, passes with identical arithmetic: a batch element is bitwise the single
    evaluation, whatever the pass it lands in (5 in one pass against 2 + 2 + 1)."""
    from robustgrape_amd.engine import GrapePlan
    fp = S.dense_problem(96, 6, rank=16)
    X = np.stack([S.dense_x(6, seed=s) for s in range(5)])
    plan = GrapePlan(fp, nparam=2, max_batch=5)
    F, Fdx, _, _ = plan.fidelity_grad(X)
    plan.close()
    one = GrapePlan(fp, nparam=2, max_batch=2)  # ragged: 2 + 2 + 1 through one plan
    F1, Fdx1, _, _ = one.fidelity_grad(X)
    one.close()
    assert np.all(np.isfinite(Fdx)) and np.array_equal(F, F1) and np.array_equal(Fdx, Fdx1)


def test_tiled_device_call_is_the_host_call():
    import torch

    from robustgrape_amd.engine import GrapePlan
    fp = S.dense_problem(80, 4, rank=16)
    X = np.stack([S.dense_x(4, seed=40 + s) for s in range(3)])
    plan = GrapePlan(fp, nparam=2, max_batch=3)
    try:
        dev = torch.device("cuda", 0)
        Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
        F = torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
        Fdx = torch.full(X.shape, float("nan"), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        plan.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), Fdx.data_ptr(), 3)
        plan.synchronize()
        Fh, Fdxh, _, _ = plan.fidelity_grad(X)
        assert plan.sectors() == ((80, 1),)
    finally:
        plan.close()
    assert np.all(np.isfinite(Fdxh))
    assert np.array_equal(F.cpu().numpy(), Fh) and np.array_equal(Fdx.cpu().numpy(), Fdxh)


def test_a_tiled_plan_refuses_the_analysis_entry_points_and_the_slices():
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    d, nt = 65, 2
    plan = GrapePlan(S.dense_problem(d, nt, rank=16), nparam=2, max_batch=1)
    L = _capi.lib()
    x = S.dense_x(nt, seed=1)
    buf = np.zeros(2 * d * d * nt * 2)
    try:
        with pytest.raises(_capi.GrapeError, match="UNSUPPORTED"):
            plan.unitary_derivs(x)
        for call in (lambda: L.grape_interaction_error_operators(plan.handle, _capi.dptr(x), _capi.dptr(buf)),
                     lambda: L.grape_expectation_values(plan.handle, _capi.dptr(x), _capi.dptr(buf)),
                     lambda: L.grape_slice_forward(plan.handle, _capi.dptr(x), _capi.dptr(buf)),
                     lambda: L.grape_slice_gradient(plan.handle, _capi.dptr(buf), _capi.dptr(buf))):
            assert call() == _capi.ERR_UNSUPPORTED, L.grape_last_error()
        F, _, _, _ = plan.fidelity_grad(x[None, :])  # the plan still serves what it serves
        assert np.isfinite(F[0])
    finally:
        plan.close()
