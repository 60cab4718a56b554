"""GPU parity of the tiled engine's error path, 64 < d <= 128 with GRAPE_OPT_TILED_ERR (DESIGN.md 7.3 "Error
sources"): all four outputs against the CPU oracle and the exact (longdouble) evaluator -- live at d = 65, from
the committed fixture tests/golden/tiled_err.npz (tests/golden/make_golden_tiled_err.py) for the slow cases.

Tolerances: the tiled suite's for F and F_dx (tests/test_gpu_tiled.py _assert_fid), the dense suite's error
tiers (tests/test_gpu_dense.py _assert_err)
  F_d2err     <= 1e-6 max|ref| + 1e-7
  F_d2err_dx  <= 1e-5 max|ref| + 1e-7
against the oracle and against the exact value, and, as a condition on the input, the oracle alone within half
the tier of the exact value.
"""
import functools
import os
import re

import numpy as np
import pytest

from robustgrape_amd import synthetic as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T2E, T2E_ABS = 1e-6, 1e-7
T3E, T3E_ABS = 1e-5, 1e-7
SLAB_ITEMS, BUDGET, SLAB_IMAGES = 1024, 6 << 30, 9  # grape_plan_build.hip: kTiledSlabItems, kTiledBudgetBytes, ...


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _problem(d, ntimes, nerr, phase, scale=1.0):
    x = S.dense_x(ntimes, seed=500 + ntimes)
    fp = S.dense_error_problem(d, ntimes, rank=16, scale=scale, nerr=nerr, phase=phase)
    return fp, (np.concatenate([x, [0.7]]) if phase else x)


def _assert_tier(test, name, got, ref, exact, rel, floor):
    from tests.parity_log import record
    got, ref, exact = np.asarray(got), np.asarray(ref), np.asarray(exact)
    assert got.shape == ref.shape == exact.shape, (name, got.shape, ref.shape)
    se, sr = float(np.max(np.abs(exact))), float(np.max(np.abs(ref)))
    noise = float(np.max(np.abs(ref - exact)))
    ee, er = float(np.max(np.abs(got - exact))), float(np.max(np.abs(got - ref)))
    record(test + "_oracle_vs_exact", name, noise, se, 0.5 * (rel * se + floor))
    record(test + "_vs_exact", name, ee, se, rel * se + floor)
    record(test, name, er, sr, rel * sr + floor)
    print(f"{test}: {name} vs exact {ee:.3e} (tier {rel * se + floor:.2e}), vs oracle {er:.3e} "
          f"(tier {rel * sr + floor:.2e}), oracle vs exact {noise:.2e}")
    assert noise <= 0.5 * (rel * se + floor), ("oracle vs exact", name, noise)
    assert ee <= rel * se + floor, ("vs exact", name, ee, se)
    assert er <= rel * sr + floor, ("vs oracle", name, er, sr)


def _assert_all(test, out, ref, exact):
    from tests.test_gpu_tiled import _assert_fid
    _assert_fid(test, out[0], out[1], float(ref[0]), ref[1], float(exact[0]), exact[1])
    _assert_tier(test, "F_d2err", out[2], ref[2], exact[2], T2E, T2E_ABS)
    _assert_tier(test, "F_d2err_dx", out[3], ref[3], exact[3], T3E, T3E_ABS)


@pytest.mark.parametrize("d,ntimes,nerr,phase", [(65, 1, 1, False), (65, 5, 2, True)])
def test_tiled_error_outputs_match_live_oracle_and_exact(d, ntimes, nerr, phase):
    """One chunk of one step (no prefix, no B update; P = 80 != d), then a chunk remainder with the carries, two
    sources and the target rows of F_d2err_dx -- through the public function, which retries with the option."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_fidelity_and_derivatives
    fp, x = _problem(d, ntimes, nerr, phase)
    ref = O.calculate_fidelity_and_derivatives(fp, x)
    exact = E.fidelity_and_derivatives(fp, x, nparam=2)
    out = calculate_fidelity_and_derivatives(fp, x)
    assert out[2].shape == (nerr,) and out[3].shape == (len(x), nerr)
    _assert_all(f"tiled_err_live_d{d}_nt{ntimes}", out, ref, exact)


@functools.lru_cache(maxsize=1)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "tiled_err.npz"), allow_pickle=False))


@pytest.mark.parametrize("case", range(4))
def test_tiled_error_outputs_match_golden(case):
    """81 levels with a last chunk of one step; P = d = 128 with the x_add target; d = 113 at Taylor 8 (weights in
    the first tile only); d = 96 at scale 1.75 (|A|_1 = 0.88 .. 1.28): steps with one squaring, shared by every
    variant of the step, beside steps with none (at scale 2.0 the oracle's own F_dx distance was 0.92 of half the
    tier, above the 0.75 a case is kept at; make_golden_tiled_err.py)."""
    from robustgrape_amd import calculate_fidelity_and_derivatives
    g = _golden()
    d, ntimes, nerr, phase = (int(v) for v in g["cases"][case])
    fp, x = _problem(d, ntimes, nerr, bool(phase), float(g["scales"][case]))
    assert np.array_equal(x, g[f"x{case}"])
    out = calculate_fidelity_and_derivatives(fp, x)
    names = ("F", "F_dx", "F_d2err", "F_d2err_dx")
    _assert_all(f"tiled_err_golden_d{d}_nt{ntimes}", out, [g[f"{n}{case}"] for n in names],
                [g[f"{n}_exact{case}"] for n in names])


def test_the_public_function_retries_with_the_option_and_returns_the_reference_shapes():
    from robustgrape_amd import _capi, calculate_fidelity_and_derivatives
    from robustgrape_amd.engine import GrapePlan
    fp, x = _problem(65, 2, 2, True)
    with pytest.raises(_capi.GrapeError, match="error sources"):
        GrapePlan(fp, nparam=2, max_batch=1)
    F, Fdx, d2, d2dx = calculate_fidelity_and_derivatives(fp, x)
    assert np.isfinite(F) and Fdx.shape == (len(x),) and d2.shape == (2,) and d2dx.shape == (len(x), 2)
    assert np.all(np.isfinite(d2)) and np.all(np.isfinite(d2dx))


def test_without_error_sources_the_option_changes_nothing():
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    fp, x = _problem(65, 5, 0, True)
    outs = []
    for opts in (0, OPT_TILED_ERR):
        plan = GrapePlan(fp, nparam=2, max_batch=1, options=opts)
        outs.append(plan.fidelity_grad(x[None, :]))
        plan.close()
    assert outs[1][2].shape == (1, 0) and outs[1][3].shape == (1, len(x), 0)
    assert np.all(np.isfinite(outs[0][1]))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def _equal4(a, b):
    return all(np.all(np.isfinite(u)) and np.array_equal(u, v) for u, v in zip(a, b))


def test_tiled_error_batch_equals_single():
    """5 in one pass against 2 + 2 + 1: bitwise on all four outputs."""
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    fp = S.dense_error_problem(96, 6, rank=16, nerr=2)
    X = np.stack([S.dense_x(6, seed=s) for s in range(5)])
    plan = GrapePlan(fp, nparam=2, max_batch=5, options=OPT_TILED_ERR)
    a = plan.fidelity_grad(X)
    plan.close()
    one = GrapePlan(fp, nparam=2, max_batch=2, options=OPT_TILED_ERR)
    b = one.fidelity_grad(X)
    one.close()
    assert a[2].shape == (5, 2) and a[3].shape == (5, 12, 2) and _equal4(a, b)


def test_tiled_error_slab_seam_in_mid_chunk():
    """d = 65 (P = 80): the error plan's slab is 1 024 steps (np + 1 held images beside the nine of a plain plan), so
    147 evaluations of N_t = 7 are 1 029 steps: the second slab starts at step 2 of evaluation 146, the last of its
    first chunk (L = 3), not a chunk start, so its local frames take Q_{k-1}.  Bitwise the one-evaluation passes;
    the evaluation on the seam against the oracle and the exact value (from the fixture)."""
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    d, nt, nb, npar = 65, 7, 147, 2
    slab = min(SLAB_ITEMS, (BUDGET // 4) // ((SLAB_IMAGES + npar + 1) * 2 * 80 * 80 * 8))
    assert slab < nb * nt < slab + nt and (slab % nt) % 3 != 0
    fp = S.dense_error_problem(d, nt, rank=16, nerr=1)
    X = np.stack([S.dense_x(nt, seed=900 + s) for s in range(nb)])
    g = _golden()  # case 4: the evaluation on the seam
    assert [int(v) for v in g["cases"][4]] == [d, nt, 1, 0]
    X[146] = g["x4"]
    plan = GrapePlan(fp, nparam=npar, max_batch=nb, options=OPT_TILED_ERR)
    a = plan.fidelity_grad(X)
    plan.close()
    one = GrapePlan(fp, nparam=npar, max_batch=1, options=OPT_TILED_ERR)
    b = one.fidelity_grad(X)
    one.close()
    assert _equal4(a, b)
    names = ("F", "F_dx", "F_d2err", "F_d2err_dx")
    _assert_all("tiled_err_seam_d65_nt7", [float(a[0][146])] + [v[146] for v in a[1:]], [g[f"{n}4"] for n in names],
                [g[f"{n}_exact4"] for n in names])


def test_tiled_error_device_call_is_the_host_call():
    import torch

    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    fp = S.dense_error_problem(80, 4, rank=16, nerr=1)
    X = np.stack([S.dense_x(4, seed=40 + s) for s in range(3)])
    plan = GrapePlan(fp, nparam=2, max_batch=3, options=OPT_TILED_ERR)
    try:
        dev = torch.device("cuda", 0)
        nan = lambda *sh: torch.full(sh, float("nan"), dtype=torch.float64, device=dev)
        Xd = torch.as_tensor(np.ascontiguousarray(X), device=dev)
        F, Fdx, d2, d2dx = nan(3), nan(*X.shape), nan(3, 1), nan(3, 1, X.shape[1])
        torch.cuda.synchronize()
        plan.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), Fdx.data_ptr(), 3, d2.data_ptr(), d2dx.data_ptr())
        plan.synchronize()
        host = plan.fidelity_grad(X)
    finally:
        plan.close()
    devs = (F.cpu().numpy(), Fdx.cpu().numpy(), d2.cpu().numpy(), d2dx.cpu().numpy().transpose(0, 2, 1))
    assert _equal4(host, devs)


def test_a_problem_whose_one_evaluation_exceeds_the_budget_is_refused_with_the_byte_counts():
    """d = 128, N_t = 4 096, np = 2, ne = 2: 8 local-frame images per step are 8 GB per evaluation, above the plan's
    6 GB; the check precedes every allocation."""
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    with pytest.raises(_capi.GrapeError, match=r"GRAPE_ERR_ALLOC: tiled engine: one evaluation needs \d+ bytes") as ei:
        GrapePlan(S.dense_error_problem(128, 4096, rank=16, nerr=2), nparam=2, max_batch=1, options=OPT_TILED_ERR)
    need, budget = (int(v) for v in re.findall(r"\d{6,}", str(ei.value)))
    assert budget == BUDGET and need > 8 * 4096 * 2 * 128 * 128 * 8


def test_an_option_plan_refuses_the_analysis_entry_points_and_the_slices():
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    d, nt = 65, 2
    plan = GrapePlan(S.dense_error_problem(d, nt, rank=16, nerr=1), nparam=2, max_batch=1, options=OPT_TILED_ERR)
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
        _, _, d2, _ = plan.fidelity_grad(x[None, :])  # the plan still serves what it serves
        assert np.isfinite(d2[0, 0])
    finally:
        plan.close()
