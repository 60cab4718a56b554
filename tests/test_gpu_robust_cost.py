"""grape_robust_cost (the fused optimiser cost, csrc/grape_lbfgs.hip k_robust_cost) on synthetic
engine outputs against a longdouble restatement (tests/lbfgs_ref.py robust_cost_ref): step counts
on both sides of every strided trip and of the end stencils, every regulariser kind and mix, tail
entries, with and without error sources, coefficients of order 1."""
import ctypes

import numpy as np
import pytest
import torch

from tests import lbfgs_ref as LR
from tests import parity_log

pytestmark = pytest.mark.gpu
INVALID = -1
R = 3
# (reg_kind per control, nadd, nerr): every kind alone, all-0, a 0 between two regularised controls
MIXES = [((1,), 0, 0), ((2,), 1, 2), ((0,), 2, 0), ((1, 2), 1, 2), ((2, 0), 0, 0), ((0, 0), 0, 2),
         ((2, 0, 1), 2, 2), ((1, 2, 2), 0, 0), ((0, 0, 0), 1, 2)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _inputs(nt, kinds, na, ne, seed):
    npar = len(kinds)
    nx = npar * nt + na
    rng = np.random.default_rng(seed)
    X = rng.uniform(-np.pi, np.pi, size=(R, nx))  # rough rows
    k = np.arange(nt)
    for p in range(npar):  # row 1 smooth: the differences cancel
        X[1, p:npar * nt:npar] = (p + 1) * np.sin(2 * np.pi * k / nt + p)
    return dict(X=X, F=rng.uniform(size=R), Fdx=rng.normal(size=(R, nx)), Fd2=rng.normal(size=(R, max(ne, 1))),
                Fd2dx=rng.normal(size=(R, max(ne, 1), nx)), ce=rng.uniform(0.5, 2, size=ne + 1),
                c1=rng.uniform(0.5, 2, size=npar), c2=rng.uniform(0.5, 2, size=npar),
                kind=np.asarray(kinds, dtype=np.int32))


def _call(rows, npar, nt, na, ne, t, cost, grad, null_err=False):
    from robustgrape_amd import _capi
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    err = [ctypes.c_void_p(None)] * 3 if null_err else [p(t["Fd2"]), p(t["Fd2dx"]), p(t["ce"])]
    code = _capi.lib().grape_robust_cost(rows, npar, nt, na, ne, p(t["X"]), p(t["F"]), p(t["Fdx"]), err[0], err[1],
                                         err[2], p(t["c1"]), p(t["c2"]), p(t["kind"]), p(cost), p(grad),
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return code


@pytest.mark.parametrize("mix", range(len(MIXES)))
@pytest.mark.parametrize("nt", [4, 5, 255, 256, 257, 513, 4096])
def test_fused_cost_matches_longdouble_reference(nt, mix):
    """|dev - ref| <= 64 * 2^-52 * S for the cost and every gradient entry, S the reference's own
    expression with absolute addends (16 serial adds per thread at 4 096 steps, the reduction
    tree, 2-ulp cos / sin); a wrong stencil coefficient or a missed end point is off by order 1."""
    kinds, na, ne = MIXES[mix]
    h = _inputs(nt, kinds, na, ne, seed=1000 * mix + nt)
    t = {k: torch.as_tensor(v, device="cuda") for k, v in h.items()}
    nx = len(kinds) * nt + na
    cost = torch.full((R,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((R, nx), float("nan"), dtype=torch.float64, device="cuda")
    assert _call(R, len(kinds), nt, na, ne, t, cost, grad, null_err=ne == 0) == 0
    cost, grad = cost.cpu().numpy(), grad.cpu().numpy()
    worst_c = worst_g = 0.0
    for r in range(R):
        c, g, sc, sg = LR.robust_cost_ref(h["X"][r], h["F"][r], h["Fdx"][r], h["Fd2"][r, :ne], h["Fd2dx"][r, :ne],
                                          h["ce"][:ne], h["c1"], h["c2"], kinds, nt, na)
        ec = float(abs(LR.LD(cost[r]) - c) / sc)
        eg = float(np.max(np.abs(grad[r].astype(LR.LD) - g) / sg))
        worst_c, worst_g = max(worst_c, ec), max(worst_g, eg)
        if na:  # the tail receives no regulariser term: -F_dx and the error term only
            tail = -h["Fdx"][r, nx - na:] + sum(2 * h["ce"][e] * h["Fd2"][r, e] * h["Fd2dx"][r, e, nx - na:]
                                                for e in range(ne))
            assert np.max(np.abs(grad[r, nx - na:] - tail)) <= 8 * LR.EPS * float(np.max(sg[nx - na:]))
    name = f"robust_cost nt={nt} kinds={kinds} nadd={na} nerr={ne}"
    print(f"{name}: cost {worst_c / LR.EPS:.2f} grad {worst_g / LR.EPS:.2f} (units of 2^-52 S, bound 64)")
    parity_log.record(name, "cost / S", worst_c, 1.0, 64 * LR.EPS)
    parity_log.record(name, "grad / S", worst_g, 1.0, 64 * LR.EPS)
    assert worst_c <= 64 * LR.EPS and worst_g <= 64 * LR.EPS


def test_fused_cost_limits():
    """3 and 4 097 steps are refused; no rows is OK and writes nothing."""
    for nt in (3, 4097):
        h = _inputs(nt, (1, 2), 1, 2, seed=nt)
        t = {k: torch.as_tensor(v, device="cuda") for k, v in h.items()}
        cost = torch.full((R,), float("nan"), dtype=torch.float64, device="cuda")
        grad = torch.full((R, 2 * nt + 1), float("nan"), dtype=torch.float64, device="cuda")
        assert _call(R, 2, nt, 1, 2, t, cost, grad) == INVALID
        assert bool(torch.isnan(cost).all()) and bool(torch.isnan(grad).all())
    h = _inputs(8, (1, 2), 1, 2, seed=8)
    t = {k: torch.as_tensor(v, device="cuda") for k, v in h.items()}
    cost = torch.full((R,), float("nan"), dtype=torch.float64, device="cuda")
    grad = torch.full((R, 17), float("nan"), dtype=torch.float64, device="cuda")
    assert _call(0, 2, 8, 1, 2, t, cost, grad) == 0
    assert bool(torch.isnan(cost).all()) and bool(torch.isnan(grad).all())


def test_three_step_problem_is_not_fused():
    """The fused launch needs four steps for its end stencils: a 3-step problem keeps the torch
    assembly, a 4-step one takes the kernel."""
    from robustgrape_amd import optimize as OPT
    from robustgrape_amd import regularization as REG
    from robustgrape_amd.types import FidelityRobustGRAPEParameters
    from tests import problems as P
    for nt, fused in ((3, False), (4, True)):
        params = FidelityRobustGRAPEParameters(
            x_initial=P.random_x(nt, 1), regularization_functions=[REG.regularization_cost_phase],
            regularization_coeff1=[1.0], regularization_coeff2=[1.0], error_source_coeff=[])
        cost = OPT.RobustCost(P.sym_problem(nt), params, nparam=1, max_batch=2)
        try:
            assert (cost._fused is not None) == fused
        finally:
            cost.close()
