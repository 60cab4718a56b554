"""The scalar optimiser reference (tests/lbfgs_ref.py) checked on the CPU before the GPU tests lean
on it: against lbfgs_batched's torch path on Rosenbrock, its own scenario table for coverage of
the line search's branches, and its regulariser against the oracle's."""
import numpy as np
import pytest
import torch

from oracle import grape_oracle as O
from robustgrape_amd import optimize as OPT
from tests import lbfgs_ref as LR


def _rosen_t(X, rows=None):
    a, b = X[:, :-1], X[:, 1:]
    f = torch.sum(100 * (b - a * a) ** 2 + (1 - a) ** 2, dim=1)
    g = torch.zeros_like(X)
    g[:, :-1] += -400 * a * (b - a * a) - 2 * (1 - a)
    g[:, 1:] += 200 * (b - a * a)
    return f, g


def _rosen(x):
    a, b = x[:-1], x[1:]
    g = np.zeros_like(x)
    g[:-1] += -400 * a * (b - a * a) - 2 * (1 - a)
    g[1:] += 200 * (b - a * a)
    return float(np.sum(100 * (b - a * a) ** 2 + (1 - a) ** 2)), g


def _cubics_agree(info, row):
    """The float64 and the longdouble cubic within 1e-14 of the bracket, plus one unit in the last
    place of a step length of order 1..4: a collapsing bracket next to a kept point at a = 1 gets
    narrower than 1e4 such units, where no two float64 evaluations can agree more closely."""
    return info["cubic_diff"] <= 1e-14 * info["width"] + LR.EPS * max(1.0, row.a_cur)


@pytest.mark.parametrize("m,steepest", [(10, False), (10, True), (3, False)])
def test_reference_follows_torch_path_on_rosenbrock(m, steepest):
    """R = 9, n = 6, seed 5, the first 20 iterations (later a rounding flip at |df| ~ 1e-15 may
    separate single rows): equal iterations, call counts and flags, minimisers to 1e-10.  m = 3
    wraps the ring buffer."""
    X0 = np.random.default_rng(5).uniform(-2, 2, size=(9, 6))
    res = OPT.lbfgs_batched(_rosen_t, torch.as_tensor(X0), m=m, iterations=20, steepest=steepest)
    wrapped = 0
    for r in range(9):
        row = LR.minimize(_rosen, X0[r], m=m, iterations=20, steepest=steepest)
        assert row.iters == int(res.iterations[r]) and row.f_calls == int(res.f_calls[r]), r
        flags = (row.gconv, row.fconv, row.xconv, row.lsfail)
        assert flags == tuple(int(getattr(res, k)[r]) for k in ("g_converged", "f_converged", "x_converged",
                                                               "ls_failed")), r
        assert np.max(np.abs(row.X - res.minimizer[r].numpy())) <= 1e-10, r
        assert abs(row.f - float(res.minimum[r])) <= 1e-10 * max(1.0, abs(row.f))
        wrapped += row.iters > m
    assert steepest or m == 10 or wrapped == 9


def test_scenario_table_covers_the_line_search():
    """The (f_t, phi'_t) table takes all eight transitions, the collapsed-bracket exit, a step
    without acceptance, ls_failed and both clamps of the cubic; the float64 and longdouble cubics
    agree on every trial (_cubics_agree).  In float64 the bracket of (1e6, 1e6) repeated is
    0.1^k rounded up, so it collapses at the 14th trial, not the 13th.
    No sequence reaches the bisection fallback, and none with finite values can: the discriminant
    is negative only if both slopes have one sign and the secant slope from lo to hi is below minus
    a third of their mean size; but hi either lies above lo or merely fails Armijo (its secant is
    above c1 phi'(0) = -1e-4 |phi'(0)|), and lo's slope is at least 0.9 |phi'(0)| in size, or lo
    would have been accepted."""
    seen, clamps, ends = set(), set(), set()
    for name, sc in LR.SCENARIOS.items():
        for n in (1, 513):
            row, infos = LR.run_scenario(name, n)
            assert [i["transition"] for i in infos] == sc["path"], name
            assert row.phase == 2, name
            assert all(not i["collapsed"] for i in infos[:-1])
            assert all(_cubics_agree(i, row) for i in infos), name
            assert not any(i["bisected"] for i in infos), name
            row.step()
            end = "accepted" if row.accepted else "moved" if not row.lsfail else "failed"
            assert end == sc["end"], name
            assert infos[-1]["collapsed"] == (end != "accepted"), name
            assert (row.iters, row.lsfail) == ((0, 1) if end == "failed" else (1, 0))
            if end == "failed":
                assert len(infos) == 14 and np.array_equal(row.X, np.zeros(n)) and row.f == 0.0
        seen |= {i["transition"] for i in infos}
        clamps |= {i["clamp"] for i in infos}
        ends.add(end)
    assert seen == set(LR.TRANSITIONS)
    assert {"lo", "hi"} <= clamps
    assert ends == {"accepted", "moved", "failed"}


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_exact_vectors(n):
    """The integer vectors' dot products are exact and sit in the second trip and the tail."""
    D = LR.exact_direction(n)
    for P in (-20, -19, 0, 3, 20000000):
        v = LR.exact_vector(P, D, salt=P % 7)
        assert float(np.dot(v, D)) == P == float(np.dot(v[::-1], D[::-1]))
        if n > 257:
            assert v[256] * D[256] + v[n - 1] * D[n - 1] == P and (P == 0 or v[n - 1] != 0)
        else:
            assert v[n - 1] * D[n - 1] == P


@pytest.mark.parametrize("m", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_generic_rows_have_margins(n, m):
    """The seeds the GPU tests use for random vectors (the quartic, rows 0..4, four iterations):
    every comparison the reference makes is wider than 1e-9 of its larger side, so a device whose
    dot products differ in the last bits must decide alike."""
    for r in range(5):
        w, c = LR.quartic(n, seed=r)
        x0 = LR.quartic_x0(n, r)
        log = []
        row = LR.minimize(LR.quartic_np(w, c), x0, m=m, iterations=4, g_tol=1e-12, log=log)
        assert row.iters == 4 and row.min_margin > 1e-9, (r, row.min_margin)
        assert all(_cubics_agree(i, row) for i in log)


@pytest.mark.parametrize("n", [4, 5, 257])
def test_regulariser_reference_matches_oracle(n):
    x = np.random.default_rng(n).uniform(-np.pi, np.pi, size=n)
    for kind, fn in ((1, O.regularization_cost), (2, O.regularization_cost_phase)):
        val, mag = LR.reg_ref(x, kind)
        for k, (a, s, b) in enumerate(zip(val, mag, fn(x))):
            err = np.max(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b)))
            assert err <= 16 * LR.EPS * float(np.max(s)), (kind, k, err)
            assert np.all(np.abs(a) <= s * (1 + 1e-15))
