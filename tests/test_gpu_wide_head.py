"""The wide pass's head and difference weights.

k_wide_head (csrc/grape_projector.hip) serves a wide pass with one lane per evaluation: F, alpha per sector and the
x_add column of F_dx from U_cc of three sectors, psi_N passed evaluation-minor between the walks.  The wide
gradient walk takes its difference weights from a per-plan base (csrc/grape_fd_weight.hpp, grape_walk_merged.hpp
wide_fd_weights): a step whose fl(x_k + eps) - x_k is close to eps adds a first-order term to the weights at
a eps, any other step takes cis_m1 and the recurrence as the chunked walks do at every step.

Plans as test_gpu_wide_walk.py makes them (GRAPE_GAUGE_NCHUNKS = 4, OPT_NO_EVAL1, scan_waves = 1), so that a wide
pass is a few hundred evaluations.  The chunked passes (GRAPE_OPT_NO_WIDE) keep the row-group head and the
per-step weights, so wide against chunked on the same rows sets the new forms against the old ones.  Every call's
output buffers arrive full of NaN with a guard row behind them (_run).

Tolerances (the project's own, test_gpu_wide_walk.py):
  T1      1e-12 on F
  M1      1e-11 max|F_dx| + 1e-13 per row, the x_add column included
  T_EXACT 1e-9 max|F_dx| + 2e-11 against the exact forward difference (oracle/grape_exact.py)

Rows: small controls (2 pi 0.001 U, the bench's range), large ones (2 pi U), one row of controls in +-40, and in
the exact and determinism checks one row of controls near 8e7, where x + eps rounds to x + 1.49e-8: the guard
hands every step of that row to the per-step form, in a wave whose other lanes take the fast one.
"""
import numpy as np
import pytest

from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
M1 = (1e-11, 1e-13)
T_EXACT = (1e-9, 2e-11)
NCHUNKS = 4
W_WEIGHTED = np.diag([1.0, 2.0, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
X_OFF_GRID = 8.05e7  # 2^26 < x < 2^27: a unit in the last place of 1.49e-8, so fl(x + 1e-8) - x = 1.49e-8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("GRAPE_GAUGE_NCHUNKS", str(NCHUNKS))  # (read at plan creation)


def _wide(nt, max_batch):
    L = -(-nt // min(NCHUNKS, nt))
    return max_batch * -(-nt // L)


def _run(fp, X, max_batch, options=0, repeat=1):
    """[(F, F_dx)] of `repeat` device-resident calls over X and the plan's sector_info.  The output buffers hold one
    row more than the call is given and arrive full of NaN: no NaN may be left in the caller's rows, and the
    row after them must still be NaN."""
    import torch
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1
    pl = GrapePlan(fp, nparam=1, device=0, max_batch=max_batch, options=options | OPT_NO_EVAL1, scan_waves=1)
    try:
        info = pl.sector_info()
        n, nx = X.shape
        Xd = torch.as_tensor(np.ascontiguousarray(X), device="cuda:0")
        outs = []
        for _ in range(repeat):
            F = torch.full((n + 1,), float("nan"), dtype=torch.float64, device="cuda:0")
            G = torch.full((n + 1, nx), float("nan"), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), n)
            pl.synchronize()
            F, G = F.cpu().numpy(), G.cpu().numpy()
            assert not np.any(np.isnan(F[:n])) and not np.any(np.isnan(G[:n])), "a NaN left in the caller's rows"
            assert np.isnan(F[n]) and np.all(np.isnan(G[n])), "a write past the caller's rows"
            outs.append((F[:n], G[:n]))
    finally:
        pl.close()
    return outs, info


def _within(test, G, G0, tier):
    err = np.max(np.abs(G - G0), axis=-1)
    scale = np.max(np.abs(G0), axis=-1)
    bound = tier[0] * scale + tier[1]
    print(f"{test}: max|dF_dx| {float(np.max(err)):.3e}, worst err / bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound), (test, float(np.max(err / bound)))


def _batch(nt, n, seed):
    X = np.stack([P.random_x(nt, seed + s, small=(s % 2 == 0)) for s in range(n)])
    X[1, :nt] = np.random.default_rng(seed).uniform(-40.0, 40.0, size=nt)
    return X


def _wide_against_chunked(test, fp, X, max_batch, options=0, nrem=0):
    from robustgrape_amd.operators import OPT_NO_WIDE
    W = len(X) - nrem
    (wide,), iw = _run(fp, X, max_batch, options)
    (chunked,), ic = _run(fp, X, max_batch, options | OPT_NO_WIDE)
    assert iw["rank1"] is True and iw["wide"] == W and ic["wide"] == 0, (iw, ic, W)
    dF = float(np.max(np.abs(wide[0] - chunked[0])))
    print(f"{test}: max|dF| {dF:.2e}")
    assert dF <= T1
    _within(test, wide[1], chunked[1], M1)
    if nrem:  # what is left of the call below W runs the chunked passes in both plans
        assert np.array_equal(wide[0][W:], chunked[0][W:]) and np.array_equal(wide[1][W:], chunked[1][W:])
    return iw


@pytest.mark.parametrize("max_batch", [40, 100])  # W = 160: one workgroup, partly filled; 400: two, the second ragged
@pytest.mark.parametrize("nt", [1, 3, 70])        # 70: a 6-step last tile
def test_wide_pass_matches_chunked_passes(nt, max_batch):
    """W + 5 rows: one wide pass against the chunked passes (F at T1, F_dx at M1), the 5 remainder rows bit for bit."""
    W = _wide(nt, max_batch)
    _wide_against_chunked(f"head_wide_vs_chunked_nt{nt}_mb{max_batch}", P.full9_problem(nt), _batch(nt, W + 5, 4700 + nt),
                          max_batch, nrem=5)


def test_weighted_projector_and_non_twin_forms():
    from robustgrape_amd.operators import OPT_NO_TWIN
    nt = 70
    W = _wide(nt, 40)
    X = _batch(nt, W, 7700)
    _wide_against_chunked("head_weighted", P.full9_problem(nt).replace(projector=W_WEIGHTED), X, 40)
    info = _wide_against_chunked("head_non_twin", P.full9_problem(nt), X, 40, OPT_NO_TWIN)
    assert not any(info["twin"]), info


@pytest.mark.parametrize("case", ["swap-A", "swap-B1", "reversed", "stiff"])
def test_family_cases(case):
    """General charges (swap-A, swap-B1, reversed: one weight per level pair from the runtime charge differences, a
    weighted level other than the first, c differing between class B's sectors), a control scaled by a = 0.5
    (reversed) and stiff propagators."""
    nt = 70
    W = _wide(nt, 40)
    info = _wide_against_chunked(f"head_family_{case}", P.gauge_family_problem(case, nt)[0], _batch(nt, W, 8700), 40)
    want = P.GAUGE_FAMILY[case][2]
    if want is not None:
        assert (info["twin"][1], all(info["ladder"])) == want, info


def test_wide_pass_against_the_exact_forward_difference():
    """full9_problem(96): a small row, a row in +-40 and a row the guard refuses, against the reference's forward
    difference evaluated in longdouble from the same fl(x + eps)."""
    from oracle import grape_exact as E
    nt = 96
    f = P.full9_problem(nt)
    W = _wide(nt, 40)
    X = _batch(nt, W, 6700)
    X[3, :nt] = X_OFF_GRID + np.random.default_rng(6703).uniform(-1.0e3, 1.0e3, size=nt)
    eps = f.unitary_problem.eps
    assert np.all(np.abs(((X[3, :nt] + eps) - X[3, :nt]) - eps) > 0.4 * eps)  # (every step of the row is refused)
    assert np.max(np.abs(((X[:2, :nt] + eps) - X[:2, :nt]) - eps)) < 1.0e-6 * eps  # (rows 0, 1: the fast form)
    assert P.max_step_norm(f, X[:4]) < 1.0  # (no squarings in the longdouble evaluator: T_EXACT's floor as it stands)
    (out,), info = _run(f, X, 40)
    assert info["wide"] == W, info
    F, G = out
    for b in (0, 1, 3):
        Fe, ge = E.fidelity_and_gradient(f, X[b])
        print(f"head_wide_vs_exact_{b}: |dF| {abs(F[b] - Fe):.2e}")
        assert abs(F[b] - Fe) <= T1
        _within(f"head_wide_vs_exact_{b}", G[b][:nt], ge[:nt], T_EXACT)


def test_lanes_and_calls_repeat_their_bits():
    """The same controls at lane 0 and at the last lane of a pass (a fast row, and a refused row beside fast ones)
    give equal bits; a repeated call repeats its bits."""
    nt = 70
    f = P.full9_problem(nt)
    W = _wide(nt, 100)
    X = _batch(nt, W, 1700)
    X[W - 1] = X[0]
    X[2, :nt] = X_OFF_GRID + np.random.default_rng(1703).uniform(-1.0e3, 1.0e3, size=nt)
    X[W - 2] = X[2]
    (a, b), info = _run(f, X, 100, repeat=2)
    assert info["wide"] == W, info
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for i, j in ((0, W - 1), (2, W - 2)):
        assert a[0][i] == a[0][j] and np.array_equal(a[1][i], a[1][j]), (i, j)
