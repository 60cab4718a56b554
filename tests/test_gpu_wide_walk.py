"""The wide pass (csrc/grape_walk.hpp "The wide pass").

A rank-one merged plan serves device-resident calls (fidelity_grad_device_async) of at least
W = max_batch x nchunks evaluations in passes of W with one lane per evaluation over all N_t steps: a forward
state walk psi = U e_c, the head (alpha per sector), a time-reversed gradient walk from psi_N and
phi_N = conj(alpha) e_c -- no chunk totals, no carries, no scan.  What is left of a call below W runs the
chunked passes; GRAPE_OPT_NO_WIDE keeps them for every count; sector_info()["wide"] reports W (0: none).

Every plan here is created as test_gpu_rank1_walk's (OPT_NO_EVAL1, scan_waves = 1) with GRAPE_GAUGE_NCHUNKS=4,
so that W is a few hundred evaluations.

Tolerances (the project's own):
  T1      1e-12 on F (the wide pass walks a vector chain, the chunked passes a matrix chain: rounding only)
  M1      1e-11 max|F_dx| + 1e-13   (test_gpu_gauge.test_merged_walks_match_per_class_walks; the recompute
                                     drift of psi_{k-1} = E_k^dag psi_k modelled at <= 3e-13 for N_t <= 512)
  T_EXACT 1e-9 max|F_dx| + 2e-11    (test_gpu_gauge.T_EXACT)
"""
import os

import numpy as np
import pytest

from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
M1 = (1e-11, 1e-13)
T_EXACT = (1e-9, 2e-11)
NCHUNKS = 4
W_WEIGHTED = np.diag([1.0, 2.0, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
W_TWO_LEVELS = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("GRAPE_GAUGE_NCHUNKS", str(NCHUNKS))  # (read at plan creation)


def _wide(nt, max_batch):
    """W of a plan whose chunk count was forced to NCHUNKS (the engine's L and chunk count)."""
    L = -(-nt // min(NCHUNKS, nt))
    return max_batch * -(-nt // L)


def _run(fp, X, max_batch, options=0, profile=False, repeat=1):
    """(F, F_dx, sector_info, gradient-walk launches) of one device-resident call over X; repeat > 1: a list
    of (F, F_dx) of the same call made again."""
    import torch
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1
    pl = GrapePlan(fp, nparam=1, device=0, max_batch=max_batch, options=options | OPT_NO_EVAL1, scan_waves=1)
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        Xd = torch.as_tensor(np.ascontiguousarray(X), device="cuda:0")
        torch.cuda.synchronize()
        if profile:
            pl.set_profiling(True)
        outs = []
        for _ in range(repeat):
            F = torch.full((len(X),), float("nan"), dtype=torch.float64, device="cuda:0")
            G = torch.full(X.shape, float("nan"), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), len(X))
            pl.synchronize()
            outs.append((F.cpu().numpy(), G.cpu().numpy()))
        launches = pl.kernel_times()["k_walk_grad"][1] if profile else None
    finally:
        pl.close()
    if repeat > 1:
        return outs, info
    return outs[0][0], outs[0][1], info, launches


def _within(test, G, G0, tier):
    """every row of G within tier of G0, relative to the row's max|G0|"""
    err = np.max(np.abs(G - G0), axis=-1)
    scale = np.max(np.abs(G0), axis=-1)
    bound = tier[0] * scale + tier[1]
    worst = int(np.argmax(np.atleast_1d(err / bound)))
    print(f"{test}: max|dF_dx| {float(np.max(err)):.3e} (worst row {worst}: {float(np.atleast_1d(err)[worst]):.3e} "
          f"of bound {float(np.atleast_1d(bound)[worst]):.3e}, scale {float(np.atleast_1d(scale)[worst]):.3e})")
    assert np.all(err <= bound), (test, float(np.max(err / bound)))


def _batch(nt, n, seed):
    X = np.stack([P.random_x(nt, seed + s, small=(s % 2 == 0)) for s in range(n)])
    X[1, :nt] = np.random.default_rng(seed).uniform(-40.0, 40.0, size=nt)  # large phases
    return X


def _c2_golden():
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c2.npz"),
                        allow_pickle=False))


@pytest.mark.parametrize("max_batch", [100, 40])  # W = 400: two workgroups, the second ragged; 160: one, partly filled
@pytest.mark.parametrize("nt", [1, 3, 70, 128])   # 70: a 6-step last F_dx tile
def test_wide_pass_matches_chunked_passes(nt, max_batch):
    """The same plan with and without GRAPE_OPT_NO_WIDE over 2 W + 37 evaluations: two wide passes and a
    chunked remainder against three chunked passes.  F within T1, F_dx within M1, the 37 remainder rows bit
    for bit; the gradient-walk launches counted through the profiling events."""
    from robustgrape_amd.operators import OPT_NO_WIDE
    W = _wide(nt, max_batch)
    f = P.full9_problem(nt)
    X = _batch(nt, 2 * W + 37, 4100 + nt)
    F1, G1, i1, n1 = _run(f, X, max_batch, profile=True)
    F0, G0, i0, n0 = _run(f, X, max_batch, OPT_NO_WIDE, profile=True)
    assert i1["rank1"] is True and i0["rank1"] is True, (i1, i0)
    assert i1["wide"] == W and i0["wide"] == 0, (i1, i0, W)
    nchunked = -(-(2 * W + 37) // max_batch)
    assert n1 == 2 + 1 and n0 == nchunked, (n1, n0)
    print(f"wide_vs_chunked_nt{nt}_mb{max_batch}: max|dF| {float(np.max(np.abs(F1 - F0))):.2e}")
    assert float(np.max(np.abs(F1 - F0))) <= T1
    _within(f"wide_vs_chunked_nt{nt}_mb{max_batch}", G1, G0, M1)
    assert np.array_equal(F1[2 * W:], F0[2 * W:]) and np.array_equal(G1[2 * W:], G0[2 * W:])


def test_wide_pass_at_the_c2_golden():
    """N_t = 512 with the C2 golden x as a row of a wide pass: against the golden at its tier in
    test_rank_one_walk_at_the_c2_golden, and against the chunked passes within M1."""
    from robustgrape_amd.operators import OPT_NO_WIDE
    g2 = _c2_golden()
    f = P.full9_problem(512)
    W = _wide(512, 64)
    X = _batch(512, W, 5200)
    X[5] = g2["x"]
    F1, G1, i1, _ = _run(f, X, 64)
    F0, G0, i0, _ = _run(f, X, 64, OPT_NO_WIDE)
    assert i1["wide"] == W and i0["wide"] == 0, (i1, i0)
    print(f"wide_c2: max|dF| {float(np.max(np.abs(F1 - F0))):.2e}, golden |dF| {abs(F1[5] - float(g2['F'])):.2e}")
    assert float(np.max(np.abs(F1 - F0))) <= T1
    _within("wide_vs_chunked_c2", G1, G0, M1)
    assert abs(F1[5] - float(g2["F"])) <= T1
    _within("wide_c2_golden", G1[5], g2["F_dx"], (1e-7, 1e-9))


def test_wide_pass_against_the_exact_forward_difference():
    """full9_problem(96), small and large controls, and the first 96 steps of the C2 golden pulse as rows of a
    wide pass: F_dx of the controls against the reference's forward difference evaluated in longdouble
    (oracle/grape_exact.py), within T_EXACT."""
    from oracle import grape_exact as E
    nt = 96
    g2 = _c2_golden()
    f = P.full9_problem(nt)
    W = _wide(nt, 40)
    X = _batch(nt, W, 6100)
    X[2] = np.concatenate([g2["x"][:nt], g2["x"][-1:]])
    assert P.max_step_norm(f, X[:3]) < 1.0  # (no squarings in the longdouble evaluator: T_EXACT's floor as it stands)
    F, G, info, _ = _run(f, X, 40)
    assert info["wide"] == W, info
    for b in (0, 1, 2):
        Fe, ge = E.fidelity_and_gradient(f, X[b])
        print(f"wide_vs_exact_{b}: |dF| {abs(F[b] - Fe):.2e}")
        assert abs(F[b] - Fe) <= T1
        _within(f"wide_vs_exact_{b}", G[b][:nt], ge[:nt], T_EXACT)


def _against_oracle(test, fp, X, F, G, rows):
    """test_gpu_gauge's oracle check: F at T1; F_dx at the FD tier of the rows' step norms plus the
    oracle's own measured distance from the exact forward difference."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    for b in rows:
        F0, g0 = O.calculate_fidelity_and_derivatives(fp, X[b])[:2]
        Fe, ge = E.fidelity_and_gradient(fp, X[b])
        print(f"{test}_{b}: |dF| {abs(F[b] - F0):.2e}")
        assert abs(F[b] - F0) <= T1
        t2, t2a = P.fd_tier(fp, X[b])
        _within(f"{test}_{b}", G[b], np.asarray(g0), (t2, t2a + float(np.max(np.abs(np.asarray(g0) - ge)))))


def test_second_weighted_level_takes_no_wide_pass():
    """|rr> weighted beside |11>: no rank-one walk, hence no wide pass; the call matches the oracle."""
    nt = 96
    f = P.full9_problem(nt).replace(projector=W_TWO_LEVELS)
    X = _batch(nt, _wide(nt, 40), 8300)
    F, G, info, _ = _run(f, X, 40)
    assert info["rank1"] is False and info["wide"] == 0, info
    _against_oracle("wide_ineligible", f, X, F, G, (0, 1))


def test_non_twin_class_stays_wide():
    """GRAPE_OPT_NO_TWIN: class B's two sectors each walk their own (psi, phi) over their own propagator."""
    from robustgrape_amd.operators import OPT_NO_TWIN, OPT_NO_WIDE
    nt = 70
    f = P.full9_problem(nt)
    W = _wide(nt, 40)
    X = _batch(nt, W, 9300)
    F1, G1, i1, _ = _run(f, X, 40, OPT_NO_TWIN)
    F0, G0, i0, _ = _run(f, X, 40, OPT_NO_TWIN | OPT_NO_WIDE)
    assert i1["wide"] == W and not any(i1["twin"]) and i0["wide"] == 0, (i1, i0)
    assert float(np.max(np.abs(F1 - F0))) <= T1
    _within("wide_non_twin", G1, G0, M1)


def test_weighted_projector_stays_wide():
    """Weights other than 1 only scale alpha."""
    nt = 96
    f = P.full9_problem(nt).replace(projector=W_WEIGHTED)
    W = _wide(nt, 40)
    X = _batch(nt, W, 7300)
    F, G, info, _ = _run(f, X, 40)
    assert info["wide"] == W, info
    _against_oracle("wide_weighted", f, X, F, G, (0, 1))


def test_wide_call_repeats_its_bits():
    nt = 70
    f = P.full9_problem(nt)
    W = _wide(nt, 40)
    (a, b), info = _run(f, _batch(nt, W + 5, 1300), 40, repeat=2)
    assert info["wide"] == W, info
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.any(np.isnan(a[0])) and not np.any(np.isnan(a[1]))


def test_count_just_below_w_runs_no_wide_pass():
    """W - 1 evaluations: the chunked passes, bit for bit those of GRAPE_OPT_NO_WIDE."""
    from robustgrape_amd.operators import OPT_NO_WIDE
    nt = 70
    f = P.full9_problem(nt)
    W = _wide(nt, 40)
    X = _batch(nt, W - 1, 2300)
    F1, G1, i1, n1 = _run(f, X, 40, profile=True)
    F0, G0, i0, n0 = _run(f, X, 40, OPT_NO_WIDE, profile=True)
    assert i1["wide"] == W and i0["wide"] == 0, (i1, i0)
    assert n1 == n0 == -(-(W - 1) // 40), (n1, n0)
    assert np.array_equal(F1, F0) and np.array_equal(G1, G0)
