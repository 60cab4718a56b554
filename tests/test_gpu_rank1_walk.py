"""The rank-one merged gradient walk (csrc/grape_walk.hpp merged_step_grad_r1).

With the diagonal head and exactly one projector-weighted level per sector, every sector block of M has
one non-zero row, M = e_c m^T, so the merged gradient walk carries psi = Q e_c and phi = Q conj(m)
instead of X = Q M Q^dag: the same F_dx, other roundings.  GRAPE_OPT_NO_RANK1 keeps the matrix walk,
sector_info()["rank1"] tells which one a plan runs.

Every plan here is created with OPT_NO_EVAL1 and one-wave scans (scan_waves = 1), the throughput
chunking, so that plans of a few hundred evaluations take the merged walks (asserted through
sector_info()["rank1"]: a plan that did not merge reports False).

Tolerances (the project's own):
  M1      1e-11 max|F_dx| + 1e-13   (test_gpu_gauge.test_merged_walks_match_per_class_walks)
  T_EXACT 1e-9 max|F_dx| + 2e-11    (test_gpu_gauge.T_EXACT; the steps of full9_problem(96) are below
                                     |dt H|_1 = 1, where the longdouble evaluator takes no squaring)
"""
import os

import numpy as np
import pytest

from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
M1 = (1e-11, 1e-13)
T_EXACT = (1e-9, 2e-11)
W_WEIGHTED = np.diag([1.0, 2.0, 1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
# a second weighted level inside the 3-level sector {11, (1r + r1) / sqrt 2, rr}: |rr> is level 8 of
# rydberg.py's basis |00>,|01>,|10>,|11>,|0r>,|r0>,|1r>,|r1>,|rr>
W_TWO_LEVELS = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0])


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _plan(fp, max_batch, options=0):
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1
    return GrapePlan(fp, nparam=1, device=0, max_batch=max_batch, options=options | OPT_NO_EVAL1, scan_waves=1)


def _run(fp, X, options=0, max_batch=None):
    """(F, F_dx, sector_info) of one plan over X."""
    pl = _plan(fp, max_batch or len(X), options)
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        F, G, _, _ = pl.fidelity_grad(X)
    finally:
        pl.close()
    return np.array(F), np.array(G), info


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


@pytest.mark.parametrize("nt,n,nchunks", [
    (1, 300, None), (3, 300, None),
    (70, 300, 4),     # 4 chunks of 18 steps: a ragged last chunk (16 steps) and a 2-step second F_dx tile
    (128, 300, None),
    (70, 3, 4),       # three evaluations: one partly filled workgroup
])
def test_rank_one_walk_matches_matrix_walk(nt, n, nchunks, monkeypatch):
    """The same plan with and without GRAPE_OPT_NO_RANK1: F bit for bit (the gradient walk does not
    touch it), F_dx within M1.  300 evaluations: a ragged last workgroup."""
    from robustgrape_amd.operators import OPT_NO_RANK1
    if nchunks:
        monkeypatch.setenv("GRAPE_GAUGE_NCHUNKS", str(nchunks))  # (read at plan creation)
    f = P.full9_problem(nt)
    X = _batch(nt, n, 4100 + nt)
    F1, G1, i1 = _run(f, X)
    F0, G0, i0 = _run(f, X, OPT_NO_RANK1)
    assert i1["rank1"] is True and i0["rank1"] is False, (i1, i0)
    assert np.array_equal(F1, F0)
    _within(f"rank1_vs_matrix_nt{nt}_n{n}", G1, G0, M1)


def test_rank_one_walk_at_the_c2_golden():
    """N_t = 512 with the C2 golden x inside the batch (as test_gpu_gauge.py has it): against the golden
    at its tier there, and against the matrix walk within M1."""
    from robustgrape_amd.operators import OPT_NO_RANK1
    g2 = _c2_golden()
    f = P.full9_problem(512)
    X = _batch(512, 300, 5200)
    X[5] = g2["x"]
    F1, G1, i1 = _run(f, X)
    F0, G0, i0 = _run(f, X, OPT_NO_RANK1)
    assert i1["rank1"] is True and i0["rank1"] is False, (i1, i0)
    assert np.array_equal(F1, F0)
    _within("rank1_vs_matrix_c2", G1, G0, M1)
    assert abs(F1[5] - float(g2["F"])) <= T1
    _within("rank1_c2_golden", G1[5], g2["F_dx"], (1e-7, 1e-9))


def test_rank_one_walk_against_the_exact_forward_difference():
    """full9_problem(96), small and large controls, and the first 96 steps of the C2 golden pulse (with
    its phase parameter) as a row: F_dx of the controls against the reference's forward difference
    evaluated in longdouble (oracle/grape_exact.py), within T_EXACT."""
    from oracle import grape_exact as E
    nt = 96
    g2 = _c2_golden()
    f = P.full9_problem(nt)
    X = _batch(nt, 300, 6100)
    X[2] = np.concatenate([g2["x"][:nt], g2["x"][-1:]])
    assert P.max_step_norm(f, X[:3]) < 1.0  # (no squarings in the longdouble evaluator: T_EXACT's floor as it stands)
    F, G, info = _run(f, X)
    assert info["rank1"] is True, info
    for b in (0, 1, 2):
        Fe, ge = E.fidelity_and_gradient(f, X[b])
        print(f"rank1_vs_exact_{b}: |dF| {abs(F[b] - Fe):.2e}")
        assert abs(F[b] - Fe) <= T1
        _within(f"rank1_vs_exact_{b}", G[b][:nt], ge[:nt], T_EXACT)


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


def test_weighted_projector_stays_rank_one():
    """Weights other than 1 only scale m: still one weighted level per sector."""
    nt = 96
    f = P.full9_problem(nt).replace(projector=W_WEIGHTED)
    X = _batch(nt, 300, 7300)
    F, G, info = _run(f, X)
    assert info["rank1"] is True, info
    _against_oracle("rank1_weighted", f, X, F, G, (0, 1))


def test_second_weighted_level_keeps_the_matrix_walk():
    """|rr> weighted beside |11>: the 3-level sector's M block has two non-zero rows, so the plan must
    keep the matrix walk -- and match the oracle as it does today (guards the eligibility rule)."""
    nt = 96
    f = P.full9_problem(nt).replace(projector=W_TWO_LEVELS)
    X = _batch(nt, 300, 8300)
    F, G, info = _run(f, X)
    assert info["rank1"] is False, info
    _against_oracle("rank1_ineligible", f, X, F, G, (0, 1))


def test_non_twin_class_takes_per_sector_vector_pairs():
    """GRAPE_OPT_NO_TWIN: class B's two sectors each carry their own (psi, phi) over their own propagator.
    Against the per-class matrix walks (GRAPE_OPT_NO_MERGE) within M1; F to T1 (the chain is
    associated differently there)."""
    from robustgrape_amd.operators import OPT_NO_MERGE, OPT_NO_TWIN
    nt = 70
    f = P.full9_problem(nt)
    X = _batch(nt, 300, 9300)
    F1, G1, i1 = _run(f, X, OPT_NO_TWIN)
    F0, G0, i0 = _run(f, X, OPT_NO_TWIN | OPT_NO_MERGE)
    assert i1["rank1"] is True and not any(i1["twin"]), i1
    assert i0["rank1"] is False, i0
    assert float(np.max(np.abs(F1 - F0))) <= T1
    _within("rank1_non_twin_vs_per_class", G1, G0, M1)
