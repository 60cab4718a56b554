"""The wide walks' tile traffic at the seams of its fast path (csrc/grape_walk_merged.hpp wide_load_x_full,
wide_flush_full).

A workgroup of the wide pass whose 128 rows are all evaluations moves a tile of 16 steps that lies wholly inside
N_t by a uniform stride, with no clamp and no predicate; every other workgroup and tile keeps the clamped load
and the predicated flush.  The shapes here sit on both seams of that branch:

  max_batch 32   W = 128: one full workgroup, the fast path alone
  max_batch 33   W = 132: a full workgroup and one of four rows
  N_t 15, 16, 17, 32, 33   a ragged tile alone, one full, full + one step, two full, two full + one

Every plan is created as test_gpu_wide_walk's (GRAPE_GAUGE_NCHUNKS=4, OPT_NO_EVAL1, scan_waves = 1), so that
W = 4 max_batch at each of these N_t.  A call is W + 5 evaluations, row W - 1 a copy of row 0, into F and F_dx
buffers with two more rows than the call: the rows of the call start as NaN, the two beyond as a sentinel.

Tolerances (the project's own, test_gpu_wide_walk.py):
  T1      1e-12 on F
  M1      1e-11 max|F_dx| + 1e-13 per row
  T_EXACT 1e-9 max|F_dx| + 2e-11
"""
import functools

import numpy as np
import pytest

from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
M1 = (1e-11, 1e-13)
T_EXACT = (1e-9, 2e-11)
NCHUNKS = 4
SENTINEL = -7.25e300
NTS = (15, 16, 17, 32, 33)
MAX_BATCHES = (32, 33)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _wide(nt, max_batch):
    """W of a plan whose chunk count was forced to NCHUNKS (the engine's L and chunk count)."""
    L = -(-nt // min(NCHUNKS, nt))
    return max_batch * -(-nt // L)


def _problem(case, nt):
    return P.full9_problem(nt) if case == "full9" else P.gauge_family_problem(case, nt)[0]


@functools.lru_cache(maxsize=None)
def _batch(nt, max_batch):
    """W + 5 rows alternating small and 2 pi-scale controls, row 1 with phases in +-40, row W - 1 = row 0"""
    W = _wide(nt, max_batch)
    seed = 7700 + 10 * nt + max_batch
    X = np.stack([P.random_x(nt, seed + s, small=(s % 2 == 0)) for s in range(W + 5)])
    X[1, :nt] = np.random.default_rng(seed).uniform(-40.0, 40.0, size=nt)
    X[W - 1] = X[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _call(case, nt, max_batch, wide):
    """(F, F_dx, sector_info) of one device-resident call over _batch(nt, max_batch), after the guard: the two
    rows past the call's keep their sentinel, and no row of the call keeps its NaN."""
    import os
    import torch
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1, OPT_NO_WIDE
    X = _batch(nt, max_batch)
    n = len(X)
    old = os.environ.get("GRAPE_GAUGE_NCHUNKS")
    os.environ["GRAPE_GAUGE_NCHUNKS"] = str(NCHUNKS)  # (read at plan creation)
    try:
        pl = GrapePlan(_problem(case, nt), nparam=1, device=0, max_batch=max_batch,
                       options=OPT_NO_EVAL1 | (0 if wide else OPT_NO_WIDE), scan_waves=1)
    finally:
        if old is None:
            del os.environ["GRAPE_GAUGE_NCHUNKS"]
        else:
            os.environ["GRAPE_GAUGE_NCHUNKS"] = old
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        Xd = torch.as_tensor(np.array(X), device="cuda:0")  # (a writable copy)
        F = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
        G = torch.full((n + 2, X.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
        F[n:] = SENTINEL
        G[n:] = SENTINEL
        torch.cuda.synchronize()
        pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), n)
        pl.synchronize()
        F, G = F.cpu().numpy(), G.cpu().numpy()
    finally:
        pl.close()
    assert np.all(F[n:] == SENTINEL) and np.all(G[n:] == SENTINEL), (case, nt, max_batch, wide)
    assert not np.any(np.isnan(F[:n])) and not np.any(np.isnan(G[:n])), (case, nt, max_batch, wide)
    F, G = F[:n], G[:n]
    F.setflags(write=False)
    G.setflags(write=False)
    return F, G, info


def _within(test, G, G0, tier):
    """every row of G within tier of G0, relative to the row's max|G0|"""
    err = np.atleast_1d(np.max(np.abs(G - G0), axis=-1))
    scale = np.atleast_1d(np.max(np.abs(G0), axis=-1))
    bound = tier[0] * scale + tier[1]
    worst = int(np.argmax(err / bound))
    print(f"{test}: max|dF_dx| {float(np.max(err)):.3e} (worst row {worst}: {float(err[worst]):.3e} of bound "
          f"{float(bound[worst]):.3e}, scale {float(scale[worst]):.3e})")
    assert np.all(err <= bound), (test, float(np.max(err / bound)))


def _wide_against_chunked(case, nt, max_batch):
    W = _wide(nt, max_batch)
    F1, G1, i1 = _call(case, nt, max_batch, True)
    F0, G0, i0 = _call(case, nt, max_batch, False)
    assert i1["rank1"] is True and i0["rank1"] is True, (i1, i0)
    assert i1["wide"] == W and i0["wide"] == 0, (i1, i0, W)
    print(f"tiles_{case}_nt{nt}_mb{max_batch}: max|dF| {float(np.max(np.abs(F1 - F0))):.2e}")
    assert float(np.max(np.abs(F1 - F0))) <= T1
    _within(f"tiles_{case}_nt{nt}_mb{max_batch}", G1, G0, M1)
    assert np.array_equal(F1[W:], F0[W:]) and np.array_equal(G1[W:], G0[W:])
    return i1


@pytest.mark.parametrize("max_batch", MAX_BATCHES)
@pytest.mark.parametrize("nt", NTS)
def test_tile_seams_match_chunked_passes(nt, max_batch):
    """One wide pass and a chunked remainder of five rows against the same plan with GRAPE_OPT_NO_WIDE: F within
    T1, every F_dx row within M1, the five remainder rows bit for bit; the guard rows intact (_call)."""
    info = _wide_against_chunked("full9", nt, max_batch)
    assert all(info["ladder"]), info


@pytest.mark.parametrize("nt", NTS)
def test_full_workgroup_rows_equal_ragged_workgroup_rows(nt):
    """The same controls in row 0 (the full workgroup: the fast path on every full tile) and in row W - 1 (the
    workgroup of four rows: the clamped load, the predicated flush): F and the F_dx row bit for bit."""
    W = _wide(nt, 33)
    F, G, info = _call("full9", nt, 33, True)
    assert info["wide"] == W and W - 1 >= 128, (info, W)
    assert np.array_equal(_batch(nt, 33)[0], _batch(nt, 33)[W - 1])
    assert F[0] == F[W - 1] and np.array_equal(G[0], G[W - 1]), (F[0], F[W - 1])


def test_seam_shape_against_the_exact_forward_difference():
    """N_t = 33, max_batch = 33: row 1 (the full workgroup, phases in +-40) and row W - 2 (the ragged one) against
    the reference's forward difference evaluated in longdouble (oracle/grape_exact.py), within T_EXACT as it stands (the steps are long at this N_t, |dt H| about 2.5: the
    evaluator squares, and the tier takes no factor for that)."""
    from oracle import grape_exact as E
    nt, mb = 33, 33
    W = _wide(nt, mb)
    f = P.full9_problem(nt)
    X = _batch(nt, mb)
    rows = (1, W - 2)
    F, G, info = _call("full9", nt, mb, True)
    assert info["wide"] == W, info
    for b in rows:
        Fe, ge = E.fidelity_and_gradient(f, X[b])
        print(f"tiles_vs_exact_{b}: |dF| {abs(F[b] - Fe):.2e}")
        assert abs(F[b] - Fe) <= T1
        _within(f"tiles_vs_exact_{b}", G[b][:nt], ge[:nt], T_EXACT)


def test_general_charge_plan_takes_the_tile_fast_path():
    """swap-B1 of the gauge family (tests/problems.py: two different 2-level sectors, general charges) takes a
    wide pass through the kernels without ladder charges: the tile paths there, against GRAPE_OPT_NO_WIDE."""
    info = _wide_against_chunked("swap-B1", 33, 33)
    assert not all(info["ladder"]) and not info["twin"][1], info
