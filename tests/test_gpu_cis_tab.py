"""The merged walks' table-driven step phase (csrc/grape_cis.hpp cis_tab, grape_walk_gauge.hpp gauge_cis_tab) and the
fused products of the phase helpers, on the GPU.

Every form of k_walk_fwd_m / k_walk_grad_m -- the wide pass, the chunked rank-one walk, the chunked matrix walk --
takes e^{i a x_k} from a 128-entry table staged in LDS.  Here one batch whose phases a x_k are uniform over
[-4 pi, 4 pi] (a row has 33 steps, so the batch as a whole is checked to meet every table index with both signs of
the argument), with one step just above the fast-path bound (the library sincos in the divergent branch) and one
row of zeros, goes through the three forms: against each other, against the exact forward difference
(oracle/grape_exact.py), and twice for the same bits.  N_t = 33 with max_batch 40 and GRAPE_GAUGE_NCHUNKS=4
(test_gpu_wide_walk.py's set-up): W = 160, x tiles of 16 + 16 + 1 steps, a partly filled second workgroup.  The
same for "swap-B1" of tests/problems.py GAUGE_FAMILY: general charges and two unequal 2-level sectors, so the
runtime loops of gauge_pow and gauge_fd_weights_dn run at a charge difference of 2 in class A.

Tolerances (the project's own, test_gpu_wide_walk.py / test_gpu_gauge_family.py):
  T1      1e-12 on F
  M1      1e-11 max|F_dx| + 1e-13 between walks of the same per-step arithmetic
  T_EXACT 1e-9 max|F_dx| + 2e-11 2^squarings(max step norm), the controls' F_dx against the exact difference
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
NT = 33
MAX_BATCH = 40
W = 160               # MAX_BATCH x 4 chunks of 9 steps
TAB_FAST = 5.0e4      # grape_cis::kCisTabFast
ROWS = (0, 1, 2)      # uniform phases, the step above the bound, zeros
CASES = ("full9", "swap-B1")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("GRAPE_GAUGE_NCHUNKS", str(NCHUNKS))  # (read at plan creation)


@functools.lru_cache(maxsize=None)
def _case(case):
    """(problem, X, {row: (F exact, F_dx exact)}): W rows, the references of ROWS evaluated once."""
    from oracle import grape_exact as E
    if case == "full9":
        fp, a = P.full9_problem(NT), 1.0
    else:
        fp, a = P.gauge_family_problem(case, NT)[0], P.GAUGE_FAMILY[case][0].get("a", 1.0)
    rng = np.random.default_rng(1100 + CASES.index(case))
    X = np.empty((W, NT + 1))
    X[:, :NT] = rng.uniform(-4 * np.pi, 4 * np.pi, size=(W, NT)) / a
    X[:, NT] = 2 * np.pi * rng.uniform(size=W)
    X[1, 7] = (TAB_FAST + 3.0) / a
    X[2] = 0.0
    idx = np.rint(a * X[:, :NT] * (64 / np.pi)).astype(np.int64)
    assert set((idx[idx >= 0] & 127).tolist()) == set(range(128)) and set((idx[idx < 0] & 127).tolist()) == set(range(128))
    assert abs(a * X[1, 7]) > TAB_FAST and np.max(np.abs(a * np.delete(X[:, :NT].ravel(), NT + 7))) < TAB_FAST
    refs = {b: E.fidelity_and_gradient(fp, X[b]) for b in ROWS}
    X.setflags(write=False)
    return fp, X, refs


def _device_call(fp, X, options, repeat=1):
    """[(F, F_dx)] of `repeat` device-resident calls over X on one plan, and its sector_info."""
    import torch
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1
    pl = GrapePlan(fp, nparam=1, device=0, max_batch=MAX_BATCH, options=options | OPT_NO_EVAL1, scan_waves=1)
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        Xd = torch.as_tensor(np.array(X), device="cuda:0")  # (a writable copy: the cached batch is read-only)
        outs = []
        for _ in range(repeat):
            F = torch.full((len(X),), float("nan"), dtype=torch.float64, device="cuda:0")
            G = torch.full(X.shape, float("nan"), dtype=torch.float64, device="cuda:0")
            torch.cuda.synchronize()
            pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), len(X))
            pl.synchronize()
            outs.append((F.cpu().numpy(), G.cpu().numpy()))
    finally:
        pl.close()
    return outs, info


def _within(test, G, G0, tier):
    """every row of G within tier of G0, relative to the row's max|G0|"""
    err = np.max(np.abs(G - G0), axis=-1)
    scale = np.max(np.abs(G0), axis=-1)
    bound = tier[0] * scale + tier[1]
    worst = int(np.argmax(np.atleast_1d(err / bound)))
    print(f"{test}: max err {float(np.max(err)):.3e} (worst row {worst}: {float(np.atleast_1d(err)[worst]):.3e} of bound "
          f"{float(np.atleast_1d(bound)[worst]):.3e})")
    assert np.all(err <= bound), (test, float(np.max(err / bound)))


@pytest.mark.parametrize("case", CASES)
def test_three_forms_agree_and_match_the_exact_difference(case):
    """Wide pass, chunked rank-one walk, chunked matrix walk: F at T1 and F_dx at M1 between them, the rank-one
    and the matrix walk's F bit for bit (one forward walk), F at T1 and the controls' F_dx at T_EXACT against the
    exact forward difference for the three special rows -- through all three forms."""
    from oracle import grape_exact as E
    from robustgrape_amd.operators import OPT_NO_RANK1, OPT_NO_WIDE
    fp, X, refs = _case(case)
    (wide,), iw = _device_call(fp, X, 0)
    (r1,), ir = _device_call(fp, X, OPT_NO_WIDE)
    (mat,), im = _device_call(fp, X, OPT_NO_WIDE | OPT_NO_RANK1)
    assert iw["wide"] == W and iw["rank1"] is True, iw
    assert ir["wide"] == 0 and ir["rank1"] is True, ir
    assert im["wide"] == 0 and im["rank1"] is False, im
    if case != "full9":
        assert (iw["twin"][1], all(iw["ladder"])) == P.GAUGE_FAMILY[case][2] == (False, False), iw
    for name, (F, G) in (("wide", wide), ("rank1", r1), ("matrix", mat)):
        assert not np.any(np.isnan(F)) and not np.any(np.isnan(G)), name
    for name, (F, G) in (("wide", wide), ("rank1", r1)):
        print(f"cis_tab_{case}_{name}_vs_matrix: max|dF| {float(np.max(np.abs(F - mat[0]))):.2e}")
        assert float(np.max(np.abs(F - mat[0]))) <= T1
        _within(f"cis_tab_{case}_{name}_vs_matrix", G, mat[1], M1)
    print(f"cis_tab_{case}_wide_vs_rank1: max|dF| {float(np.max(np.abs(wide[0] - r1[0]))):.2e}")
    assert float(np.max(np.abs(wide[0] - r1[0]))) <= T1
    _within(f"cis_tab_{case}_wide_vs_rank1", wide[1], r1[1], M1)
    assert np.array_equal(r1[0], mat[0])
    for b in ROWS:
        Fe, ge = refs[b]
        tier = (T_EXACT[0], T_EXACT[1] * 2.0 ** E.squarings(P.max_step_norm(fp, X[b])))
        for name, (F, G) in (("wide", wide), ("rank1", r1), ("matrix", mat)):
            print(f"cis_tab_{case}_{name}_vs_exact_{b}: |dF| {abs(F[b] - Fe):.2e}")
            assert abs(F[b] - Fe) <= T1
            _within(f"cis_tab_{case}_{name}_vs_exact_{b}", G[b][:NT], np.asarray(ge)[:NT], tier)


def test_repeated_call_returns_the_same_bits():
    """W + 5 rows: one wide pass and a chunked remainder, called twice on one plan."""
    fp, X, _ = _case("full9")
    (a, b), info = _device_call(fp, np.concatenate([X, X[:5]]), 0, repeat=2)
    assert info["wide"] == W, info
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert not np.any(np.isnan(a[0])) and not np.any(np.isnan(a[1]))
