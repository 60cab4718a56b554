"""The wide walks in the step frame (csrc/grape_walk_merged.hpp wide_step_grad_frame, wide_fwd_body).

With ladder charges both wide walks carry chi = D_k^dag psi (the gradient walk eta = D_k^dag phi too) and never
form E_k: a step re-frames its vectors by dl = e^{i a (x_prev - x_k)}, the phase of the controls' difference, with
x_prev the control of the step walked before (0 before the first one), held in a register across the tile seams.

Every plan is created as test_gpu_wide_tiles' (GRAPE_GAUGE_NCHUNKS=4, OPT_NO_EVAL1, scan_waves = 1), so that
W = max_batch x min(4, N_t):

  max_batch 32, 33    W = 128, 132 from N_t = 16 on: a full workgroup; a full one and one of four rows
                      (N_t = 1, 2: W = 32, 33 and 64, 66 -- one partly filled workgroup)
  max_batch 128       N_t = 1, 2 only: the full workgroup at those N_t too (W = 128, 256)
  N_t 1, 2, 16, 17, 33   no neighbour, one neighbour, a seam-free tile, a seam, two seams and a ragged tile

Problems: full9 (twin class B, ladder), scaled (a = -2.5), stiff, unequal (not twin, ladder).

A call is W + 5 evaluations (a wide pass and a chunked remainder of five rows) into buffers with two guard rows:
  row 0, and every row not named here   small and 2 pi-scale controls in turn
  row 1       controls in +-40
  row 2       equal controls: every dl after the first is 1 exactly
  row 3       zeros
  row 4       +-4e4 / |a| in turn: every phase a x_k is inside the phase table's bound (5e4), every difference is
              above it, so dl takes the library branch that a x_k alone never takes
  row W - 3   row 2's controls, row W - 2 row 4's negated (in the workgroup of four rows at max_batch 33)
  row W - 1   row 0's controls

Tolerances (the project's own, test_gpu_wide_walk.py / test_gpu_gauge_family.py):
  T1      1e-12 on F
  M1      1e-11 max|F_dx| + 1e-13 per row, wide against the chunked passes
  T_EXACT 1e-9 max|F_dx| + 2e-11 2^squarings(max step norm) against the exact forward difference
          (oracle/grape_exact.py), as test_gpu_gauge_family.py takes it

Do the +-4e4 / |a| rows count against the exact difference?  The evaluator's two forms -- the operator basis
(coefficients in longdouble from the double controls) and the closure (the Hamiltonian in double) -- were compared
on the CPU for every problem and N_t here, rows 0, 1, 4 and W - 2, as max|dF_dx| over half of T_EXACT:
  full9    N_t 1, 2: 0.03 .. 0.6;  17, 33: 1.0 .. 1.8   (rows 0 and 1 of the same plans: 0.1 .. 5.2)
  unequal  0.1 .. 2.5                                     (rows 0 and 1: 0.04 .. 4.1)
  stiff    0.00 .. 0.09                                   (rows 0 and 1: 0.02 .. 0.15)
  scaled   N_t 1: 0.1 .. 0.2;  N_t 2, 17, 33: 35 000 .. 57 000   (rows 0 and 1: 0.3 .. 234)
F agrees to 9e-16 everywhere.  Where a = 1 and b = 0 the large rows lie no further apart than the ordinary ones:
the distance there is the closure form's own noise (two double Hamiltonians differenced over eps), which the
operator-basis form exists to remove, and its arguments a x are exact.  Those rows count, at T_EXACT as it stands.
With scaled's b = 0.7 the argument a x + b itself is rounded at 4e4, in longdouble too: one ulp there, 2^-63 x 2^15
= 3.6e-15, against the phase difference |a| eps = 2.5e-8 of the forward difference is 1.4e-7 of the step's
F_dx in the evaluator itself (the device adds nothing at x: b lives in E~ and a x is exact).  So scaled's +-4e4
rows at N_t >= 2 are held to T_EXACT plus that 1.4e-7 of max|F_dx|, said in the test's output, and to M1 against
the chunked passes like every row; at N_t = 1 F_dx is below 1e-11 and the tier's absolute part decides.
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
CASES = ("full9", "scaled", "stiff", "unequal")
NTS = (1, 2, 16, 17, 33)
SHAPES = [(nt, mb) for nt in NTS for mb in (32, 33)] + [(1, 128), (2, 128)]
EXACT_NTS = (1, 2, 17, 33)
CIS_TAB_FAST = 5.0e4  # grape_cis.hpp kCisTabFast


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


def _gauge_a(case):
    return 1.0 if case == "full9" else float(P.GAUGE_FAMILY[case][0].get("a", 1.0))


@functools.lru_cache(maxsize=None)
def _batch(case, nt, max_batch):
    W = _wide(nt, max_batch)
    assert W >= 32
    seed = 9100 + 10 * nt + max_batch
    X = np.stack([P.random_x(nt, seed + s, small=(s % 2 == 0)) for s in range(W + 5)])
    X[1, :nt] = np.random.default_rng(seed).uniform(-40.0, 40.0, size=nt)
    X[2, :nt] = 1.2345678
    X[3, :nt] = 0.0
    big = 4e4 / abs(_gauge_a(case))
    X[4, :nt] = big * (1.0 - 2.0 * (np.arange(nt) % 2))
    a = _gauge_a(case)
    assert np.all(np.abs(a * X[4, :nt]) <= CIS_TAB_FAST)
    assert nt == 1 or np.all(np.abs(a * np.diff(X[4, :nt])) > CIS_TAB_FAST)
    X[W - 3] = X[2]
    X[W - 2] = X[4]
    X[W - 2, :nt] = -X[4, :nt]
    X[W - 1] = X[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _call(case, nt, max_batch, wide):
    """(F, F_dx, sector_info, F and F_dx of a second call into fresh buffers) of one device-resident call over
    _batch, after the guard: the two rows past the call's keep their sentinel, no row of the call its NaN."""
    import os
    import torch
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1, OPT_NO_WIDE
    X = _batch(case, nt, max_batch)
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
    out = []
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        Xd = torch.as_tensor(np.array(X), device="cuda:0")  # (a writable copy)
        for _ in range(2 if wide else 1):
            F = torch.full((n + 2,), float("nan"), dtype=torch.float64, device="cuda:0")
            G = torch.full((n + 2, X.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
            F[n:] = SENTINEL
            G[n:] = SENTINEL
            torch.cuda.synchronize()
            pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), n)
            pl.synchronize()
            out.append((F.cpu().numpy(), G.cpu().numpy()))
        assert np.array_equal(Xd.cpu().numpy(), X)  # the controls are read only
    finally:
        pl.close()
    res = []
    for F, G in out:
        assert np.all(F[n:] == SENTINEL) and np.all(G[n:] == SENTINEL), (case, nt, max_batch, wide)
        assert not np.any(np.isnan(F[:n])) and not np.any(np.isnan(G[:n])), (case, nt, max_batch, wide)
        F, G = F[:n], G[:n]
        F.setflags(write=False)
        G.setflags(write=False)
        res += [F, G]
    return res[0], res[1], info, (res[2], res[3]) if wide else None


def _within(test, G, G0, tier):
    """every row of G within tier of G0, relative to the row's max|G0|"""
    err = np.atleast_1d(np.max(np.abs(G - G0), axis=-1))
    scale = np.atleast_1d(np.max(np.abs(G0), axis=-1))
    bound = tier[0] * scale + tier[1]
    worst = int(np.argmax(err / bound))
    print(f"{test}: max|dF_dx| {float(np.max(err)):.3e} (worst row {worst}: {float(err[worst]):.3e} of bound "
          f"{float(bound[worst]):.3e}, scale {float(scale[worst]):.3e})")
    assert np.all(err <= bound), (test, float(np.max(err / bound)), worst)


@pytest.mark.parametrize("nt,max_batch", SHAPES)
@pytest.mark.parametrize("case", CASES)
def test_step_frame_walks_match_the_chunked_passes(case, nt, max_batch):
    """One wide pass and a chunked remainder of five rows against the same plan with GRAPE_OPT_NO_WIDE: F within
    T1, every F_dx row within M1, the five remainder rows bit for bit, rows 0 and W - 1 bit for bit, a second call
    bit for bit; the plan reports rank1, wide = W and the case's kernel variant; the guard rows intact (_call)."""
    W = _wide(nt, max_batch)
    t = f"frame_{case}_nt{nt}_mb{max_batch}"
    F1, G1, i1, again = _call(case, nt, max_batch, True)
    F0, G0, i0, _ = _call(case, nt, max_batch, False)
    assert i1["rank1"] is True and i0["rank1"] is True, (i1, i0)
    assert i1["wide"] == W and i0["wide"] == 0, (i1, i0, W)
    assert all(i1["ladder"]) and i1["twin"][1] == (case != "unequal"), i1
    dF = np.abs(F1 - F0)
    print(f"{t}: max|dF| {float(np.max(dF)):.2e} (row {int(np.argmax(dF))})")
    assert float(np.max(dF)) <= T1
    _within(t, G1, G0, M1)
    assert np.array_equal(F1[W:], F0[W:]) and np.array_equal(G1[W:], G0[W:])
    X = _batch(case, nt, max_batch)
    assert np.array_equal(X[0], X[W - 1])
    assert F1[0] == F1[W - 1] and np.array_equal(G1[0], G1[W - 1]), (F1[0], F1[W - 1])
    assert F1[2] == F1[W - 3] and np.array_equal(G1[2], G1[W - 3]), (F1[2], F1[W - 3])
    assert np.array_equal(F1, again[0]) and np.array_equal(G1, again[1])


@functools.lru_cache(maxsize=None)
def _exact(case, nt, row):
    from oracle import grape_exact as E
    fp = _problem(case, nt)
    x = _batch(case, nt, 33)[row]
    Fe, ge = E.fidelity_and_gradient(fp, x)
    s = E.squarings(P.max_step_norm(fp, x))
    return Fe, np.asarray(ge), s


@pytest.mark.parametrize("nt", EXACT_NTS)
@pytest.mark.parametrize("case", CASES)
def test_step_frame_walks_against_the_exact_forward_difference(case, nt):
    """max_batch = 33: rows 0 .. 4 and W - 2 (small, +-40, equal, zero and both +-4e4 / |a| rows; W - 2 in the
    ragged workgroup) against the reference's forward difference evaluated in longdouble: F within T1, the
    controls' F_dx within T_EXACT."""
    mb = 33
    W = _wide(nt, mb)
    F, G, info, _ = _call(case, nt, mb, True)
    assert info["wide"] == W, info
    up = _problem(case, nt).unitary_problem
    terms = [t for t in up.H0.terms if t.var == 1]
    for b in (0, 1, 2, 3, 4, W - 2):
        Fe, ge, s = _exact(case, nt, b)
        rel = T_EXACT[0]
        if b in (4, W - 2) and any(t.b != 0.0 for t in terms):  # (the evaluator's own argument rounding: see above)
            arg = max(abs(t.a) * 4e4 / abs(_gauge_a(case)) + abs(t.b) for t in terms)
            own = float(np.spacing(np.longdouble(arg))) / (abs(_gauge_a(case)) * up.eps)
            print(f"frame_vs_exact_{case}_nt{nt}_{b}: a x + b rounds in the evaluator: tier {rel:.1e} + {own:.2e}")
            rel += own
        print(f"frame_vs_exact_{case}_nt{nt}_{b}: |dF| {abs(F[b] - Fe):.2e} squarings {s}")
        assert abs(F[b] - Fe) <= T1, (case, nt, b, abs(F[b] - Fe))
        _within(f"frame_vs_exact_{case}_nt{nt}_{b}", G[b][:nt], ge[:nt], (rel, T_EXACT[1] * 2.0 ** s))
