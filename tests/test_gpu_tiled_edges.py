"""The tiled engine (64 < d <= 128) where tests/test_gpu_tiled.py's one input family never goes:
slab seams (s0 > 0 in both slab loops of launch_pipeline and in launch_expm_raw), projectors whose weights are
not their pattern and reach the remainder tile and the last level, every served term kind with np = 3 / 1 and
na = 2, steps of mixed Taylor degree and squaring count inside one gradient, a plan called twice, and
grape_expm_batch on matrices that are not skew-Hermitian.

Tiers and the three assertions of a fidelity case are tests/test_gpu_tiled.py's (_assert_fid, imported unchanged):
device vs exact, device vs oracle, and the oracle alone within half the device-vs-exact tier.  That last one is a
condition on the INPUT: a live case is kept only if its oracle - exact distance, measured on a CPU when the case
was chosen, is at most 0.75 of half the tier (another BLAS may move it); the measured ratio stands beside each
case.  Cases above 81 levels or with more than about ten steps come from tests/golden/tiled_edges.npz
(tests/golden/make_golden_tiled_edges.py).  No test here feeds the engine a non-finite value: that rule of
make_ctl is checked on the host alone (tests/test_tiled_ctl_cpu.py).
"""
import functools
import math
import os

import numpy as np
import pytest

from tests import problems as Pm
from tests.test_gpu_tiled import _assert_fid

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D = 65
SLOT = {3: 0, 5: 1, 7: 2, 9: 3, 13: 4}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@functools.lru_cache(maxsize=1)
def _golden():
    return dict(np.load(os.path.join(GOLDEN, "tiled_edges.npz"), allow_pickle=False))


def _live(name, fp, x, nparam):
    """One live case: device against the CPU oracle and the exact forward difference."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd import calculate_fidelity_and_derivatives
    F0, g0, _, _ = O.calculate_fidelity_and_derivatives(fp, x)
    Fe, ge = E.fidelity_and_gradient(fp, x, nparam=nparam)
    F, g, _, _ = calculate_fidelity_and_derivatives(fp, x)
    assert g.shape == x.shape
    _assert_fid(name, F, g, F0, g0, Fe, ge)


def _from_golden(name, F, Fdx):
    g = _golden()
    _assert_fid("tiled_edges_" + name, F, Fdx, float(g[f"F_{name}"]), g[f"F_dx_{name}"], float(g[f"F_exact_{name}"]),
                g[f"F_dx_exact_{name}"])


# --- 1. projectors -------------------------------------------------------------------------------------------
def _sixteen_negative():
    w = Pm.tiled_sixteen_weights(D)
    w[40] = -0.5
    return w


# name -> weights; oracle - exact as a fraction of half the tier, measured when the case was chosen
PROJECTORS = {
    "sixteen": lambda: Pm.tiled_sixteen_weights(D),     # 0.72: weights != pattern, rows of both tiles
    "negative": _sixteen_negative,                      # 0.68: a nonzero weight that is not positive
    "full": lambda: {i: 1.0 for i in range(D)},         # 0.51: all d rows with P = 80 != d
    "last": lambda: {D - 1: 1.0},                       # 0.09: rank one on the last level (remainder tile only)
}


@pytest.mark.parametrize("name", list(PROJECTORS))
def test_projector_weights_patterns_and_the_remainder_tile(name):
    """k_thead1 takes W as a weight on rows and as a pattern on columns, k_thead2 as a pattern on rows: with unequal
    (or negative) weights the two differ, and with weighted levels at and beyond row 64 the remainder tile's rows of
    W K, K^dag W K and M decide F and F_dx.  Five steps of every term kind, np = 3, na = 2."""
    fp, x = Pm.tiled_rich_problem(D, Pm.TILED_X0S, PROJECTORS[name](), 0.1)
    _live(f"tiled_edges_proj_{name}", fp, x, 3)


def test_sixteen_weights_at_113_levels_from_the_fixture():
    """P = 128 != d = 113: the remainder tile has 49 live rows and 15 of padding (oracle at 0.26 of half the tier)."""
    from robustgrape_amd import calculate_fidelity_and_derivatives
    fp, x, _ = Pm.tiled_edge_case("proj113")
    assert np.array_equal(x, _golden()["x_proj113"])
    F, Fdx, _, _ = calculate_fidelity_and_derivatives(fp, x)
    _from_golden("proj113", F, Fdx)


# --- 2. steps of mixed degree and squaring count ---------------------------------------------------------------
# |A_k|_1 = 0.600 1.300 0.200 3.550 0.054 0.900 0.300: Taylor 16, (s = 1, Taylor 16), 12, (s = 2, Taylor 20), 8,
# 20, 12 -- non-monotone, the smallest step directly after the s = 2 one
MIXED_X0S = (1.205, 2.599, 0.395, 7.098, 0.0, 1.783, 0.57)
SMALL_X0S = (0.2, -0.1, 0.3, 0.15, -0.25, 0.1, 0.2)     # every step at s = 0 (|A_k|_1 = 0.06 .. 0.16)


def _mixed():
    return Pm.tiled_rich_problem(D, MIXED_X0S, Pm.tiled_sixteen_weights(D), 0.05)


def test_mixed_degrees_and_squaring_counts_in_one_gradient():
    """Every Taylor band at s = 0, one step at s = 1 with a lower block count, one at s = 2, in one evaluation: an
    item writes B.E / B.Ev on its own last launch while the pass's smax is 2, and every eps-variant is scaled,
    expanded and squared by its nominal's ctl word.  The bands are asserted from the norms of this very input.
    Oracle at 0.25 of half the tier (it rises with the norm: 0.90 with steps up to 12.5, so s stops at 2 here)."""
    fp, x = _mixed()
    n = Pm.step_norms(fp, x, 3)
    print("step norms", n)
    bands = [(0.335, 0.826), (0.95, 1.65), (0.069, 0.335), (3.3, 3.8), (0.0, 0.069), (0.826, 0.95), (0.069, 0.335)]
    for nk, (lo, hi) in zip(n, bands):
        assert lo < nk <= hi, (n, bands)
    _live("tiled_edges_mixed", fp, x, 3)


# --- 3. np = 1 --------------------------------------------------------------------------------------------------
def test_one_control_per_step():
    """np = 1 (the terms on x[1], x[2] dropped; the step-index term stays): with the cases above (np = 3) and
    tests/test_gpu_tiled.py (np = 2) the three counts of the P.np loop.  Oracle at 0.24 of half the tier."""
    fp, x = Pm.tiled_rich_problem(D, Pm.TILED_X0S, Pm.tiled_sixteen_weights(D), 0.1, nparam=1)
    assert len(x) == 5 + 2
    _live("tiled_edges_np1", fp, x, 1)


# --- 4. batch with x_add ------------------------------------------------------------------------------------------
def _xadd_batch():
    rows = []
    for j, xa in enumerate(((0.3, -0.7), (-1.1, 0.4), (2.0, 1.3))):
        fp, x = Pm.tiled_rich_problem(D, Pm.TILED_X0S, Pm.tiled_sixteen_weights(D), 0.1, x_add=xa)
        x[:15] = np.random.default_rng(50 + j).uniform(-1.0, 1.0, 15) * np.tile([1.6, 1.0, 1.0], 5)
        rows.append(x)
    return fp, np.stack(rows)


def test_batch_with_two_additional_parameters_equals_single_calls():
    """Three evaluations with their own controls and x_add, na = 2: the (1 + na) strides of U0, K, ST_HEADK and
    ST_HEADT and Fdx[b nx + np N_t + q] at b > 0, item % N_t in k_tctl / k_tgen across a batch.  One pass of three and
    passes of 2 + 1 are bitwise three single calls; evaluation 2 against oracle and exact (oracle at 0.30)."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd.engine import GrapePlan
    fp, X = _xadd_batch()
    res = []
    for mb, chunks in ((3, [X]), (2, [X]), (1, [X[0:1], X[1:2], X[2:3]])):
        plan = GrapePlan(fp, nparam=3, max_batch=mb)
        try:
            out = [plan.fidelity_grad(c) for c in chunks]
        finally:
            plan.close()
        res.append((np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])))
    (F3, G3), (F2, G2), (F1, G1) = res
    assert np.all(np.isfinite(G1)) and G1.shape == X.shape
    assert np.array_equal(F3, F1) and np.array_equal(G3, G1)
    assert np.array_equal(F2, F1) and np.array_equal(G2, G1)
    assert len({float(f) for f in F1}) == 3
    F0, g0, _, _ = O.calculate_fidelity_and_derivatives(fp, X[2])
    Fe, ge = E.fidelity_and_gradient(fp, X[2], nparam=3)
    _assert_fid("tiled_edges_xadd_batch_eval2", float(F3[2]), G3[2], F0, g0, Fe, ge)


# --- 5. the slab seam -------------------------------------------------------------------------------------------
def test_the_slab_seam_inside_an_evaluation():
    """24 evaluations of 43 steps at d = 65 through a plan of max_batch = 24: one pass of 1 032 steps.  The slab is
    min(1 024, a quarter of the byte budget / (9 images of 2 80^2 doubles), max_batch N_t) = 1 024 items, so both slab
    loops of launch_pipeline run twice, 1 024 + 8, with s0 = 1 024 = 23 * 43 + 35: the seam falls inside evaluation
    23 at step k = 35, in the middle of chunk 5 (L_c = N_c = 7: chunks of 7 steps, the last one step long).  The test
    cannot observe the slab size; this arithmetic is what makes it a seam test.  A plan of max_batch = 1 has a slab of
    43 and no seam, and passes have identical arithmetic: all 24 results must be bitwise equal.
    Evaluation 23 also meets the tiers against oracle and exact from the fixture (oracle at 0.67 of half the tier).
    Workspace of the large plan: about 280 MB."""
    from robustgrape_amd.engine import GrapePlan
    assert Pm.SEAM_EVALS * Pm.SEAM_NT == 1032 and 1024 == 23 * Pm.SEAM_NT + 35 and math.ceil(math.sqrt(Pm.SEAM_NT)) == 7
    fp, X = Pm.seam_batch()
    assert np.array_equal(X[23], _golden()["x_seam23"])
    big = GrapePlan(fp, nparam=2, max_batch=Pm.SEAM_EVALS)
    try:
        F, G, _, _ = big.fidelity_grad(X)
    finally:
        big.close()
    one = GrapePlan(fp, nparam=2, max_batch=1)
    try:
        F1, G1, _, _ = one.fidelity_grad(X)
    finally:
        one.close()
    assert np.all(np.isfinite(G)) and G.shape == X.shape
    bad = [b for b in range(Pm.SEAM_EVALS) if F[b] != F1[b] or not np.array_equal(G[b], G1[b])]
    assert not bad, ("evaluations that differ from the seamless plan", bad)
    _from_golden("seam23", float(F[23]), G[23])


# --- 6. plan reuse ----------------------------------------------------------------------------------------------
def test_a_second_call_of_a_plan_equals_a_fresh_plan():
    """Items that return at once leave the ping-pong buffers, Q, Carry and M'_c of the previous call in place: after a
    call with squarings (smax = 2, every degree), a call whose steps all stop at s = 0 must not see them."""
    from robustgrape_amd.engine import GrapePlan
    fp, xa = _mixed()
    _, xb = Pm.tiled_rich_problem(D, SMALL_X0S, Pm.tiled_sixteen_weights(D), 0.05)
    assert Pm.step_norms(fp, xb, 3).max() <= 0.335 < 3.3 < Pm.step_norms(fp, xa, 3).max()
    plan = GrapePlan(fp, nparam=3, max_batch=1)
    try:
        Fa, Ga, _, _ = plan.fidelity_grad(xa[None, :])
        Fb, Gb, _, _ = plan.fidelity_grad(xb[None, :])
        Fa2, Ga2, _, _ = plan.fidelity_grad(xa[None, :])
    finally:
        plan.close()
    fresh = GrapePlan(fp, nparam=3, max_batch=1)
    try:
        Ff, Gf, _, _ = fresh.fidelity_grad(xb[None, :])
    finally:
        fresh.close()
    assert np.all(np.isfinite(Gb)) and Fa[0] != Fb[0]
    assert np.array_equal(Fb, Ff) and np.array_equal(Gb, Gf)
    assert np.array_equal(Fa2, Fa) and np.array_equal(Ga2, Ga)


# --- 7. grape_expm_batch ------------------------------------------------------------------------------------------
GINIBRE_NORMS = (0.06, 0.3, 0.8, 0.95, 1.9, 4.0, 12.0)


def _norm1(A):
    """|A|_1 in k_tctl's order: thread c adds hypot(re, im) down column c, row after row."""
    cs = np.zeros(A.shape[1])
    for row in A:
        cs = cs + np.hypot(row.real, row.imag)
    return float(cs.max())


def _on_threshold(d, rng, target):
    """A non-normal matrix whose entries are each real or imaginary (their moduli are exact on any hypot, so the
    device's column sums are the host's to the bit), rescaled until its computed 1-norm is `target` or a double
    beside it; the caller reads the norm back and takes the expected slot from the value obtained."""
    A = rng.normal(size=(d, d)) * np.where(rng.uniform(size=(d, d)) < 0.5, 1.0, 1j)
    for _ in range(8):
        n = _norm1(A)
        if n == target:
            break
        A = A * (target / n)
    return A


@functools.lru_cache(maxsize=2)
def _expm_items(d):
    """Eleven matrices (name, A) and their exponentials by oracle.grape_exact.exp_ld (longdouble Taylor 40), computed
    once per size: seven non-normal complex Ginibre matrices by 1-norm, the zero matrix, a skew-Hermitian matrix
    whose 1-norm is carried by the last column alone, and non-normal matrices rescaled onto 0.95 and 0.95 2."""
    from concurrent.futures import ThreadPoolExecutor

    from oracle import grape_exact as E
    rng = np.random.default_rng(2000 + d)
    gin = lambda: rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))  # noqa: E731
    items = []
    for nm in GINIBRE_NORMS:
        G = gin()
        G = G / _norm1(G) * nm
        items.append((f"ginibre{nm}", G))
    items.append(("zero", np.zeros((d, d), complex)))
    # last column (and, skew-Hermitian, last row) of moduli 3.55 / (d - 1); the rest a Hermitian Ginibre of norm 0.5
    H = gin()
    H = (H + H.conj().T) / 2
    H[:, d - 1] = H[d - 1, :] = 0.0
    H = H / _norm1(H) * 0.5
    v = np.exp(2j * np.pi * rng.uniform(size=d - 1)) * (3.55 / (d - 1))
    H[:d - 1, d - 1] = v
    H[d - 1, :d - 1] = v.conj()
    items.append(("lastcol", -1j * H))
    items.append(("on0.95", _on_threshold(d, rng, 0.95)))
    items.append(("on1.9", _on_threshold(d, rng, 0.95 * 2)))
    with ThreadPoolExecutor(4) as pool:
        refs = list(pool.map(lambda it: np.asarray(E.exp_ld(it[1].astype(np.clongdouble)), np.complex128), items))
    return items, refs


def _expm(d, mats):
    from robustgrape_amd import _capi
    Acm = np.ascontiguousarray(np.stack(mats).transpose(0, 2, 1))  # column-major per matrix
    Eo = np.full_like(Acm, np.nan)
    stats = (_capi.ctypes.c_int * 5)()
    _capi.check(_capi.lib().grape_expm_batch(0, d, len(mats), _capi.dptr(Acm), _capi.dptr(Eo), stats))
    return Eo.transpose(0, 2, 1), list(stats)


def _histogram(mats):
    from oracle import grape_oracle as O
    h = [0] * 5
    for A in mats:
        h[SLOT[O.pade_degree(_norm1(A))[0]]] += 1
    return h


def _check_expm_items(d, E, n):
    from tests.parity_log import record
    items, refs = _expm_items(d)
    for j in range(n):
        name, A = items[j]
        nm = _norm1(A)
        rel = float(np.max(np.abs(E[j] - refs[j])) / np.max(np.abs(refs[j])))
        tol = (1e-12 if nm > 2.1 else 1e-13) * max(1.0, nm)   # T0; 1e-12 where Julia takes Pade 13
        record(f"tiled_edges_expm_d{d}_{name}", "exp", rel, 1.0, tol)
        print(f"tiled expm d={d} {name} |A|_1={nm!r}: rel {rel:.2e} (tol {tol:.1e})")
        assert rel <= tol, (d, name, nm, rel)


@pytest.mark.parametrize("d", [65, 128])
def test_expm_of_matrices_that_are_not_skew_hermitian(d):
    """grape_expm_batch promises any A of moderate norm: non-normal complex Ginibre matrices in every Taylor band
    and at s = 1, 3, 4, norms exactly on 0.95 and 0.95 2 (or beside them: the slot follows the norm read back), the
    zero matrix (exactly I), and a 1-norm carried by column d - 1 alone, against the longdouble exponential at T0."""
    items, _ = _expm_items(d)
    mats = [A for _, A in items]
    names = [n for n, _ in items]
    n95, n19 = _norm1(mats[names.index("on0.95")]), _norm1(mats[names.index("on1.9")])
    print(f"norms on the thresholds: {n95!r} {n19!r}")
    assert abs(n95 - 0.95) <= 1e-15 and abs(n19 - 1.9) <= 2e-15
    last = mats[names.index("lastcol")]
    cols = np.abs(last).sum(axis=0)
    assert np.argmax(cols) == d - 1 and 3.3 < cols[d - 1] <= 3.8 and cols[d - 1] >= 4 * cols[:d - 1].max()
    assert np.array_equal(last, -last.conj().T)
    E, stats = _expm(d, mats)
    _check_expm_items(d, E, len(mats))
    z = E[names.index("zero")]
    assert np.array_equal(z.real, np.eye(d)) and not np.any(z.imag)
    El = E[names.index("lastcol")]
    assert np.max(np.abs(El.conj().T @ El - np.eye(d))) < 1e-12 * cols[d - 1]
    assert stats == _histogram(mats), (stats, [_norm1(A) for A in mats])


def test_expm_batch_beyond_one_slab():
    """1 750 items at d = 65 (P = 80): launch_expm_raw's slab is 2^30 B / (6 images of 2 80^2 doubles) = 1 747 items,
    so the second slab holds 3 (s0 = 1 747: ctl + s0, E + s0 img, k_tgen's raw[step]).  Ten matrices cycled: every
    item is bitwise its first occurrence, the first ten meet the reference, stats = 175 x the ten-item histogram."""
    d, n = 65, 1750
    assert (1 << 30) // (6 * 2 * 80 * 80 * 8) == 1747
    items, _ = _expm_items(d)
    mats = [A for _, A in items[:10]]
    E, stats = _expm(d, [mats[i % 10] for i in range(n)])
    _check_expm_items(d, E, 10)
    bad = [i for i in range(10, n) if not np.array_equal(E[i], E[i % 10])]
    assert not bad, bad[:10]
    assert stats == [175 * h for h in _histogram(mats)]
