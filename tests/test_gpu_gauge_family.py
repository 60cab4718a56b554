"""The phase-covariant walks beyond the benchmark Hamiltonian (tests/problems.py GAUGE_FAMILY).

Every other GPU test of these kernels runs rydberg_full_operator_basis(1, 1, 0, 0, 10) at t0 = 7.613 in its
natural level order: ladder charges N_j = j, twin 2-level sectors (or GRAPE_OPT_NO_TWIN over identical data),
the weighted level first in its sector, cos / sin(x), no detuning.  The engine accepts far more (find_gauge:
any common factor a and offset b, any integer charges in any order, any x-independent diagonal), and
merged_variant compiles {twin class B or not} x {ladder charges or general} of every merged kernel.  The
family here reaches them with nine d = 9 problems:

  detuned, scaled, mixed, stiff   twin, ladder: detunings, cos / sin(a x + b), another Rabi frequency, B = 0
                                  and B = 500 (squarings in E~), another t0
  unequal                         two different 2-level sectors: not twin, ladder
  swap-A, swap-B2, swap-B1        relabellings: general charges in class A / both sectors of class B / one
                                  sector of class B, the weighted level last in its sector
  reversed                        every level renamed i -> 8 - i

each through every kernel family that can serve it (the wide pass, the chunked rank-one and matrix merged
walks, the per-class chunk walks, k_eval1, the pair kernels, the per-step exponentials), rows 0, 1, 2 against
the exact forward difference (oracle/grape_exact.py) and the oracle, and the paths against each other.

Tolerances (the project's own, as in test_gpu_gauge.py / test_gpu_wide_walk.py / test_gpu_eval1.py):
  T1      1e-12 on F
  T_EXACT 1e-9 max|F_dx| + 2e-11 2^squarings(max step norm), the controls' F_dx against the exact difference
  fd_tier tests/problems.py: the per-step exponentials' path, and the whole F_dx (the x_add entry is the
          target's forward difference formed in double) against the oracle, plus the oracle's own measured
          distance from the exact value
  M1      1e-11 max|F_dx| + 1e-13 between walks of the same per-step arithmetic
  T_PAIR  1e-13 on F, 1e-11 max|F_dx| + 1e-13 between k_eval1 and the pair kernels
"""
import functools

import numpy as np
import pytest

from tests import problems as P

pytestmark = pytest.mark.gpu
T1 = 1e-12
M1 = (1e-11, 1e-13)
T_EXACT = (1e-9, 2e-11)
T_PAIR = (1e-13, 1e-11, 1e-13)
NCHUNKS = 4
MAX_BATCH = 40          # W = 160 at N_t = 70
ROWS = (0, 1, 2)
CASES = list(P.GAUGE_FAMILY)
CASE_NT = [(c, 70) for c in CASES] + [(c, nt) for c in ("swap-B1", "scaled") for nt in (1, 3)]
WORST = {}              # path -> check -> worst err / bound seen (printed when the module is done)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield
    for path in sorted(WORST):
        print(f"\nworst err / bound [{path}]: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(WORST[path].items())))


@pytest.fixture(autouse=True)
def _chunks(monkeypatch):
    monkeypatch.setenv("GRAPE_GAUGE_NCHUNKS", str(NCHUNKS))  # (read at plan creation)


def _wide(nt):
    """W of a plan whose chunk count was forced to NCHUNKS (the engine's L and chunk count)."""
    L = -(-nt // min(NCHUNKS, nt))
    return MAX_BATCH * -(-nt // L)


@functools.lru_cache(maxsize=None)
def _case(case, nt):
    """(problem, X, {row: (F exact, F_dx exact, F oracle, F_dx oracle)}): W + 37 rows alternating small and
    2 pi-scale controls, row 1 with phases in +-40; the references of rows 0, 1, 2 evaluated once per module."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    fp, _ = P.gauge_family_problem(case, nt)
    seed = 5100 + 97 * CASES.index(case) + nt
    X = np.stack([P.random_x(nt, seed + s, small=(s % 2 == 0)) for s in range(_wide(nt) + 37)])
    X[1, :nt] = np.random.default_rng(seed).uniform(-40.0, 40.0, size=nt)
    refs = {}
    for b in ROWS:
        Fe, ge = E.fidelity_and_gradient(fp, X[b])
        F0, g0 = O.calculate_fidelity_and_derivatives(fp, X[b])[:2]
        refs[b] = (Fe, np.asarray(ge), float(F0), np.asarray(g0))
    X.setflags(write=False)
    return fp, X, refs


def _note(path, what, err, bound):
    w = WORST.setdefault(path, {})
    w[what] = max(w.get(what, 0.0), err / bound)


def _check(path, test, what, a, ref, tier):
    """max|a - ref| <= tier[0] max|ref| + tier[1], printed and recorded (tests/parity_log.py)."""
    from tests.parity_log import record
    err = float(np.max(np.abs(np.asarray(a) - np.asarray(ref))))
    scale = float(np.max(np.abs(ref)))
    bound = tier[0] * scale + tier[1]
    record(test, what, err, scale, bound)
    _note(path, what, err, bound)
    print(f"{test} {what}: err {err:.3e} bound {bound:.3e} (scale {scale:.3e}, ratio {err / bound:.3g})")
    assert err <= bound, (test, what, err, bound)


def _rows_within(path, test, what, G, G0, tier):
    """every row of G within tier of G0, relative to the row's max|G0|"""
    err = np.max(np.abs(G - G0), axis=-1)
    scale = np.max(np.abs(G0), axis=-1)
    bound = tier[0] * scale + tier[1]
    from tests.parity_log import record
    worst = int(np.argmax(err / bound))
    record(test, what, float(err[worst]), float(scale[worst]), float(bound[worst]))
    _note(path, what, float(err[worst]), float(bound[worst]))
    print(f"{test} {what}: worst row {worst}: err {float(err[worst]):.3e} bound {float(bound[worst]):.3e} "
          f"(scale {float(scale[worst]):.3e}, ratio {float(err[worst] / bound[worst]):.3g})")
    assert np.all(err <= bound), (test, what, float(np.max(err / bound)))


def _against_references(path, test, fp, X, refs, F, G, exact_tier=None):
    """Rows 0, 1, 2 of one path: F within T1 of the exact value and of the oracle; the controls' F_dx within
    T_EXACT of the exact forward difference (exact_tier "fd": the FD tier, for the per-step exponentials); the
    whole F_dx within the FD tier plus the oracle's own distance from the exact value, against the oracle."""
    from oracle import grape_exact as E
    nt = fp.unitary_problem.ntimes
    for b in ROWS:
        Fe, ge, F0, g0 = refs[b]
        _check(path, f"{test}_{b}", "F vs exact", F[b], Fe, (0.0, T1))
        _check(path, f"{test}_{b}", "F vs oracle", F[b], F0, (0.0, T1))
        if exact_tier == "fd":
            tier = P.fd_tier(fp, X[b])
        else:
            tier = (T_EXACT[0], T_EXACT[1] * 2.0 ** E.squarings(P.max_step_norm(fp, X[b])))
        _check(path, f"{test}_{b}", "F_dx vs exact", G[b][:nt], ge[:nt], tier)
        t2, t2a = P.fd_tier(fp, X[b])
        _check(path, f"{test}_{b}", "F_dx vs oracle", G[b], g0, (t2, t2a + float(np.max(np.abs(g0 - ge)))))


def _plan(fp, max_batch, options=0, throughput=False):
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_NO_EVAL1
    if throughput:  # test_gpu_rank1_walk's: the throughput chunking at a few hundred evaluations
        return GrapePlan(fp, nparam=1, device=0, max_batch=max_batch, options=options | OPT_NO_EVAL1, scan_waves=1)
    return GrapePlan(fp, nparam=1, device=0, max_batch=max_batch, options=options)


def _device_call(fp, X, options):
    """(F, F_dx, sector_info, kernel launches) of one device-resident call over X (profiled)."""
    import torch
    pl = _plan(fp, MAX_BATCH, options, throughput=True)
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        Xd = torch.as_tensor(np.ascontiguousarray(X), device="cuda:0")
        F = torch.full((len(X),), float("nan"), dtype=torch.float64, device="cuda:0")
        G = torch.full(X.shape, float("nan"), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        pl.set_profiling(True)
        pl.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), len(X))
        pl.synchronize()
        kt = pl.kernel_times()
    finally:
        pl.close()
    return F.cpu().numpy(), G.cpu().numpy(), info, kt


def _host_call(fp, X, max_batch, options, throughput):
    """(F, F_dx, sector_info, kernel launches) of fidelity_grad over X (profiled)."""
    pl = _plan(fp, max_batch, options, throughput)
    try:
        info = pl.sector_info()
        assert pl.sectors() == P.FULL9_SYM, pl.sectors()
        pl.set_profiling(True)
        pl.kernel_times(reset=True)
        F, G, _, _ = pl.fidelity_grad(np.ascontiguousarray(X))
        kt = pl.kernel_times(reset=True)
    finally:
        pl.close()
    return np.array(F), np.array(G), info, kt


def test_cases_reach_every_merged_variant():
    """The coverage condition: over the cases, each of the four (twin class B, ladder charges in both classes)
    variants of the merged kernels is reported by a plan that runs the rank-one walk and the wide pass; one such
    plan has the weighted level not first in class A's sector, one not first in a class B sector (c from the
    relabelled projector and the sector's levels in ascending order, tests/problems.py weighted_indices)."""
    seen, c_a, c_b = set(), set(), set()
    for case in CASES:
        fp, _ = P.gauge_family_problem(case, 70)
        pl = _plan(fp, MAX_BATCH, throughput=True)
        try:
            info, sectors = pl.sector_info(), pl.sectors()
        finally:
            pl.close()
        c = P.weighted_indices(fp)
        print(f"{case}: sectors {sectors} {info} c_A {c[3]} c_B {c[2]}")
        assert sectors == P.FULL9_SYM and info["symmetric"] and info["gauge"] == (True, True), (case, sectors, info)
        assert info["rank1"] is True and info["wide"] == _wide(70), (case, info)
        variant = (info["twin"][1], all(info["ladder"]))
        want = P.GAUGE_FAMILY[case][2]
        assert want is None or variant == want, (case, variant, want, info)
        seen.add(variant)
        c_a.add(c[3][0])
        c_b.update(c[2])
    assert seen == {(True, True), (True, False), (False, True), (False, False)}, seen
    assert c_a - {0, None} and c_b - {0, None}, (c_a, c_b)


@pytest.mark.parametrize("case,nt", CASE_NT)
def test_throughput_walks_of_the_family(case, nt):
    """The wide pass, the chunked rank-one walk, the chunked matrix walk (the merged kernels' variants) and the
    per-class chunk walks over W + 37 rows: each against the references, wide vs chunked (F at T1, F_dx at M1,
    the 37 remainder rows bit for bit), rank-one vs matrix (F bit for bit, F_dx at M1), merged vs per-class
    (T1, M1); the launches counted through the profiling events."""
    from robustgrape_amd.operators import OPT_NO_MERGE, OPT_NO_RANK1, OPT_NO_WIDE
    fp, X, refs = _case(case, nt)
    W, n = _wide(nt), len(X)
    passes = -(-n // MAX_BATCH)
    t = f"family_{case}_nt{nt}"
    Fw, Gw, iw, kw = _device_call(fp, X, 0)
    Fc, Gc, ic, kc = _device_call(fp, X, OPT_NO_WIDE)
    Fr, Gr, ir, kr = _host_call(fp, X, MAX_BATCH, OPT_NO_WIDE, True)
    Fm, Gm, im, km = _host_call(fp, X, MAX_BATCH, OPT_NO_WIDE | OPT_NO_RANK1, True)
    Fp, Gp, ip, kp = _host_call(fp, X, MAX_BATCH, OPT_NO_WIDE | OPT_NO_RANK1 | OPT_NO_MERGE, True)
    assert iw["rank1"] is True and iw["wide"] == W and all(iw["gauge"]), iw
    assert ic["rank1"] is True and ic["wide"] == 0, ic
    assert im["rank1"] is False and im["wide"] == 0 and ip["rank1"] is False, (im, ip)
    assert iw["twin"] == ic["twin"] == im["twin"] == ip["twin"] and iw["ladder"] == im["ladder"] == ip["ladder"]
    want = P.GAUGE_FAMILY[case][2]
    assert want is None or (iw["twin"][1], all(iw["ladder"])) == want, (case, iw)
    # one wide pass and one chunked remainder; chunked passes of MAX_BATCH; one merged gradient walk per pass,
    # one per class without the merge
    assert kw["k_walk_grad"][1] == 2 and kc["k_walk_grad"][1] == passes, (kw, kc)
    assert kr["k_walk_grad"][1] == passes and km["k_walk_grad"][1] == passes and kp["k_walk_grad"][1] == 2 * passes, \
        (kr, km, kp)
    for kt in (kw, kc, kr, km, kp):
        assert kt["k_eval1"][1] == 0, kt
    assert not np.any(np.isnan(Fw)) and not np.any(np.isnan(Gw)) and not np.any(np.isnan(Gc))
    _against_references("wide", f"{t}_wide", fp, X, refs, Fw, Gw)
    _against_references("rank1", f"{t}_rank1", fp, X, refs, Fc, Gc)
    _against_references("matrix", f"{t}_matrix", fp, X, refs, Fm, Gm)
    _against_references("per-class", f"{t}_per_class", fp, X, refs, Fp, Gp)
    _check("wide vs chunked", t, "F wide vs chunked", Fw, Fc, (0.0, T1))
    _rows_within("wide vs chunked", t, "F_dx wide vs chunked", Gw, Gc, M1)
    assert np.array_equal(Fw[W:], Fc[W:]) and np.array_equal(Gw[W:], Gc[W:])
    assert np.array_equal(Fr, Fm)
    _rows_within("rank1 vs matrix", t, "F_dx rank1 vs matrix", Gr, Gm, M1)
    _rows_within("rank1 vs matrix", t, "F_dx rank1 (device call) vs matrix", Gc, Gm, M1)
    _check("merged vs per-class", t, "F merged vs per-class", Fm, Fp, (0.0, T1))
    _rows_within("merged vs per-class", t, "F_dx merged vs per-class", Gm, Gp, M1)


@pytest.mark.parametrize("case,nt", CASE_NT)
def test_latency_kernels_of_the_family(case, nt):
    """Five evaluations through k_eval1, the pair kernels and the per-step exponentials (GRAPE_OPT_NO_GAUGE):
    each against the references (the per-step exponentials at the FD tier), k_eval1 vs the pair kernels at
    T_PAIR."""
    from robustgrape_amd.operators import OPT_NO_EVAL1, OPT_NO_GAUGE
    fp, X, refs = _case(case, nt)
    X5 = X[:5]
    t = f"family_{case}_nt{nt}"
    Fe, Ge, ie, ke = _host_call(fp, X5, 5, 0, False)
    Fq, Gq, iq, kq = _host_call(fp, X5, 5, OPT_NO_EVAL1, False)
    Fn, Gn, i_n, _ = _host_call(fp, X5, 5, OPT_NO_GAUGE, False)
    assert ie["eval1"] is True and all(ie["gauge"]), ie
    assert iq["eval1"] is False and all(iq["gauge"]), iq
    assert i_n["eval1"] is False and not any(i_n["gauge"]), i_n
    assert ke["k_eval1"][1] == 1 and sum(m for k, (_, m) in ke.items() if k != "k_eval1") == 0, ke
    assert kq["k_eval1"][1] == 0 and kq["k_walk_fwd"][1] == 1 and kq["k_walk_grad"][1] == 1, kq  # one pair launch per stage
    _against_references("eval1", f"{t}_eval1", fp, X5, refs, Fe, Ge)
    _against_references("pair", f"{t}_pair", fp, X5, refs, Fq, Gq)
    _against_references("per-step exp", f"{t}_no_gauge", fp, X5, refs, Fn, Gn, exact_tier="fd")
    _check("eval1 vs pair", t, "F eval1 vs pair", Fe, Fq, (0.0, T_PAIR[0]))
    _rows_within("eval1 vs pair", t, "F_dx eval1 vs pair", Ge, Gq, T_PAIR[1:])


@pytest.mark.parametrize("case", ["detuned", "reversed"])
def test_idle_dark_level_is_left_out_of_the_sectors(case):
    """With a detuning the dark state (|1r> - |r1>) / sqrt 2 has a diagonal entry: a level of its own that
    evolves by a phase.  Without projector weight that phase reaches neither F nor F_dx, and the sector layout
    leaves the level out (grape_plan_setup.hpp find_sectors, grape_descriptor.hip idle_levels) -- as a third, padded 2-level sector it
    kept the plan off the pair, merged and one-workgroup kernels.  Checked with the general head
    (GRAPE_OPT_GENERAL_HEAD assembles the whole U, zero on that level), and with weight on |1r> and |r1>: the
    level stays, a 1-level sector in the 2-level class, and the plan matches the oracle."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    from robustgrape_amd.operators import OPT_GENERAL_HEAD, OPT_NO_EVAL1
    nt = 70
    fp, X, refs = _case(case, nt)
    X5 = X[:5]
    F, G, info, _ = _host_call(fp, X5, 5, OPT_GENERAL_HEAD | OPT_NO_EVAL1, False)  # (_host_call: sectors 3 + 2 + 2)
    assert info["eval1"] is False and all(info["gauge"]), info
    _against_references("general head", f"family_{case}_nt{nt}_general_head", fp, X5, refs, F, G)
    perm = P.GAUGE_FAMILY[case][1] or list(range(9))
    W = np.array(fp.projector, np.float64)
    W[perm[6], perm[6]] = W[perm[7], perm[7]] = 0.5
    fw = fp.replace(projector=W)
    pl = _plan(fw, 5)
    try:
        assert pl.sectors() == ((3, 1), (2, 3)), pl.sectors()
        Fw, Gw, _, _ = pl.fidelity_grad(np.ascontiguousarray(X5))
    finally:
        pl.close()
    for b in (0, 1):
        F0, g0 = O.calculate_fidelity_and_derivatives(fw, X[b])[:2]
        Fe, ge = E.fidelity_and_gradient(fw, X[b])
        g0 = np.asarray(g0)
        t = f"family_{case}_nt{nt}_weighted_dark_{b}"
        _check("weighted dark level", t, "F vs oracle", Fw[b], float(F0), (0.0, T1))
        _check("weighted dark level", t, "F vs exact", Fw[b], Fe, (0.0, T1))
        t2, t2a = P.fd_tier(fw, X[b])
        _check("weighted dark level", t, "F_dx vs oracle", Gw[b], g0, (t2, t2a + float(np.max(np.abs(g0 - ge)))))
