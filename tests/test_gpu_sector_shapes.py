"""The sector path on block structures beyond the three Rydberg Hamiltonians (tests/sector_problems.py): two
components sharing a sector, four and six sectors in a class, sectors of 5 and 6 levels (no walk, the general
head), a walking class next to a non-walking one, several fixed levels, an all-diagonal H0, an error source that
merges H0's components, and symmetry-adapted sectors behind a complex basis V (hidden blocks: the rotated
projector is complex Hermitian and the rotated target dense).

Every case: the sector plan against the whole-matrix plan (GRAPE_OPT_NO_SECTORS) and the live oracle on the
closure form, with the layout of the table (sector_problems.CASES, pinned on the host by
tests/test_sector_shapes_cpu.py) asserted on the plan.  Tolerances are the project's: T1 on F, problems.fd_tier
on F_dx, T2 on F_d2err, T3 on F_d2err_dx (both times problems.fd_factor on long steps), the x_add rows of
F_d2err_dx through tests/xadd_pin.py."""
import numpy as np
import pytest

from tests import problems as P
from tests import sector_problems as SP
from tests.parity_log import record
from tests.xadd_pin import check_xadd, exact_rows

pytestmark = pytest.mark.gpu
T1 = 1e-12
T2, T2_ABS = 1e-6, 1e-7
T3, T3_ABS = 1e-5, 1e-7
NT, NT_HIDDEN, NB = 37, 13, 4   # 37 steps at scan_waves = 1: 21 / 16 / 32 / 12 / 10 chunks for S = 3 / 4 / 2 / 5 / 6
ORACLE_ROWS = (0, 3)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _run(fp, X, options=0, nparam=1, scan_waves=0, max_batch=None):
    """(sectors(), sector_info(), the four outputs) of a fresh plan."""
    from robustgrape_amd.engine import GrapePlan
    pl = GrapePlan(fp, nparam=nparam, device=0, max_batch=max_batch or len(X), options=options, scan_waves=scan_waves)
    try:
        return pl.sectors(), pl.sector_info(), pl.fidelity_grad(X)
    finally:
        pl.close()


def _compare(test, got, ref, fp, X, nparam, xadd_exact=None):
    """got / ref: (F, F_dx, F_d2err, F_d2err_dx) of one evaluation or of a batch."""
    up = fp.unitary_problem
    nmain = up.ntimes * nparam
    t2, t2a = P.fd_tier(fp, X, nparam)
    fac = P.fd_factor(fp, X, nparam)
    got, ref = [np.asarray(v) for v in got], [np.asarray(v) for v in ref]
    ef = float(np.max(np.abs(got[0] - ref[0])))
    record(test, "F", ef, 1.0, T1)
    assert ef <= T1, (test, "F", ef)
    err, sc = float(np.max(np.abs(got[1] - ref[1]))), float(np.max(np.abs(ref[1])))
    record(test, "F_dx", err, sc, t2 * sc + t2a)
    print(f"{test}: F {ef:.1e} F_dx {err:.2e} / {sc:.2e} (tier {t2 * sc + t2a:.2e})", end="")
    assert err <= t2 * sc + t2a, (test, "F_dx", err, sc)
    if len(up.error_sources) == 0:
        print()
        return
    e2, s2 = float(np.max(np.abs(got[2] - ref[2]))), float(np.max(np.abs(ref[2])))
    record(test, "F_d2err", e2, s2, fac * (T2 * s2 + T2_ABS))
    main = (Ellipsis, slice(0, nmain), slice(None))
    e3, s3 = float(np.max(np.abs(got[3][main] - ref[3][main]))), float(np.max(np.abs(ref[3][main])))
    record(test, "F_d2err_dx", e3, s3, fac * (T3 * s3 + T3_ABS))
    print(f" F_d2err {e2:.2e} / {s2:.2e} F_d2err_dx {e3:.2e} / {s3:.2e}")
    assert e2 <= fac * (T2 * s2 + T2_ABS), (test, "F_d2err", e2, s2)
    assert e3 <= fac * (T3 * s3 + T3_ABS), (test, "F_d2err_dx", e3, s3)
    if got[3].ndim == 2:  # one evaluation: the x_add rows against their exact value (or the stencil residue's bound)
        check_xadd(test, got[3], ref[3], nmain, xadd_exact, rel=T3 * fac, ab=T3_ABS * fac)


_DONE = {}   # results of _evaluate by its arguments: shared by the table tests and the exact comparison


def _evaluate(name, nt, options, scan_waves=0, projector=None, oracle_rows=ORACLE_ROWS, **over):
    """The case `name` (sector_problems.case_problem arguments `over`) on the sector plan and on the whole-matrix
    plan, four evaluations each, and on the oracle (closure form) for `oracle_rows`; every comparison made."""
    from oracle import grape_oracle as O
    from robustgrape_amd.operators import OPT_NO_SECTORS
    key = (name, nt, options, scan_waves, projector, oracle_rows, tuple(sorted(over.items())))
    if key in _DONE:
        return _DONE[key]
    fp, fo = SP.case_problem(name, nt, **over), SP.case_problem(name, nt, device=False, **over)
    d = fp.unitary_problem.ndim
    if projector == "dense":
        P0 = SP.dense_projector(d, seed=d)
        fp, fo = fp.replace(projector=P0), fo.replace(projector=P0)
    nparam, na = over.get("nparam", 1), fp.unitary_problem.nb_additional_param
    X = SP.case_x(name, nt, nparam, na)[:NB]
    sec, info, out = _run(fp, X, options, nparam, scan_waves)
    whole, _, ref = _run(fp, X, options | OPT_NO_SECTORS, nparam)
    assert whole == ((d, 1),)
    label = f"{name}_nt{nt}_" + "_".join(f"{k}{v}" for k, v in sorted(over.items()) if k != "weights") + (projector or "")
    _compare(label + "_vs_whole", out, ref, fp, X, nparam)
    oracle = {}
    for b in oracle_rows:
        oracle[b] = O.calculate_fidelity_and_derivatives(fo, X[b])
        _compare(f"{label}_vs_oracle_{b}", [o[b] for o in out], oracle[b], fp, X[b], nparam,
                 exact_rows(fp, X[b], nparam) if fp.unitary_problem.error_sources else None)
    res = dict(fp=fp, X=X, sec=sec, info=info, out=out, ref=ref, oracle=oracle, nparam=nparam)
    _DONE[key] = res
    return res


def _nosym():
    from robustgrape_amd.operators import OPT_NO_SYMMETRY
    return OPT_NO_SYMMETRY


# the table, and the merge case without the error source that couples two of H0's components
TABLE = [(n, {}, SP.CASES[n][3]) for n in sorted(SP.CASES)] + [("merge", dict(nerr=0, err_couples=None), SP.MERGE_WITHOUT)]


@pytest.mark.parametrize("nt", [NT, 1])
@pytest.mark.parametrize("name,over,layout", TABLE, ids=[n + ("-h0" if o else "") for n, o, _ in TABLE])
def test_table_case_matches_whole_matrices_and_oracle(name, over, layout, nt):
    r = _evaluate(name, nt, _nosym(), scan_waves=1, **over)
    assert r["sec"] == layout and r["info"]["symmetric"] == 0


VARIANTS = [
    ("c3221", dict(nerr=2), None), ("c4321f", dict(nerr=2), None), ("c431", dict(nerr=2), None),
    ("c55", dict(nerr=1), None),                       # the error path on a non-walking class
    ("c431", dict(nparam=2), None), ("c532f", dict(nparam=2), None),
    # H0 reading x_add: that row of F_dx sums one forward difference per step, each with u / eps ~ 1e-8 of rounding
    # noise in any double implementation -- at 37 steps the oracle itself is 4.3e-7 from the longdouble value on
    # c3221 (its C port 2.2e-7 on the other side) where the short-step tier allows 3.1e-7.  So these two run at
    # |dt H|_1 = 0.5, in the T2 tier (1e-6 max|F_dx| + 1e-7), as the Rydberg x_add tests do with their long steps.
    ("c3221", dict(nerr=2, xadd_h0=True, step_norm=0.5), None), ("c55", dict(nerr=2, xadd_h0=True, step_norm=0.5), None),
    ("q3333", dict(target="dense"), None), ("c4321f", dict(target="dense"), None),
    ("c3221", {}, "dense"), ("c532f", {}, "dense"),    # a dense real rank-3 projector couples every sector
]


@pytest.mark.parametrize("name,over,projector", VARIANTS,
                         ids=[n + "-" + "-".join(f"{k}={w}" for k, w in o.items()) + (p or "") for n, o, p in VARIANTS])
def test_variants(name, over, projector):
    """Error sources, two controls, an H0 and an error source reading x_add, a dense target, a dense projector.
    (nerr = 1 on the merge case is its table entry above.)"""
    r = _evaluate(name, NT, _nosym(), scan_waves=1, projector=projector, **over)
    assert r["sec"] == SP.CASES[name][3] and r["info"]["symmetric"] == 0


@pytest.mark.parametrize("name", ["c4321f", "c55"])
def test_parked_high_norm_steps(name):
    """|dt H|_1 = 8: the sector exponentials square; every tier scales by fd_tier / fd_factor."""
    r = _evaluate(name, 6, _nosym(), scan_waves=1, step_norm=8.0)
    assert r["sec"] == SP.CASES[name][3]
    assert P.fd_tier(r["fp"], r["X"])[0] > 1e-6  # beyond Julia's Pade-13 threshold


# ---------------------------------------------------------------------------------------------------------------
# hidden blocks: the symmetry-adapted sectors behind a complex V
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("projector", [None, "dense"])
@pytest.mark.parametrize("name", sorted(SP.HIDDEN))
def test_hidden_blocks(name, projector):
    """A diagonal lab-basis projector becomes a general complex P0' = V^dag P0 V in the rotated basis."""
    r = _evaluate(name, NT_HIDDEN, 0, projector=projector)
    assert r["info"]["symmetric"] == 1 and r["sec"] == SP.HIDDEN[name][2]
    no = _run(r["fp"], r["X"], _nosym())  # no permutation sectors exist
    assert no[0] == ((r["fp"].unitary_problem.ndim, 1),) and no[1]["symmetric"] == 0


def test_hidden_blocks_with_an_error_source():
    r = _evaluate("h3+22", NT_HIDDEN, 0, nerr=1)
    assert r["info"]["symmetric"] == 1 and r["sec"] == SP.HIDDEN["h3+22"][2]


def test_hidden_twin_blocks():
    """h3+22: the 2-level block of multiplicity two.  sector_info()["twin"] is what grape_plan_build.hip decide_class's
    conditions give (a walking 2-level class of two sectors without error sources whose blocks of every H0
    operator are identical, bit for bit), and GRAPE_OPT_NO_TWIN changes no number beyond the tiers."""
    from robustgrape_amd.operators import OPT_NO_TWIN
    from tests.test_symmetry_cpu import _basis
    r = _evaluate("h3+22", NT_HIDDEN, 0)
    fp, X = r["fp"], r["X"]
    rc, V, blk, _ = _basis(fp)
    assert rc == 1
    a, b = [np.flatnonzero(blk == k) for k in sorted(set(blk.tolist())) if np.sum(blk == k) == 2]
    diff = big = 0.0
    for t in fp.unitary_problem.H0.terms:
        R = V.conj().T @ t.op @ V
        diff = max(diff, float(np.max(np.abs(R[np.ix_(a, a)] - R[np.ix_(b, b)]))))
        big = max(big, float(np.max(np.abs(R))))
    assert diff == 0.0 or diff > 1e-6 * big, diff  # the bitwise comparison is predictable from here
    assert r["info"]["twin"] == (False, diff == 0.0), (r["info"], diff)
    sec, info, out = _run(fp, X, OPT_NO_TWIN)
    assert sec == r["sec"] and info["twin"] == (False, False)
    _compare("h3+22_notwin_vs_default", out, r["out"], fp, X, 1)


# ---------------------------------------------------------------------------------------------------------------
# kernel choices must not change the numbers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c3221-idle", "c431", "q3333"])
def test_kernel_choices_agree(name):
    from robustgrape_amd.operators import OPT_GENERAL_HEAD, OPT_NO_EVAL1, OPT_NO_PAIR, OPT_NO_WALK
    r = _evaluate(name, NT, _nosym(), scan_waves=1)
    for label, opt in (("nowalk", OPT_NO_WALK), ("generalhead", OPT_GENERAL_HEAD), ("nopair_noeval1", OPT_NO_PAIR | OPT_NO_EVAL1)):
        for waves in (1, 0):
            sec, _, out = _run(r["fp"], r["X"], _nosym() | opt, scan_waves=waves)
            assert sec == r["sec"]
            _compare(f"{name}_{label}_w{waves}_vs_default", out, r["out"], r["fp"], r["X"], 1)


@pytest.mark.parametrize("name", ["c4321f", "c55"])
def test_split_batches_are_the_single_calls(name):
    """Five evaluations on a plan of max_batch = 2 (three passes, the last one short): bitwise the single calls."""
    from robustgrape_amd.engine import GrapePlan
    fp, X = SP.case_problem(name, NT), SP.case_x(name, NT)
    pl = GrapePlan(fp, nparam=1, device=0, max_batch=2, options=_nosym())
    try:
        assert pl.sectors() == SP.CASES[name][3]
        F, Fdx, _, _ = pl.fidelity_grad(X)
        for b in range(5):
            Fs, gs, _, _ = pl.fidelity_grad(X[b:b + 1])
            assert Fs[0] == F[b] and np.array_equal(gs[0], Fdx[b]), b
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------------------------
# against the exact evaluator
# ---------------------------------------------------------------------------------------------------------------
EXACT = [t for t in TABLE if t[0] != "merge" or t[1]]   # without error sources: the merge case as H0 alone


@pytest.mark.parametrize("name,over,layout", EXACT, ids=[n for n, _, _ in EXACT])
def test_gradient_against_the_exact_forward_difference(name, over, layout):
    """The device's F_dx within fd_tier of oracle/grape_exact.py's longdouble forward difference (no error
    sources, H0 free of x_add); the oracle's own distance, inside the same tier for every case
    (tests/test_sector_shapes_cpu.py), is recorded beside it."""
    from oracle import grape_exact as E
    r = _evaluate(name, NT, _nosym(), scan_waves=1, **over)
    fp, x = r["fp"], r["X"][0]
    F, g = E.fidelity_and_gradient(fp, x)
    t2, t2a = P.fd_tier(fp, x)
    sc = float(np.max(np.abs(g)))
    dev = float(np.max(np.abs(r["out"][1][0] - g)))
    ora = float(np.max(np.abs(np.asarray(r["oracle"][0][1]) - g)))
    record(f"{name}_device_vs_exact", "F_dx", dev, sc, t2 * sc + t2a)
    record(f"{name}_oracle_vs_exact", "F_dx", ora, sc, t2 * sc + t2a)
    print(f"{name}: device - exact {dev:.2e}, oracle - exact {ora:.2e}, scale {sc:.2e}, tier {t2 * sc + t2a:.2e}")
    assert abs(r["out"][0][0] - F) <= T1
    assert dev <= t2 * sc + t2a, (dev, sc)
    assert r["sec"] == layout
