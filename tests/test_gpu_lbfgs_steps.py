"""The optimiser kernels of csrc/grape_lbfgs.hip one call at a time: grape_lbfgs_ls_init / _ls_begin /
_ls_end / _step / _async_advance and grape_lbfgs_direction on crafted grape_lbfgs_state buffers,
the whole state compared after every call with the scalar reference (tests/lbfgs_ref.py), at row
lengths on both sides of the 256-thread strided loops, batch sizes on both sides of the
1 024-thread compaction, and histories of 1 to 64 pairs.  Before each call the reference takes the
device's state, so every call is judged on its own inputs; tolerances are the reference's
(Row.tol: bitwise unless a dot product or the cubic is involved)."""
import ctypes

import numpy as np
import pytest
import torch

from robustgrape_amd import optimize as OPT
from tests import lbfgs_ref as LR
from tests import parity_log

pytestmark = pytest.mark.gpu
INVALID = -1
NS = [1, 255, 256, 257, 513]
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Dev:
    """grape_lbfgs_state on the GPU: torch tensors behind the ctypes struct of optimize._CLbfgsState.
    Everything starts as a NaN / -1 sentinel; load() writes reference rows into it."""

    def __init__(self, R, n, m, **cfg):
        from robustgrape_amd import _capi
        self.L, self.R, self.n, self.m = _capi.lib(), R, n, m
        self.cfg = dict(LR.CFG, **cfg)
        dev, t = "cuda", {}
        for k in LR.VEC + ("Xt",):
            t[k] = torch.full((R, n), NAN, dtype=torch.float64, device=dev)
        for k in OPT._LS_F64:
            if k not in t:
                shape = {"S": (m, R, n), "Y": (m, R, n), "rho": (m, R)}.get(k, (R,))
                t[k] = torch.full(shape, NAN, dtype=torch.float64, device=dev)
        for k in OPT._LS_I64:
            t[k] = torch.full((R,), -1, dtype=torch.int64, device=dev)
        for k in OPT._LS_I32:
            t[k] = torch.full((max(R, 1),), -1, dtype=torch.int32, device=dev)
        self.t = t
        st = OPT._CLbfgsState.get()()
        st.R, st.n, st.m = R, n, m
        for k in OPT._LS_F64 + OPT._LS_I64 + OPT._LS_I32:
            setattr(st, k, t[k].data_ptr())
        c = self.cfg
        st.f_abstol, st.f_reltol, st.x_abstol, st.x_reltol = c["f_abstol"], c["f_reltol"], c["x_abstol"], c["x_reltol"]
        st.iterations, st.f_calls_limit = c["iterations"], c["f_calls_limit"]
        self.st, self.sp = st, ctypes.byref(st)

    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def load(self, rows):
        for k in LR.VEC + LR.SCAL + LR.INTS:
            val = np.stack([np.asarray(getattr(r, k)) for r in rows])
            self.t[k].copy_(torch.as_tensor(val).to(self.t[k].dtype))
        for k in ("S", "Y", "rho"):
            self.t[k].copy_(torch.as_tensor(np.stack([getattr(r, k) for r in rows], axis=1)))

    def snap(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def row(self, snap, r):
        row = LR.Row(self.n, self.m, **self.cfg)
        for k in LR.VEC:
            setattr(row, k, snap[k][r].copy())
        for k in LR.SCAL:
            setattr(row, k, float(snap[k][r]))
        for k in LR.INTS:
            setattr(row, k, int(snap[k][r]))
        row.S, row.Y, row.rho = snap["S"][:, r].copy(), snap["Y"][:, r].copy(), snap["rho"][:, r].copy()
        return row

    def call(self, name, *args):
        code = getattr(self.L, "grape_lbfgs_" + name)(self.sp, *args, self.stream())
        assert code == 0, (name, code)


class Worst:
    """The largest error of a test per kind of quantity, in units of its tolerance (0 for bitwise)."""

    def __init__(self, test):
        self.test, self.w = test, {}

    def add(self, kind, err, tol):
        self.w[kind] = max(self.w.get(kind, 0.0), err / tol if tol else 0.0)

    def report(self):
        print(self.test + ": " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(self.w.items())) + " (of the tolerance)")
        for k, v in self.w.items():
            parity_log.record(self.test, k + " / tol", v, 1.0, 1.0)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def check(row, snap, r, what, worst):
    """The device's row r against the reference row: bitwise, or within row.tol where it names one."""
    for k in LR.VEC + LR.SCAL:
        dev, ref, tol = snap[k][r], getattr(row, k), row.tol.get(k, 0.0)
        if tol == 0.0:
            assert same(dev, ref), (what, r, k, dev, ref)
        else:
            err = float(np.max(np.abs(dev - ref)))
            assert err <= tol, (what, r, k, err, tol)
            worst.add(k if k in ("D", "a_cur", "gamma") else "dot", err, tol)
    for k in LR.INTS:
        assert int(snap[k][r]) == getattr(row, k), (what, r, k, int(snap[k][r]), getattr(row, k))
    assert same(snap["S"][:, r], row.S) and same(snap["Y"][:, r], row.Y), (what, r, "S/Y")
    for slot in range(row.m):
        dev, ref = snap["rho"][slot, r], row.rho[slot]
        if slot == row.upd_slot and "rho" in row.tol:
            assert abs(dev - ref) <= row.tol["rho"], (what, r, "rho", dev, ref)
            worst.add("rho", abs(dev - ref), row.tol["rho"])
        else:
            assert same(dev, ref), (what, r, "rho", slot)


def upload(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def begin_round(d, worst, what):
    """grape_lbfgs_ls_begin checked: rows[0:count) the ascending searching rows, f_calls + 1 on them
    only, their trial points within 2^-52 |a D| (the multiply-add may be fused), the rest of Xt
    untouched.  Returns (state after, compact rows, compact trial points)."""
    pre = d.snap()
    d.t["Xt"].fill_(NAN)
    d.t["rows"].fill_(-1)
    d.call("ls_begin")
    post = d.snap()
    want = [r for r in range(d.R) if pre["phase"][r] < 2]
    cnt = int(post["count"][0])
    assert cnt == len(want) and list(post["rows"][:cnt]) == want, (what, cnt, want)
    assert np.all(post["rows"][cnt:] == -1)
    assert same(post["f_calls"], pre["f_calls"] + np.isin(np.arange(d.R), want)), what
    for i, r in enumerate(want):
        step = pre["a_cur"][r] * pre["D"][r]
        err = np.abs(post["Xt"][i] - (pre["X"][r] + step))
        assert np.all(err <= LR.EPS * np.abs(step)), (what, r, float(np.max(err)))
        worst.add("Xt", float(np.max(err / np.maximum(np.abs(step), 1e-300))), LR.EPS)
    assert np.all(np.isnan(post["Xt"][cnt:])), what
    for k in post:
        if k not in ("Xt", "rows", "count", "f_calls"):
            assert same(post[k], pre[k]), (what, k)
    return post, want, post["Xt"][:cnt].copy()


def end_round(d, pre, want, Xt, ft, gt, worst, what, exact=False):
    """grape_lbfgs_ls_end on the compact batch, every row against the reference; returns the
    rows' infos.  exact: the dot products are exact (integer vectors), so only the cubic's step
    keeps a tolerance; otherwise every decision's margin must exceed 1e-9."""
    refs = [d.row(pre, r) for r in range(d.R)]
    ftd, gtd = upload(ft), upload(gt)
    code = d.L.grape_lbfgs_ls_end(d.sp, len(want), ctypes.c_void_p(ftd.data_ptr()), ctypes.c_void_p(gtd.data_ptr()),
                                  d.stream())
    assert code == 0
    post = d.snap()
    infos = {}
    for i, r in enumerate(want):
        infos[r] = refs[r].ls_end(Xt[i], ft[i], gt[i])
        if exact:
            refs[r].tol = {k: v for k, v in refs[r].tol.items() if k == "a_cur"}
        else:
            assert refs[r].min_margin > 1e-9, (what, r, refs[r].min_margin)
    for r in range(d.R):
        if r not in want:
            refs[r].tol = {}
        check(refs[r], post, r, what, worst)
    return post, infos, refs


def step_call(d, worst, what, advance=None):
    """grape_lbfgs_step (or _async_advance with advance = (steepest, max_rounds, rounds tensor)) on
    every row against the reference, the s vector left in Xt included."""
    pre = d.snap()
    refs = [d.row(pre, r) for r in range(d.R)]
    if advance is None:
        d.call("step")
    else:
        steepest, max_rounds, rounds = advance
        before = rounds.cpu().numpy()
        d.call("async_advance", steepest, max_rounds, ctypes.c_void_p(rounds.data_ptr()))
    post = d.snap()
    for r, row in enumerate(refs):
        if advance is None:
            row.step()
        else:
            new_rounds = row.advance(steepest, max_rounds, int(before[r]))
            assert int(rounds[r]) == new_rounds, (what, r, int(rounds[r]), new_rounds)
        check(row, post, r, what, worst)
        if row.last_s is not None:
            assert same(post["Xt"][r], row.last_s), (what, r, "s in Xt")
        else:
            assert same(post["Xt"][r], pre["Xt"][r]), (what, r, "Xt")
    return post, refs


def crafted_rows(n, m, count, seed):
    """Rows for a scenario batch: random X, f = 0, g . D = -SCALE exactly."""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(count):
        row = LR.Row(n, m)
        row.X = rng.uniform(-1, 1, size=n)
        row.D = LR.exact_direction(n)
        row.g = LR.exact_vector(-LR.SCALE, row.D, salt=r)
        row.Xn, row.gn = rng.normal(size=n), rng.normal(size=n)  # overwritten by ls_init
        rows.append(row)
    return rows


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_ls_init(n):
    """Active and inactive rows (each stop flag, the iteration cap, the call limit and its 0 = none),
    a direction that is no descent direction (D <- -g, history dropped), phi'(0) = 0, and a row of
    random vectors; exact vectors whose dot product sits in the second trip and the tail."""
    worst = Worst(f"ls_init n={n}")
    rng = np.random.default_rng(n)
    rows = crafted_rows(n, 3, 8, seed=n)
    for r, flag in ((1, "gconv"), (2, "fconv"), (3, "xconv"), (4, "lsfail")):
        setattr(rows[r], flag, 1)
    rows[5].iters = 7
    for r, p in ((6, 20.0), (7, 0.0)):
        rows[r].g = LR.exact_vector(p, rows[r].D)
        rows[r].hist, rows[r].head, rows[r].gamma = 2, 2, 0.7
    for row in rows:
        row.f, row.g_thr = float(rng.normal()), 1e-8
    d = Dev(8, n, 3, iterations=7)
    d.load(rows)
    d.call("ls_init")
    post = d.snap()
    for r, row in enumerate(rows):
        row.cfg = d.cfg
        row.ls_init()
        row.tol = {}  # exact vectors: bitwise
        check(row, post, r, "ls_init", worst)
        assert row.active == (r in (0, 6, 7))
    assert rows[6].hist == rows[7].hist == 0 and same(post["D"][7], -rows[7].g) and post["dphi0"][0] == -LR.SCALE
    # the call limit, and random vectors (tolerance of the dot product)
    rows = crafted_rows(n, 3, 3, seed=n + 1)
    rows[0].f_calls, rows[1].f_calls, rows[2].f_calls = 5, 4, 0
    rows[1].g = rng.normal(size=n)
    rows[1].D = -rng.uniform(0.5, 2, size=n) * rows[1].g
    d = Dev(3, n, 3, iterations=7, f_calls_limit=5)
    d.load(rows)
    d.call("ls_init")
    post = d.snap()
    for r, row in enumerate(rows):
        row.cfg = d.cfg
        row.ls_init()
        check(row, post, r, "ls_init limit", worst)
    assert [row.active for row in rows] == [0, 1, 1] and rows[1].min_margin > 1e-9
    worst.report()


@pytest.mark.parametrize("n", NS)
def test_line_search_scenarios(n):
    """The scenario table, one scenario per row of one batch, so rows in different phases (and rows
    that finished) share every launch: ls_init, then ls_begin / ls_end rounds until no row
    searches, then the step.  Every row takes its scenario's transitions and ends as the table
    says: accepted, moved without acceptance after a collapsed bracket, or ls_failed."""
    worst = Worst(f"ls scenarios n={n}")
    names = list(LR.SCENARIOS)
    R = len(names)
    d = Dev(R, n, 3)
    rows = crafted_rows(n, 3, R, seed=100 + n)
    d.load(rows)
    d.call("ls_init")
    post = d.snap()
    for r, row in enumerate(rows):
        row.ls_init()
        row.tol = {}
        check(row, post, r, "ls_init", worst)
    paths = {r: [] for r in range(R)}
    collapsed = {}
    for rnd in range(OPT.MAX_LS_ROUNDS):
        pre, want, Xt = begin_round(d, worst, f"round {rnd}")
        if not want:
            break
        ft, gt = np.zeros(len(want)), np.zeros((len(want), n))
        for i, r in enumerate(want):
            f, dp = LR.SCENARIOS[names[r]]["seq"][len(paths[r])]
            ft[i], gt[i] = LR.SCALE * f, LR.exact_vector(LR.SCALE * dp, pre["D"][r], salt=rnd)
        post, infos, refs = end_round(d, pre, want, Xt, ft, gt, worst, f"round {rnd}", exact=True)
        for r, info in infos.items():
            paths[r].append(info["transition"])
            collapsed[r] = info["collapsed"]
    assert not want and rnd == 15  # collapse_moved needs 15 trials
    post, refs = step_call(d, worst, "step")
    for r, name in enumerate(names):
        sc = LR.SCENARIOS[name]
        assert paths[r] == sc["path"], (name, paths[r])
        end = "accepted" if post["accepted"][r] else "failed" if post["lsfail"][r] else "moved"
        assert end == sc["end"] and collapsed[r] == (end != "accepted"), (name, end)
        assert int(post["iters"][r]) == (end != "failed")
    worst.report()


GENERIC = [(n, 3) for n in NS] + [(257, 1), (513, 1), (257, 10), (513, 10)]


@pytest.mark.parametrize("n,m", GENERIC)
def test_iterations_on_random_vectors(n, m):
    """Four synchronous iterations (direction, ls_init, rounds, step) of five quartic rows, every
    call against the reference with the dot products' tolerance; the seeds' decision margins are
    asserted in test_lbfgs_ref_cpu.py.  The history grows below m and, for m = 1 and 3, wraps
    (head m - 1 -> 0 with hist staying m)."""
    worst = Worst(f"iterations n={n} m={m}")
    R = 5
    funs = [LR.quartic_np(*LR.quartic(n, seed=r)) for r in range(R)]
    rows = []
    for r in range(R):
        row = LR.Row(n, m)
        row.X = LR.quartic_x0(n, r)
        row.f, row.g = funs[r](row.X)
        row.f_calls, row.g_thr = 1, 1e-12
        rows.append(row)
    d = Dev(R, n, m)
    d.load(rows)
    heads = []
    for it in range(4):
        pre = d.snap()
        refs = [d.row(pre, r) for r in range(R)]
        code = d.L.grape_lbfgs_direction(R, n, m, *[ctypes.c_void_p(d.t[k].data_ptr()) for k in
                                                     ("S", "Y", "rho", "head", "hist", "gamma", "g", "D")], d.stream())
        assert code == 0
        post = d.snap()
        for r, row in enumerate(refs):
            row.direction()
            check(row, post, r, f"direction {it}", worst)
        refs = [d.row(post, r) for r in range(R)]
        d.call("ls_init")
        post = d.snap()
        for r, row in enumerate(refs):
            row.ls_init()
            check(row, post, r, f"ls_init {it}", worst)
            assert row.active
        for rnd in range(OPT.MAX_LS_ROUNDS):
            pre, want, Xt = begin_round(d, worst, f"it {it} round {rnd}")
            if not want:
                break
            vals = [funs[r](Xt[i]) for i, r in enumerate(want)]
            ft, gt = np.array([v[0] for v in vals]), np.stack([v[1] for v in vals])
            end_round(d, pre, want, Xt, ft, gt, worst, f"it {it} round {rnd}")
        post, refs = step_call(d, worst, f"step {it}")
        assert all(row.upd_slot is not None and row.min_margin > 1e-9 for row in refs)
        heads.append(int(post["head"][0]))
        assert list(post["hist"]) == [min(it + 1, m)] * R and list(post["iters"]) == [it + 1] * R
    assert heads == [(it + 1) % m for it in range(4)]
    worst.report()


@pytest.mark.parametrize("R", [1, 1023, 1024, 1025, 2500])
def test_ls_begin_compaction(R):
    """k_ls_compact with one and with several rows per thread, R no multiple of 1 024, phases drawn
    from {0, 1, 2, 3} (3: a row that has not started), and the all-searching and none-searching
    batches."""
    worst = Worst(f"ls_begin R={R}")
    rng = np.random.default_rng(R)
    d = Dev(R, 3, 1)
    d.t["X"].copy_(upload(rng.normal(size=(R, 3))))
    d.t["D"].copy_(upload(rng.normal(size=(R, 3))))
    d.t["a_cur"].copy_(upload(rng.uniform(0.1, 4, size=R)))
    for kind, phases in (("mixed", rng.integers(0, 4, size=R)), ("all", rng.integers(0, 2, size=R)),
                         ("none", rng.integers(2, 4, size=R))):
        d.t["phase"].copy_(upload(phases, torch.int32))
        d.t["f_calls"].copy_(upload(rng.integers(1, 50, size=R), torch.int64))
        _, want, _ = begin_round(d, worst, kind)
        assert len(want) == int(np.sum(phases < 2))
        assert (kind != "all" or len(want) == R) and (kind != "none" or not want)
    worst.report()


# each stopping rule's threshold at the value it is compared with (|g|_inf = 50, |df| = 0.5 = |f|,
# |dx|_inf = 8, |x|_inf = 128, so every product is exact): it trips with <=, and one unit in the last
# place below it does not
TRIPS = {"g_thr": 50.0, "f_abstol": 0.5, "f_reltol": 1.0, "x_abstol": 8.0, "x_reltol": 0.0625}


@pytest.mark.parametrize("n,m", [(n, 3) for n in NS] + [(513, 1), (257, 10)])
def test_step_cases(n, m):
    """grape_lbfgs_step on crafted ends of a line search: accepted; moved only; neither (ls_failed,
    X, f and g untouched); s.y <= 0 with an accepted step (X moves; history, head and gamma do
    not); the ring wrapping (head m - 1 -> 0, hist staying m); hist growing below m; an inactive
    row untouched; every other slot of S / Y / rho keeps its NaN sentinel.  Then each stopping rule
    alone, its threshold exactly at and one unit in the last place below the row maximum it is
    compared with; that maximum sits in the last entry, so a row_amax that dropped its second trip
    or its tail would trip the rule below the threshold, or miss it at the threshold."""
    worst = Worst(f"step n={n} m={m}")
    for trip, at in [(None, None)] + [(k, f) for k in TRIPS for f in (True, False)]:
        rng = np.random.default_rng(n + 7 * m)
        thr = 0.0 if trip is None else TRIPS[trip] if at else float(np.nextafter(TRIPS[trip], 0.0))
        cfg = {trip: thr} if trip and trip != "g_thr" else {}
        rows = []
        for r in range(6):
            row = LR.Row(n, m, **cfg)
            row.X, row.g = rng.normal(size=n), rng.normal(size=n)
            s = rng.normal(size=n)
            s[n - 1], row.X[n - 1] = 8.0, 120.0
            row.Xn = row.X + s
            y = (-1.0 if r == 3 else 1.0) * rng.uniform(1, 3, size=n) * s
            row.g[n - 1] = 50.0 - y[n - 1]
            row.gn = row.g + y
            row.gn[n - 1] = 50.0
            assert row.Xn[n - 1] == 128.0 and row.gn[n - 1] == 50.0
            assert np.max(np.abs(row.Xn[:n - 1]), initial=0) < 8 and np.max(np.abs(row.gn[:n - 1]), initial=0) < 50
            row.D, row.S, row.Y, row.rho = rng.normal(size=n), row.S * NAN, row.Y * NAN, row.rho * NAN
            row.f = row.f0 = 1.0
            row.fn, row.accepted, row.active, row.phase = 0.5, 1, 1, 2
            row.gamma, row.g_thr, row.iters, row.f_calls = 0.7, thr if trip == "g_thr" else 0.0, 3, 9
            row.head, row.hist = (0, 0) if m == 1 else (1, 1)
            rows.append(row)
        rows[1].accepted = 0                               # moved only
        rows[2].accepted, rows[2].fn = 0, 1.0              # neither
        rows[2].Xn, rows[2].gn = rows[2].X.copy(), rows[2].g.copy()
        rows[4].head, rows[4].hist = m - 1, m              # wrap
        rows[5].active = 0                                 # inactive (a converged row keeps its last Xn)
        d = Dev(6, n, m, **cfg)
        d.load(rows)
        post, refs = step_call(d, worst, f"step trip={trip} at={at}")
        moved = [0, 1, 3, 4]
        assert [r for r in range(6) if refs[r].upd_slot is not None] == [0, 1, 4]
        assert [int(v) for v in post["lsfail"]] == [0, 0, 1, 0, 0, 0]
        assert [int(v) for v in post["iters"]] == [4 if r in moved else 3 for r in range(6)]
        assert (int(post["head"][4]), int(post["hist"][4])) == (0, m)
        assert (int(post["head"][3]), float(post["gamma"][3])) == (rows[3].head, 0.7)
        for r in (2, 5):
            assert same(post["X"][r], rows[r].X) and same(post["g"][r], rows[r].g) and post["f"][r] == 1.0
        assert int(np.sum(~np.isnan(post["rho"]))) == 3
        for flag, by in (("gconv", ("g_thr",)), ("fconv", ("f_abstol", "f_reltol")),
                         ("xconv", ("x_abstol", "x_reltol"))):
            assert [int(v) for v in post[flag]] == [int(bool(at) and trip in by and r in moved) for r in range(6)], \
                (trip, at, flag)
    worst.report()


@pytest.mark.parametrize("steepest", [0, 1])
@pytest.mark.parametrize("n,m", [(n, 3) for n in NS] + [(513, 1), (513, 10)])
def test_async_advance(n, m, steepest):
    """One batch with a row that has not started (phase 3), a searching row below max_rounds, a
    searching row at max_rounds (its search ends: it steps on the point it kept), a finished active
    row with a full, wrapped history, and a finished inactive row: the reference's step -> clear
    (steepest) -> direction -> ls_init and its `rounds` bookkeeping."""
    worst = Worst(f"async_advance n={n} m={m} steepest={steepest}")
    rng = np.random.default_rng(31 * n + m)
    rows = []
    for r in range(5):
        row = LR.Row(n, m)
        row.X, row.g = rng.normal(size=n), rng.normal(size=n)
        s = rng.normal(size=n) + (0.5 if n == 1 else 0.0)
        row.Xn, row.gn = row.X + s, row.g + rng.uniform(1, 3, size=n) * s
        row.D = -rng.uniform(0.5, 2, size=n) * row.g
        row.S = rng.normal(size=(m, n))
        row.Y = row.S * rng.uniform(1, 3, size=(m, n))  # every pair has s . y > 0: H stays positive definite
        row.rho = 1.0 / np.sum(row.S * row.Y, axis=1)
        row.hist, row.head = (m, m // 2) if r == 3 else (min(1, m), 1 % m)
        row.gamma, row.g_thr, row.f_calls, row.iters = 0.8, 1e-12, 6, 2
        row.f = row.f0 = 1.0
        row.fn, row.active, row.phase, row.a_cur = 0.5, 1, 1, 0.3
        row.dphi0 = LR.dot(row.g, row.D)[0]
        rows.append(row)
    rows[0].phase, rows[0].active, rows[0].hist, rows[0].head, rows[0].iters = 3, 0, 0, 0, 0
    rows[3].phase, rows[3].accepted = 2, 1
    rows[4].phase, rows[4].active, rows[4].gconv = 2, 0, 1
    d = Dev(5, n, m)
    d.load(rows)
    d.t["Xt"].copy_(upload(rng.normal(size=(5, n))))
    rounds = upload(np.array([0, 3, 5, 2, 0]), torch.int32)
    post, refs = step_call(d, worst, "advance", advance=(steepest, 5, rounds))
    assert [int(v) for v in rounds] == [1, 4, 1, 1, 0]
    assert [int(v) for v in post["iters"]] == [0, 2, 3, 3, 2]
    assert [int(v) for v in post["phase"]] == [0, 1, 0, 0, 2]
    assert [int(v) for v in post["hist"]] == [0, min(1, m), 0 if steepest else min(2, m), 0 if steepest else m,
                                              min(1, m)]
    assert all(refs[r].min_margin > 1e-9 for r in (0, 2, 3))
    bad = ctypes.c_void_p(rounds.data_ptr())
    assert d.L.grape_lbfgs_async_advance(d.sp, 0, 0, bad, d.stream()) == INVALID
    worst.report()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("m", [1, 64])
def test_direction_at_the_history_limits(m, n):
    """grape_lbfgs_direction with one pair of history and with 64 (the alpha LDS array full), hist in
    {0, 1, m - 1, m} and wrapped heads, against the longdouble two-loop: 1e-13 max|ref| per row (a
    float64 numpy two-loop sits within 1.4e-15 of longdouble at m = 64; the margin is for the
    other summation tree)."""
    rng = np.random.default_rng(64 * n + m)
    R = 5
    S = rng.normal(size=(m, R, n))
    Y = S + 0.3 * rng.normal(size=(m, R, n))
    rho = 1.0 / np.sum(S * Y, axis=-1)
    hist = np.array([0, 1, m - 1, m, m])
    head = np.array([0, 0, m // 2, m - 1, 1 % m])
    gamma, g = rng.uniform(0.5, 1.5, size=R), rng.normal(size=(R, n))
    dev = [upload(a) for a in (S, Y, rho)] + [upload(head, torch.int64), upload(hist, torch.int64), upload(gamma),
                                              upload(g)]
    out = OPT._device_direction(*dev).cpu().numpy()
    worst = 0.0
    for r in range(R):
        row = LR.Row(n, m)
        row.S, row.Y, row.rho, row.g = S[:, r], Y[:, r], rho[:, r], g[r]
        row.hist, row.head, row.gamma = int(hist[r]), int(head[r]), float(gamma[r])
        ref = row.direction()
        err = float(np.max(np.abs(out[r].astype(LR.LD) - ref)) / np.max(np.abs(ref)))
        worst = max(worst, err)
        assert err <= 1e-13, (r, err)
    assert same(out[0], -gamma[0] * g[0])
    print(f"direction m={m} n={n}: worst {worst:.2e} of max|ref| (bound 1e-13)")
    parity_log.record(f"direction m={m} n={n}", "D", worst, 1.0, 1e-13)


def test_direction_refuses_bad_history_sizes():
    from robustgrape_amd import _capi
    t = upload(np.zeros(8))
    i = upload(np.zeros(1), torch.int64)
    p = lambda a: ctypes.c_void_p(a.data_ptr())  # noqa: E731
    for m in (0, 65):
        code = _capi.lib().grape_lbfgs_direction(1, 1, m, p(t), p(t), p(t), p(i), p(i), p(t), p(t), p(t),
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == INVALID


def test_whole_run_at_benchmark_row_length():
    """n = 513 (the benchmark's row length), R = 5: the device path against the CPU torch path over
    the first 4 iterations of the quartic: equal iterations and call counts, minimisers to 1e-10."""
    n, R = 513, 5
    wc = [LR.quartic(n, seed=r) for r in range(R)]
    W, C = (np.stack([p[k] for p in wc]) for k in (0, 1))
    X0 = np.stack([LR.quartic_x0(n, r) for r in range(R)])

    def make(dev):
        w, c = torch.as_tensor(W, device=dev), torch.as_tensor(C, device=dev)

        def fun(X, rows):
            u = X - c[rows]
            return torch.sum(w[rows] * u * u / 2 + 0.025 * u ** 4, dim=1), w[rows] * u + 0.1 * u ** 3
        return fun
    a = OPT.lbfgs_batched(make("cuda"), torch.as_tensor(X0, device="cuda"), iterations=4, g_tol=1e-12)
    b = OPT.lbfgs_batched(make("cpu"), torch.as_tensor(X0), iterations=4, g_tol=1e-12)
    assert a.extra.get("device_ls") and not b.extra.get("device_ls")
    assert torch.equal(a.iterations.cpu(), b.iterations) and torch.equal(a.f_calls.cpu(), b.f_calls)
    assert list(b.iterations) == [4] * R
    err = float((a.minimizer.cpu() - b.minimizer).abs().max())
    print(f"whole run n=513: max |x_dev - x_cpu| = {err:.2e}")
    parity_log.record("whole run n=513", "minimizer", err, float(b.minimizer.abs().max()), 1e-10)
    assert torch.allclose(a.minimizer.cpu(), b.minimizer, rtol=1e-10, atol=1e-12)
