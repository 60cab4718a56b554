"""A scalar reference of the optimiser kernels (csrc/grape_lbfgs.hip), one Python object per row.

Written from Nocedal & Wright alg. 3.5 / 3.6 (strong-Wolfe line search, c1 = 1e-4, c2 = 0.9),
alg. 7.4 (two-loop recursion) and the contract in include/grape.h -- not from the kernels or from
optimize.py's masked torch version.  Dot products accumulate in longdouble; every operation leaves
in `Row.tol` the absolute tolerance of each field a device result may differ in (fields not named
are bitwise), derived from the kernels' reduction shape:

  dot-derived scalars: (ceil(n / 256) + 12) * 2^-52 * sum |a_i b_i|
      (that many serial adds per thread, six shuffle levels, four wave partials)
  step lengths after the cubic: 1e-12 * |a_hi - a_lo| (the width at which a bracket counts as collapsed)
      The step is the longdouble cubic rounded once; ls_end also evaluates it in float64 and reports
      the difference.  The ends of the clamp, lo + 0.1 w and hi - 0.1 w, are rounded once from exact
      rationals: the kernel's multiply-add is fused, and next to a kept point at a = 1 a collapsing
      bracket is narrower than 1e4 units in the last place of a, where a twice-rounded end would
      already sit outside the tolerance.

Also here: the (f_t, phi'_t) scenario table that drives the line search through all of its
transitions, vectors with exact dot products for it, and a longdouble restatement of the fused cost
(grape_robust_cost) with the absolute sums its tolerance is made of.  A helper, not a test.
"""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
C1, C2 = 1e-4, 0.9
EPS = 2.0 ** -52
TRANSITIONS = ("to_zoom_a", "acc_b", "to_zoom_b", "expand", "z_hi", "z_acc", "z_flip", "z_lo")
VEC = ("X", "g", "D", "Xn", "gn")
SCAL = ("f", "fn", "f0", "dphi0", "a_cur", "a_prev", "f_prev", "dp_prev", "a_lo", "f_lo", "dp_lo", "a_hi", "f_hi",
        "dp_hi", "gamma", "g_thr")
INTS = ("f_calls", "iters", "hist", "head", "phase", "first", "accepted", "gconv", "fconv", "xconv", "lsfail",
        "active")
CFG = dict(f_abstol=0.0, f_reltol=0.0, x_abstol=0.0, x_reltol=0.0, iterations=1000, f_calls_limit=0)


def dot(a, b):
    """(sum a_i b_i, sum |a_i b_i|), accumulated in longdouble."""
    p = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
    return float(np.sum(p)), float(np.sum(np.abs(p)))


def dot_tol(n, abs_sum):
    return (math.ceil(n / 256) + 12) * EPS * abs_sum


def cubic_min(a0, f0, g0, a1, f1, g1, T=np.float64):
    """Minimiser of the cubic through (a0, f0, g0), (a1, f1, g1) (N&W eq. 3.59), kept in the middle
    80 % of the interval, bisection where there is none.  Returns (a, clamp, bisected); clamp is
    'lo', 'hi' or None."""
    a0, f0, g0, a1, f1, g1 = (T(v) for v in (a0, f0, g0, a1, f1, g1))
    with np.errstate(all="ignore"):
        d1 = g0 + g1 - T(3) * (f0 - f1) / (a0 - a1)
        disc = d1 * d1 - g0 * g1
        d2 = np.sign(a1 - a0) * np.sqrt(max(disc, T(0)))
        den = g1 - g0 + T(2) * d2
        a = a1 - (a1 - a0) * (g1 + d2 - d1) / den
    lo, hi = min(a0, a1), max(a0, a1)
    w = hi - lo
    bisected = not (disc >= 0 and np.isfinite(a) and den != 0)
    if bisected:
        a = T(0.5) * (a0 + a1)
    if T is LD:  # the clamp's two ends rounded once (a fused multiply-add), exactly
        w64 = Fraction(float(np.float64(hi) - np.float64(lo)))
        lo_c = LD(float(Fraction(float(lo)) + Fraction(0.1) * w64))
        hi_c = LD(float(Fraction(float(hi)) - Fraction(0.1) * w64))
    else:
        lo_c, hi_c = lo + T(0.1) * w, hi - T(0.1) * w
    clamp = "lo" if a < lo_c else "hi" if a > hi_c else None
    return min(max(a, lo_c), hi_c), clamp, bisected


class Row:
    """One restart's state (the per-row slice of grape_lbfgs_state) and the operations on it."""

    def __init__(self, n, m, **cfg):
        self.n, self.m = n, m
        for k in VEC:
            setattr(self, k, np.zeros(n))
        for k in SCAL:
            setattr(self, k, 0.0)
        for k in INTS:
            setattr(self, k, 0)
        self.gamma = 1.0
        self.S, self.Y, self.rho = np.zeros((m, n)), np.zeros((m, n)), np.zeros(m)
        self.cfg = dict(CFG, **cfg)
        self.min_margin = math.inf  # the narrowest comparison so far, relative to its larger side
        self.tol = {}
        self.last_s = None  # s = Xn - X of the last step (the kernels leave it in the row's Xt)
        self.upd_slot = None  # the ring slot the last step wrote, if any

    def _cmp(self, left, right, scale=None):
        """Record how far apart the two sides of a decision are (relative to `scale`, default the
        larger side)."""
        sc = max(abs(left), abs(right)) if scale is None else scale
        self.min_margin = min(self.min_margin, abs(left - right) / sc if sc > 0 else 0.0)

    # -- alg. 7.4 -------------------------------------------------------------------------------
    def direction(self):
        """D = -H g from the newest `hist` pairs (newest in slot head - 1), in longdouble."""
        q = -self.g.astype(LD)
        alpha = []
        slots = [(self.head - 1 - j) % self.m for j in range(self.hist)]
        for slot in slots:  # newest first
            a = LD(self.rho[slot]) * np.sum(self.S[slot].astype(LD) * q)
            alpha.append(a)
            q = q - a * self.Y[slot].astype(LD)
        q = q * LD(self.gamma)
        for j in reversed(range(self.hist)):  # oldest first
            slot = slots[j]
            b = LD(self.rho[slot]) * np.sum(self.Y[slot].astype(LD) * q)
            q = q + (alpha[j] - b) * self.S[slot].astype(LD)
        self.D = q.astype(np.float64)
        self.tol = {"D": 1e-13 * float(np.max(np.abs(q))) if self.n else 0.0}
        return q

    # -- start of a line search -----------------------------------------------------------------
    def ls_init(self, d_err=0.0):
        """d_err: the absolute error the caller allows on D's entries (a direction computed on the
        device), carried into the tolerance of phi'(0)."""
        c = self.cfg
        active = (not (self.gconv or self.fconv or self.xconv or self.lsfail) and self.iters < c["iterations"]
                  and (c["f_calls_limit"] <= 0 or self.f_calls < c["f_calls_limit"]))
        d0, ab = dot(self.g, self.D)
        t0 = dot_tol(self.n, ab) + d_err * float(np.sum(np.abs(self.g)))
        self.tol = {}
        if active:
            self._cmp(d0, 0.0, ab)
        if active and not d0 < 0:  # not a descent direction: steepest descent, history dropped
            self.D = -self.g
            d0, ab = dot(self.g, self.D)
            t0 = dot_tol(self.n, ab)
            self.hist, self.gamma = 0, 1.0
        elif d_err:
            self.tol["D"] = d_err
        self.Xn, self.gn = self.X.copy(), self.g.copy()
        self.active, self.phase = int(active), 0 if active else 2
        self.dphi0 = self.dp_prev = self.dp_lo = self.dp_hi = d0
        self.f0 = self.fn = self.f_prev = self.f_lo = self.f_hi = self.f
        self.a_cur, self.a_prev, self.a_lo, self.a_hi = 1.0, 0.0, 0.0, 0.0
        self.accepted, self.first = 0, 1
        for k in ("dphi0", "dp_prev", "dp_lo", "dp_hi"):
            self.tol[k] = t0

    def trial(self):
        return self.X + self.a_cur * self.D

    # -- one trial evaluation: alg. 3.5 while bracketing, alg. 3.6 in zoom ------------------------
    def ls_end(self, Xt, ft, gt):
        a, ft = self.a_cur, float(ft)
        dpt, ab = dot(gt, self.D)
        td = dot_tol(self.n, ab)
        info = {"collapsed": False, "clamp": None, "bisected": False, "cubic_diff": 0.0, "width": 0.0}
        rhs = self.f0 + C1 * a * self.dphi0
        self._cmp(ft, rhs)
        armijo = ft <= rhs
        tol = {}

        def curvature():
            self._cmp(abs(dpt), -C2 * self.dphi0)
            return abs(dpt) <= -C2 * self.dphi0

        def zoom(lo, hi):
            (self.a_lo, self.f_lo, self.dp_lo), (self.a_hi, self.f_hi, self.dp_hi) = lo, hi

        accept = False
        new = (a, ft, dpt)
        if self.phase == 0:
            worse = False
            if armijo and not self.first:
                self._cmp(ft, self.f_prev)
                worse = ft >= self.f_prev
            prev = (self.a_prev, self.f_prev, self.dp_prev)
            if not armijo or worse:
                t = "to_zoom_a"
                zoom(prev, new)
                tol["dp_hi"] = td
                self.phase = 1
            elif curvature():
                t, accept = "acc_b", True
            else:
                self._cmp(dpt, 0.0, ab)
                if dpt >= 0:
                    t = "to_zoom_b"
                    zoom(new, prev)
                    tol["dp_lo"] = td
                    self.phase = 1
                else:
                    t = "expand"
                    self.a_prev, self.f_prev, self.dp_prev = new
                    tol["dp_prev"] = td
                    self.a_cur = 4.0 * a
        else:
            assert self.phase == 1, "ls_end on a row that is not searching"
            higher = False
            if armijo:
                self._cmp(ft, self.f_lo)
                higher = ft >= self.f_lo
            if not armijo or higher:
                t = "z_hi"
                self.a_hi, self.f_hi, self.dp_hi = new
                tol["dp_hi"] = td
            elif curvature():
                t, accept = "z_acc", True
            else:
                side = dpt * (self.a_hi - self.a_lo)
                self._cmp(side, 0.0, ab * abs(self.a_hi - self.a_lo))
                t = "z_lo"
                if side >= 0:
                    t = "z_flip"
                    self.a_hi, self.f_hi, self.dp_hi = self.a_lo, self.f_lo, self.dp_lo
                self.a_lo, self.f_lo, self.dp_lo = new
                tol["dp_lo"] = td
        info["transition"] = t
        # the best Armijo point so far is what the step falls back to
        if armijo and not accept:
            self._cmp(ft, self.fn)
        if accept or (armijo and ft < self.fn):
            self.Xn, self.fn, self.gn = np.array(Xt, dtype=np.float64), ft, np.array(gt, dtype=np.float64)
        if accept:
            self.accepted, self.phase = 1, 2
        if self.phase == 1:
            args = (self.a_lo, self.f_lo, self.dp_lo, self.a_hi, self.f_hi, self.dp_hi)
            a64 = cubic_min(*args)[0]
            ald, info["clamp"], info["bisected"] = cubic_min(*args, T=LD)
            width = abs(self.a_hi - self.a_lo)
            info["cubic_diff"] = float(abs(LD(a64) - ald))  # float64 against longdouble
            info["width"] = width
            self.a_cur = float(ald)
            tol["a_cur"] = 1e-12 * width
            if width <= 1e-12 * max(abs(self.a_lo), 1.0):
                self.phase, info["collapsed"] = 2, True
        self.first = 0
        self.tol = tol
        return info

    # -- after the line search: the step, the ring buffer, the stopping rules ----------------------
    def step(self):
        c = self.cfg
        active = bool(self.active)
        if active:
            self._cmp(self.fn, self.f0)
        moved = active and self.fn < self.f0
        stp = active and (bool(self.accepted) or moved)
        s, y = self.Xn - self.X, self.gn - self.g
        sy, sy_abs = dot(s, y)
        yy, yy_abs = dot(y, y)
        dx = float(np.max(np.abs(s)))
        if stp:
            self._cmp(sy, 0.0, sy_abs)
        upd = stp and sy > 0
        slot = self.head
        self.tol = {}
        self.upd_slot = slot if upd else None
        if upd:
            self.S[slot], self.Y[slot] = s, y
        if stp:
            self.X, self.g = self.Xn.copy(), self.gn.copy()
        gmax, xmax = float(np.max(np.abs(self.g))), float(np.max(np.abs(self.X)))
        if active and not moved and not self.accepted:
            self.lsfail = 1
        if upd:
            tsy, tyy = dot_tol(self.n, sy_abs), dot_tol(self.n, yy_abs)
            self.rho[slot] = 1.0 / sy
            self.head = (slot + 1) % self.m
            self.hist = min(self.hist + 1, self.m)
            self.gamma = sy / yy
            self.tol["rho"] = (tsy / abs(sy) + 2 * EPS) / abs(sy)
            self.tol["gamma"] = (tsy / abs(sy) + tyy / yy + 2 * EPS) * abs(self.gamma)
        if stp:
            fold, self.f = self.f, self.fn
            self.iters += 1
            self._cmp(gmax, self.g_thr)
            if gmax <= self.g_thr:
                self.gconv = 1
            df = abs(self.f - fold)
            self._cmp(df, c["f_abstol"])
            self._cmp(df, c["f_reltol"] * abs(self.f))
            if df <= c["f_abstol"] or df <= c["f_reltol"] * abs(self.f):
                self.fconv = 1
            self._cmp(dx, c["x_abstol"])
            self._cmp(dx, c["x_reltol"] * xmax)
            if dx <= c["x_abstol"] or dx <= c["x_reltol"] * xmax:
                self.xconv = 1
        self.D = y  # the kernels keep y in D's row and s in Xt's row r
        self.last_s = s
        return s

    # -- asynchronous rows: the composition -------------------------------------------------------
    def advance(self, steepest, max_rounds, rounds):
        """What grape_lbfgs_async_advance does to this row; returns its new `rounds`."""
        self.last_s = None
        ph = self.phase
        if ph < 2 and rounds >= max_rounds:
            ph = 2
        if ph < 2:
            self.tol = {}
            return rounds + 1
        tol = {}
        if ph == 2:
            if not self.active:
                self.tol = {}
                return rounds
            self.step()
            tol.update(self.tol)
            if steepest:
                self.hist, self.gamma = 0, 1.0
                tol.pop("gamma", None)
        # the direction reads the device's own rho and gamma: their tolerance reaches D through
        # the two-loop linearly in the relative error (a few units of 2^-52)
        self.direction()
        d_err = self.tol["D"]
        self.ls_init(d_err=d_err)
        tol.update(self.tol)
        self.tol = tol
        return 1 if self.phase < 2 else 0


def minimize(fun, x0, m=10, iterations=1000, g_tol=1e-8, steepest=False, max_rounds=30, log=None, **cfg):
    """One row through the synchronous loop (direction, ls_init, rounds, step) with fun(x) -> (f, g).
    log: a list that receives every ls_end's info."""
    x0 = np.asarray(x0, dtype=np.float64)
    row = Row(x0.shape[0], m, iterations=iterations, **cfg)
    row.X = x0.copy()
    row.f, g = fun(row.X)
    row.g = np.asarray(g, dtype=np.float64)
    row.f_calls = 1
    row.g_thr = g_tol
    row.gconv = int(float(np.max(np.abs(row.g))) <= row.g_thr)
    while True:
        row.direction()
        row.ls_init()
        if not row.active:
            return row
        for _ in range(max_rounds):
            if row.phase >= 2:
                break
            Xt = row.trial()
            row.f_calls += 1
            ft, gt = fun(Xt)
            info = row.ls_end(Xt, ft, gt)
            if log is not None:
                log.append(info)
        row.step()
        if steepest:
            row.hist, row.gamma = 0, 1.0


# ---------------------------------------------------------------------------
# The scenario table: (f_t, phi'_t) per trial, from f0 = 0, phi'(0) = -1, with the transitions
# each must take and how its search ends.  Values are multiplied by SCALE when they are turned
# into vectors, so that every phi' is an integer (the search is invariant under f -> c f).
# ---------------------------------------------------------------------------
SCALE = 20.0
HUGE = (1e6, 1e6)
SCENARIOS = {
    "accept": dict(seq=[(-.5, -.1)], path=["acc_b"], end="accepted"),
    "expand_accept": dict(seq=[(-.5, -.95), (-2, .1)], path=["expand", "acc_b"], end="accepted"),
    "expand_zoomb_flip": dict(seq=[(-.5, -.95), (-2, 3), (-2.5, -2), (-2.6, 0)],
                              path=["expand", "to_zoom_b", "z_flip", "z_acc"], end="accepted"),
    "zooma_hi_lo": dict(seq=[(1, 5), (.5, 2), (-.01, -.95), (-.02, 0)],
                        path=["to_zoom_a", "z_hi", "z_lo", "z_acc"], end="accepted"),
    "zoom_f_prev": dict(seq=[(-.5, -.95), (-.4, -.95), (-.6, 0)], path=["expand", "to_zoom_a", "z_acc"],
                        end="accepted"),
    "clamp_hi": dict(seq=[(-2, 1), (-2.1, 0)], path=["to_zoom_b", "z_acc"], end="accepted"),
    "collapse_fail": dict(seq=[HUGE] * 14, path=["to_zoom_a"] + ["z_hi"] * 13, end="failed"),
    "collapse_moved": dict(seq=[(-.5, -.95)] + [HUGE] * 14, path=["expand", "to_zoom_a"] + ["z_hi"] * 13,
                           end="moved"),
}


def exact_direction(n):
    """D from {+-1/2, +-1, +-2} with D[n - 1] = 1/2: products with small integers are exact."""
    vals = np.array([1.0, -2.0, 0.5, -1.0, 2.0, -0.5])
    D = vals[np.arange(n) % 6]
    D[n - 1] = 0.5
    return D


def exact_vector(P, D, salt=0):
    """Integer-valued v with v . D == P exactly in any summation order.  The sum sits at index 256
    (the second trip of a 256-thread strided loop) and at n - 1 (the tail) where n allows;
    cancelling pairs fill the rest, so a dropped trip or tail changes the dot product."""
    n = D.shape[0]
    assert float(P).is_integer() and D[n - 1] == 0.5
    v = np.zeros(n)
    for i in range(0, n - 2, 2):
        if i in (256, 255):
            continue
        t = 2.0 * ((i * 7 + salt) % 5 - 2)
        v[i], v[i + 1] = t / D[i], -t / D[i + 1]
    rest = float(P)
    if n - 1 > 256:
        part = 2.0 * math.floor(P / 4.0)
        v[256] = part / D[256]
        rest -= part
    v[n - 1] = 2.0 * rest
    assert dot(v, D)[0] == P
    return v


def run_scenario(name, n=1):
    """A scenario through the reference alone: returns (row, infos)."""
    sc = SCENARIOS[name]
    D = exact_direction(n)
    row = Row(n, 3)
    row.g, row.D, row.f = exact_vector(-SCALE, D), D, 0.0
    row.g_thr = 0.0
    row.ls_init()
    infos = []
    for k, (ft, dp) in enumerate(sc["seq"]):
        assert row.phase < 2, f"{name}: the search ended before trial {k}"
        Xt = row.trial()
        infos.append(row.ls_end(Xt, SCALE * ft, exact_vector(SCALE * dp, D, salt=k)))
    return row, infos


# A well-scaled convex test function with an analytic gradient, one (w, c) per row.
def quartic(n, seed=0):
    """sum w_i (x_i - c_i)^2 / 2 + 0.1 sum (x_i - c_i)^4 / 4 with w in [1, 10]: (w, c)."""
    rng = np.random.default_rng(1000 + seed)
    return rng.uniform(1, 10, size=n), rng.uniform(-1, 1, size=n)


def quartic_np(w, c):
    def fun(x):
        u = x - c
        return float(np.sum(w * u * u / 2 + 0.025 * u ** 4)), w * u + 0.1 * u ** 3
    return fun


def quartic_x0(n, seed=0):
    return np.random.default_rng(50 + seed).uniform(-2, 2, size=n)


# ---------------------------------------------------------------------------
# The fused cost (grape_robust_cost) in longdouble, from the definitions: reg1 = sum of squared
# first differences, reg2 = sum of squared second differences of the series y (y = x, or cos x and
# sin x summed for the phase kind), their gradients by the chain rule through each difference.
# Returns (value, S): S is the same expression with every addend replaced by its absolute value
# and every difference y[k+1] - y[k] by |y[k+1]| + |y[k]|.
# ---------------------------------------------------------------------------
def _reg_series(y):
    y = np.asarray(y, dtype=LD)
    n = y.shape[0]
    ay = np.abs(y)
    d, ad = y[1:] - y[:-1], ay[1:] + ay[:-1]
    dd, add = d[1:] - d[:-1], ad[1:] + ad[:-1]
    j1, aj1, j2, aj2 = (np.zeros(n, dtype=LD) for _ in range(4))
    # d_j = y[j+1] - y[j] (j < n - 1): d(d_j^2) = 2 d_j on y[j+1], -2 d_j on y[j]
    j1[1:] += 2 * d
    j1[:-1] -= 2 * d
    aj1[1:] += 2 * ad
    aj1[:-1] += 2 * ad
    # dd_j = y[j+2] - 2 y[j+1] + y[j] (j < n - 2): 2 dd_j times the weights 1, -2, 1
    for off, w in ((0, 1), (1, -2), (2, 1)):
        j2[off:n - 2 + off] += 2 * w * dd
        aj2[off:n - 2 + off] += 2 * abs(w) * add
    return (np.sum(d * d), j1, np.sum(dd * dd), j2), (np.sum(ad * ad), aj1, np.sum(add * add), aj2)


def reg_ref(x, kind):
    """((reg1, jac1, reg2, jac2), the same with absolute addends) of one control's series."""
    x = np.asarray(x, dtype=LD)
    if kind == 1:
        return _reg_series(x)
    assert kind == 2
    cs, sn = np.cos(x), np.sin(x)
    (a, aa), (b, ab) = _reg_series(cs), _reg_series(sn)
    val = (a[0] + b[0], -sn * a[1] + cs * b[1], a[2] + b[2], -sn * a[3] + cs * b[3])
    mag = (aa[0] + ab[0], np.abs(sn) * aa[1] + np.abs(cs) * ab[1], aa[2] + ab[2],
           np.abs(sn) * aa[3] + np.abs(cs) * ab[3])
    return val, mag


def robust_cost_ref(x, F, Fdx, Fd2, Fd2dx, ce, c1, c2, kinds, nt, na):
    """One row of grape_robust_cost: x, Fdx [nx]; Fd2 [ne]; Fd2dx [ne][nx] (the device layout).
    Returns (cost, grad, S_cost, S_grad) in longdouble."""
    npar = len(kinds)
    nx = npar * nt + na
    x = np.asarray(x, dtype=LD)
    Fd2, ce = np.asarray(Fd2, dtype=LD), np.asarray(ce, dtype=LD)
    grad = -np.asarray(Fdx, dtype=LD)
    s_grad = np.abs(grad)
    cost, s_cost = LD(1) - LD(F), LD(1) + abs(LD(F))
    for e in range(Fd2.shape[0]):
        term = 2 * ce[e] * Fd2[e] * np.asarray(Fd2dx[e], dtype=LD)
        grad, s_grad = grad + term, s_grad + np.abs(term)
        cost, s_cost = cost + ce[e] * Fd2[e] ** 2, s_cost + abs(ce[e]) * Fd2[e] ** 2
    assert grad.shape[0] == nx
    for p, kd in enumerate(kinds):
        if kd == 0:
            continue
        val, mag = reg_ref(x[p:npar * nt:npar], kd)
        a1, a2 = LD(c1[p]), LD(c2[p])
        cost, s_cost = cost + a1 * val[0] + a2 * val[2], s_cost + abs(a1) * mag[0] + abs(a2) * mag[2]
        grad[p:npar * nt:npar] += a1 * val[1] + a2 * val[3]
        s_grad[p:npar * nt:npar] += abs(a1) * mag[1] + abs(a2) * mag[3]
    return cost, grad, s_cost, s_grad
