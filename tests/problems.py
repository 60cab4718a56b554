"""Problem builders shared by the tests: the reference's test/example problems
(test/runtests.jl, examples/*.jl) and the SURVEY.md section 8d configs, each in
closure form (reference idiom, host-evaluated) and operator-basis form (device)."""
from __future__ import annotations

import math

import numpy as np

from robustgrape_amd import rydberg as R
from robustgrape_amd.types import ErrorSource, FidelityRobustGRAPEProblem, UnitaryRobustGRAPEProblem

T0_TEST = 2 * math.pi * 1.22     # runtests.jl:53
T0_TO = 7.613                    # examples/time_optimal_cz.jl:14
W_SYM = np.diag([1.0, 2.0, 1.0, 0.0, 0.0])   # runtests.jl:73
W_FULLBLK = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0])  # runtests.jl:492
W_FULL9 = np.diag([1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def sym_problem(ntimes, t0=T0_TEST, errors=(), device=True, delta=0.0):
    """d=5 symmetric blockaded CZ (runtests.jl:57-75); errors subset of {'amp','freq'}; delta: H0's
    detuning (the reference's tests leave it 0)."""
    if device:
        H0 = R.rydberg_symmetric_blockaded_operator_basis(delta=delta)
        errs = [ErrorSource(R.symmetric_amplitude_error() if e == "amp" else R.symmetric_frequency_error())
                for e in errors]
        target = R.cz_symmetric_target()
    else:
        H0 = lambda t, p, xa: R.rydberg_hamiltonian_symmetric_blockaded(p[0], 0, delta)
        amp = lambda t, p, xa, e: (R.rydberg_hamiltonian_symmetric_blockaded(p[0], e, 0)
                                   - R.rydberg_hamiltonian_symmetric_blockaded(p[0], 0, 0))
        frq = lambda t, p, xa, e: (R.rydberg_hamiltonian_symmetric_blockaded(p[0], 0, e)
                                   - R.rydberg_hamiltonian_symmetric_blockaded(p[0], 0, 0))
        errs = [ErrorSource(amp if e == "amp" else frq) for e in errors]
        target = lambda xa: R.cz_with_1q_phase_symmetric(xa[0])
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=5, H0=H0, nb_additional_param=1,
                                   error_sources=errs)
    return FidelityRobustGRAPEProblem(up, W_SYM, target)


def fullblk_problem(ntimes, t0=T0_TO, errors=(), device=True):
    """d=7 full blockaded CZ (runtests.jl:474-494)."""
    if device:
        H0 = R.rydberg_full_blockaded_operator_basis()
        errs = [ErrorSource(R.full_blockaded_amplitude_error() if e == "amp"
                            else R.full_blockaded_frequency_error()) for e in errors]
        target = R.cz_full_target(rydberg_dimension=3)
    else:
        H0 = lambda t, p, xa: R.rydberg_hamiltonian_full_blockaded(p[0], 0, 0)
        amp = lambda t, p, xa, e: (R.rydberg_hamiltonian_full_blockaded(p[0], e, 0)
                                   - R.rydberg_hamiltonian_full_blockaded(p[0], 0, 0))
        frq = lambda t, p, xa, e: (R.rydberg_hamiltonian_full_blockaded(p[0], 0, e)
                                   - R.rydberg_hamiltonian_full_blockaded(p[0], 0, 0))
        errs = [ErrorSource(amp if e == "amp" else frq) for e in errors]
        target = lambda xa: R.cz_with_1q_phase_full(xa[0], rydberg_dimension=3)
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=7, H0=H0, nb_additional_param=1,
                                   error_sources=errs)
    return FidelityRobustGRAPEProblem(up, W_FULLBLK, target)


# sector layouts of the d = 9 Rydberg model (GrapePlan.sectors()): with equal Rabi frequencies and
# detunings the atom-swap symmetry splits the 4-level block (include/grape.h GRAPE_OPT_NO_SYMMETRY,
# csrc/grape_symmetry.hpp) -- one 3-level sector + two 2-level ones; single-atom error sources
# (C3) break the symmetry and keep the permutation sectors.
FULL9_SYM = ((3, 1), (2, 2))
FULL9_PERM = ((4, 1), (2, 2))


def full9_problem(ntimes=512, t0=T0_TO, nerr=0, device=True, B=10.0):
    """SURVEY.md 8d C2 (nerr=0) / C3 (nerr=4): d=9 rydberg_hamiltonian_full, Omega=1, B=10."""
    kinds = [("rabi", 1), ("rabi", 2), ("det", 1), ("det", 2)][:nerr]
    if device:
        H0 = R.rydberg_full_operator_basis(1.0, 1.0, 0.0, 0.0, B)
        errs = [ErrorSource(R.full_rabi_error(w) if k == "rabi" else R.full_detuning_error(w))
                for k, w in kinds]
        target = R.cz_full_target()
    else:
        H0 = lambda t, p, xa: R.rydberg_hamiltonian_full(p[0], 1, 1, 0, 0, B)

        def mk(k, w):
            def herr(t, p, xa, e):
                args = [1.0, 1.0, 0.0, 0.0]
                if k == "rabi":
                    args[w - 1] = 1.0 + e
                else:
                    args[1 + w] = e
                return R.rydberg_hamiltonian_full(p[0], *args, B) - R.rydberg_hamiltonian_full(p[0], 1, 1, 0, 0, B)
            return herr
        errs = [ErrorSource(mk(k, w)) for k, w in kinds]
        target = lambda xa: R.cz_with_1q_phase_full(xa[0])
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=9, H0=H0, nb_additional_param=1,
                                   error_sources=errs)
    return FidelityRobustGRAPEProblem(up, W_FULL9, target)


def full9_family(ntimes, t0=T0_TO, om=1.0, om01=None, delta=0.0, d0r=0.0, B=10.0, a=1.0, b=0.0, device=True):
    """The d = 9 model beyond the benchmark's parameters: one Rabi frequency om on every coupling
    (om01, when given, on |01>-|0r> only), the detuning delta on both atoms, d0r more on |0r> only, the
    blockade B, and the control entering as cos / sin(a x + b).  om01 != om or d0r != 0 make the two
    2-level sectors differ (no twins) and leave the swap symmetry of {11, 1r, r1, rr} alone.
    device=False: the same matrices as a closure over rydberg_hamiltonian_full."""
    from robustgrape_amd.operators import FN_COS, FN_SIN, VAR_X, OperatorBasisHamiltonian, Term
    o01 = om if om01 is None else om01
    if device:
        Hc = np.zeros((9, 9), np.complex128)
        Hs = np.zeros((9, 9), np.complex128)
        for r, c in ((1, 4), (2, 5), (3, 6), (3, 7), (6, 8), (7, 8)):  # RydbergTools.jl:118-130
            s = 0.5 * (o01 if (r, c) == (1, 4) else om)
            Hc[r, c] = Hc[c, r] = s
            Hs[r, c], Hs[c, r] = -1j * s, 1j * s   # e^{-i phi} above the diagonal
        terms = [Term(op=Hc, var=VAR_X, index=0, func=FN_COS, a=a, b=b),
                 Term(op=Hs, var=VAR_X, index=0, func=FN_SIN, a=a, b=b)]
        Hd = np.diag([0, 0, 0, 0, delta + d0r, delta, delta, delta, 2 * delta + B]).astype(np.complex128)
        if np.any(Hd != 0):
            terms.append(Term(op=Hd))
        H0 = OperatorBasisHamiltonian(terms)
        target = R.cz_full_target()
    else:
        def H0(t, p, xa):
            phi = a * p[0] + b
            H = R.rydberg_hamiltonian_full(phi, om, om, delta, delta, B)
            H[1, 4] = np.exp(-1j * phi) * o01 / 2
            H[4, 1] = np.exp(1j * phi) * o01 / 2
            H[4, 4] += d0r
            return H
        target = lambda xa: R.cz_with_1q_phase_full(xa[0])  # noqa: E731
    up = UnitaryRobustGRAPEProblem(t0=t0, ntimes=ntimes, ndim=9, H0=H0, nb_additional_param=1)
    return FidelityRobustGRAPEProblem(up, W_FULL9, target)


def relabel(fp, perm):
    """The same physics with basis state i renamed perm[i]: every H0, error and target operator becomes
    Pi op Pi^T and the projector Pi W Pi^T (Pi e_i = e_perm[i]); F and F_dx do not change.  The level
    order inside the sectors does: the charges' order and the weighted level's in-sector index.
    Operator-basis problems stay operator-basis; closures are wrapped."""
    from robustgrape_amd.operators import (OperatorBasisError, OperatorBasisHamiltonian, OperatorBasisTarget, Term)
    up = fp.unitary_problem
    perm = np.asarray(perm, int)
    assert sorted(perm.tolist()) == list(range(up.ndim))
    Pi = np.zeros((up.ndim, up.ndim))
    Pi[perm, np.arange(up.ndim)] = 1.0
    rot = lambda M: Pi @ np.asarray(M, np.complex128) @ Pi.T  # noqa: E731
    moved = lambda terms: [Term(op=rot(t.op), var=t.var, index=t.index, func=t.func, a=t.a, b=t.b,  # noqa: E731
                                scale=t.scale) for t in terms]
    if hasattr(up.H0, "terms"):
        H0 = OperatorBasisHamiltonian(moved(up.H0.terms))
        errs = [ErrorSource(OperatorBasisError(moved(es.Herror.terms))) for es in up.error_sources]
        target = OperatorBasisTarget(moved(fp.target_unitary.terms))
    else:
        h, tgt = up.H0, fp.target_unitary
        H0 = lambda t, p, xa: rot(h(t, p, xa))  # noqa: E731
        errs = [ErrorSource(lambda t, p, xa, e, f=es.Herror: rot(f(t, p, xa, e))) for es in up.error_sources]
        target = lambda xa: rot(tgt(xa))  # noqa: E731
    W = (Pi @ np.asarray(fp.projector, np.float64) @ Pi.T)
    return fp.replace(unitary_problem=up.replace(H0=H0, error_sources=errs), projector=W, target_unitary=target)


def _swap(*pairs):
    p = list(range(9))
    for i, j in pairs:
        p[i], p[j] = p[j], p[i]
    return p


# The phase-covariant walks' test family (tests/test_gauge_family_cpu.py, tests/test_gpu_gauge_family.py):
# name -> (full9_family arguments, relabelling or None, expected (twin class B, ladder charges in both
# classes) or None where the plan's report is taken as it comes).  Levels: |00>,|01>,|10>,|11>,|0r>,|r0>,
# |1r>,|r1>,|rr> = 0..8.
_DETUNED = dict(delta=0.7)
_SCALED = dict(a=-2.5, b=0.7)
_MIXED = dict(a=0.5, b=-1.1, delta=0.3, om=0.6, B=0.0, t0=T0_TEST)
_UNEQUAL = dict(om01=0.8, d0r=0.4)
GAUGE_FAMILY = {
    "detuned": (_DETUNED, None, (True, True)),
    "scaled": (_SCALED, None, (True, True)),
    "mixed": (_MIXED, None, (True, True)),
    "stiff": (dict(B=500.0, t0=3.0), None, (True, True)),   # |dt H|_1 ~ 16 at N_t = 96: squarings in E~
    "unequal": (_UNEQUAL, None, (False, True)),
    "swap-A": (_DETUNED, _swap((3, 8)), (True, False)),           # class A charges 2,1,0; c_A = 2
    "swap-B2": (_SCALED, _swap((1, 4), (2, 5)), (True, False)),   # class B charges 1,0 twice; c_B = 1,1
    "swap-B1": (_UNEQUAL, _swap((1, 4)), (False, False)),         # class B charges (1,0),(0,1); c_B = 1,0
    "reversed": (_MIXED, [8 - i for i in range(9)], None),
}


def gauge_family_problem(case, ntimes, device=True):
    """(the case's problem, the unrelabelled problem it was built from)."""
    kw, perm, _ = GAUGE_FAMILY[case]
    base = full9_family(ntimes, device=device, **kw)
    return (base if perm is None else relabel(base, perm)), base


def evered_pulse(ntimes=1000):
    """runtests.jl:127-138: the Evered et al. time-optimal CZ pulse."""
    t0 = 2 * math.pi * 1.22
    A, w0, p0, d0 = 0.7701624, 0.97525275, -0.97449603, -0.04319765
    theta = 2.0802725844516097
    ts = np.linspace(0, t0, ntimes)
    phis = A * np.cos(w0 * ts - p0) + d0 * ts
    return np.concatenate([phis, [theta]])


def max_step_norm(fp, X, nparam=1):
    """max over rows of X and steps k of |dt H0(k, x_k, x_add)|_1: the exponentials' regime.
    Up to 0.25 every implementation here and the reference evaluate exp without squaring (Taylor
    12 / Pade 5); above it the engines differ in algorithm (the chunk walks: Taylor 30 of A / 2^s
    at |A / 2^s|_1 <= 3.2; the row groups and Julia: Pade 7 / 9 / 13, squaring from 5.4)."""
    up = fp.unitary_problem
    dt = up.t0 / up.ntimes
    X = np.atleast_2d(np.asarray(X, np.float64))
    na = up.nb_additional_param
    best = 0.0
    for x in X:
        xm = x[:len(x) - na].reshape(up.ntimes, nparam)
        xa = x[len(x) - na:]
        for k in range(up.ntimes):
            H = np.asarray(up.H0(k + 1, xm[k], xa))
            best = max(best, dt * np.abs(H).sum(axis=0).max())
    return best


def short_steps(fp, X, nparam=1):
    """True when every step of every row is in the no-squaring range (the T2s tier applies)."""
    return max_step_norm(fp, X, nparam) <= 0.25


# Julia's exp! squares from |A|_1 > 5.4 (Pade 13's theta): up to there no tolerance scaling
JULIA_THETA13 = 5.4


def fd_tier(fp, X, nparam=1):
    """(relative, absolute) tolerance of eps-FD quantities (F_dx) for these rows: the short-step
    T2s tier (1e-7 max|ref| + 1e-9) when no step needs more than Taylor 12 / Pade 5, else the T2
    tier (1e-6 max|ref| + 1e-7), scaled by max(1, max_k |dt H_k|_1 / 5.4) beyond Julia's Pade-13
    threshold: there the reference squares s = ceil(log2(|A|_1 / 5.4)) times and its own rounding
    -- the u / eps noise of (E' - E) / eps -- grows like 2^s in any implementation (measured:
    profiles/r04/highnorm_study.txt, Julia's D1 error against an extended-precision evaluation is
    1.6e-7 at |A|_1 = 3, 2e-6 at 30, 5e-6 at 80; the walks' Taylor 30 matches it at every norm)."""
    n = max_step_norm(fp, X, nparam)
    if n <= 0.25:
        return 1e-7, 1e-9
    f = max(1.0, n / JULIA_THETA13)
    return 1e-6 * f, 1e-7 * f


def fd_factor(fp, X, nparam=1):
    """The step-norm factor of the FD tiers (fd_tier's rule): 1 up to Julia's Pade-13
    threshold |dt H_k|_1 = 5.4, max_k |dt H_k|_1 / 5.4 beyond it (the reference squares there and its
    u / eps noise grows like 2^s).  Used for the tiers fd_tier does not return (T2 of uncontracted
    tensors and sensitivities, T3 of the mixed stencils)."""
    return max(1.0, max_step_norm(fp, X, nparam) / JULIA_THETA13)


def tensor_factor(fp, X, nparam=1):
    """The step-norm factor for UNCONTRACTED finite-difference tensors (U_dx, U_derr, U_derr_dx of
    calculate_unitary_and_derivatives): max(1, max_k |dt H_k|_1) beyond the no-squaring range, like
    T0.  An entry of (E' - E) / eps carries the exponential's own rounding, ~u |A|_1 per entry, over
    eps; the traces of the fidelity path average it (fd_factor's 5.4 rule), a single tensor entry
    does not."""
    n = max_step_norm(fp, X, nparam)
    return 1.0 if n <= 0.25 else max(1.0, n)


def random_x(ntimes, seed, nparam=1, small=False):
    """x_main = 2pi*U (runtests.jl:335) or 2pi*0.001*U (examples/time_optimal_cz.jl:32); theta = 2pi*U."""
    rng = np.random.default_rng(seed)
    scale = 2 * math.pi * (0.001 if small else 1.0)
    return np.concatenate([scale * rng.uniform(size=ntimes * nparam), [2 * math.pi * rng.uniform()]])


def xadd_err_problem(d, ntimes, nerr=2, device=True):
    """Error sources together with an H0 that reads x_add (UnitaryCalculations.jl:57-64, 87-95,
    140-151): the d=5 symmetric (runtests.jl:57-75) or d=9 full Rydberg
    problem with a second additional parameter x_add[1], a global detuning on a diagonal
    occupation operator, and an error source whose strength is modulated by cos(x_add[1]).
    x_add[0] stays the target's single-qubit phase.  device=False: the same physics as plain
    closures (the reference's idiom), which the table path and the oracle evaluate."""
    from robustgrape_amd.operators import (FN_COS, FN_LINEAR, VAR_XADD, OperatorBasisError,
                                           OperatorBasisHamiltonian, Term)
    base = sym_problem(ntimes, errors=("amp", "freq")[:nerr]) if d == 5 else full9_problem(ntimes, nerr=nerr)
    up = base.unitary_problem
    Nr = np.diag(np.linspace(0.0, 1.0, d)).astype(np.complex128)
    H0 = OperatorBasisHamiltonian(list(up.H0.terms) + [Term(Nr, var=VAR_XADD, index=1, func=FN_LINEAR, scale=0.5)])
    errs = []
    for e, es in enumerate(up.error_sources):
        terms = list(es.Herror.terms)
        if e == 0:
            terms.append(Term(Nr, var=VAR_XADD, index=1, func=FN_COS, scale=0.3))
        errs.append(ErrorSource(OperatorBasisError(terms)))
    target = base.target_unitary
    if not device:
        Hdev, tdev, edev = H0, target, errs
        H0 = lambda t, x, xa: Hdev(t, x, xa)  # noqa: E731
        target = lambda xa: tdev(xa)  # noqa: E731
        errs = [ErrorSource(lambda t, x, xa, e, es=es: es.Herror(t, x, xa, e)) for es in edev]
    up2 = UnitaryRobustGRAPEProblem(t0=up.t0, ntimes=ntimes, ndim=d, H0=H0, nb_additional_param=2,
                                    error_sources=errs)
    return FidelityRobustGRAPEProblem(up2, base.projector, target)


def xadd_x(ntimes, seed):
    """Control vector of xadd_err_problem: x_main = 2pi U, theta = 2pi U, detuning U[-0.5, 0.5)."""
    rng = np.random.default_rng(seed)
    return np.concatenate([2 * math.pi * rng.uniform(size=ntimes), [2 * math.pi * rng.uniform(), rng.uniform(-0.5, 0.5)]])


def with_decay(fp, gamma=0.4, levels=(4,), device=True):
    """fp with a non-Hermitian H0: -i gamma/2 on each of `levels` (a Rydberg-decay term, the
    reference accepts any H0: UnitaryCalculations.jl:45-47 exponentiates and LU-inverts it).
    Device form: one more OperatorBasisHamiltonian term; oracle form: a wrapped closure."""
    up = fp.unitary_problem
    G = np.zeros((up.ndim, up.ndim), np.complex128)
    for l in levels:
        G[l, l] = 1.0
    if device:
        from robustgrape_amd.operators import OperatorBasisHamiltonian, Term
        H0 = OperatorBasisHamiltonian(list(up.H0.terms) + [Term(G, scale=-0.5j * gamma)])
    else:
        h = up.H0
        H0 = lambda t, p, xa: np.asarray(h(t, p, xa), np.complex128) - 0.5j * gamma * G  # noqa: E731
    return fp.replace(unitary_problem=up.replace(H0=H0))


def as_closures(fp):
    """The same problem with plain-function H0 / Herror / target (the reference's idiom,
    Types.jl:13,25,55): the engine then takes the host-table (closure) path."""
    from robustgrape_amd.types import ErrorSource as ES
    up = fp.unitary_problem
    h, tgt = up.H0, fp.target_unitary
    wrap_err = lambda f: (lambda t, p, xa, e: f(t, p, xa, e))  # noqa: E731
    errs = [ES(wrap_err(es.Herror)) for es in up.error_sources]
    up2 = up.replace(H0=lambda t, p, xa: h(t, p, xa), error_sources=errs)
    return fp.replace(unitary_problem=up2, target_unitary=lambda xa: tgt(xa))


def tiled_rich_problem(d, x0s, weights, small, nparam=3, x_add=(0.3, -0.7)):
    """(problem, x) of the tiled engine's wider test family (tests/test_gpu_tiled_edges.py): what
    synthetic.dense_problem never has.  Six Hermitian Ginibre operators H_i = synthetic._hermitian(d, 400 + i),
    |H_i|_1 = 1, dt = 0.5, one step per entry of x0s:

        H(k, x) = small H_0 + x[0] H_1 + small (cos(1.3 x[1] + 0.2) H_2 + sin(1.3 x[1] + 0.2) H_3)
                  + small (0.5 k - 1) H_4 + small x[2] H_5           (k = 1 .. N_t, the step index)

    so every term kind the engine serves (ONE, LINEAR, COS, SIN; on 1, x and the step index) with np = 3; nparam = 1
    drops the terms on x[1] and x[2].  x ~ U[-1, 1) (seed 5) with x[:, 0] = x0s: |A_k|_1 is 0.5 |x0s[k]| plus a
    rest of order small.  Target with na = 2: Q (I - e_0 e_0^T - e_l e_l^T) + cis(x_add[0]) Q e_0 e_0^T +
    cis(2 x_add[1] + 0.1) Q e_l e_l^T, l = d - 1 the last level.  Projector: diagonal, {level: weight}."""
    from robustgrape_amd import synthetic as S
    from robustgrape_amd.operators import (FN_CIS, FN_COS, FN_LINEAR, FN_SIN, VAR_TSTEP, VAR_X, VAR_XADD,
                                           OperatorBasisHamiltonian, OperatorBasisTarget, Term)
    assert nparam in (1, 3)
    H = [S._hermitian(d, 400 + i) for i in range(6)]
    terms = [Term(small * H[0]), Term(H[1], var=VAR_X, index=0, func=FN_LINEAR)]
    if nparam == 3:
        terms += [Term(small * H[2], var=VAR_X, index=1, func=FN_COS, a=1.3, b=0.2),
                  Term(small * H[3], var=VAR_X, index=1, func=FN_SIN, a=1.3, b=0.2)]
    terms.append(Term(small * H[4], var=VAR_TSTEP, func=FN_LINEAR, a=0.5, b=-1.0))
    if nparam == 3:
        terms.append(Term(small * H[5], var=VAR_X, index=2, func=FN_LINEAR))
    ntimes = len(x0s)
    up = UnitaryRobustGRAPEProblem(t0=0.5 * ntimes, ntimes=ntimes, ndim=d, H0=OperatorBasisHamiltonian(terms),
                                   nb_additional_param=2)
    Q = S.dense_target(d)
    P0, Pl = np.zeros((d, d)), np.zeros((d, d))
    P0[0, 0] = Pl[d - 1, d - 1] = 1.0
    target = OperatorBasisTarget([Term(Q @ (np.eye(d) - P0 - Pl)),
                                  Term(Q @ P0, var=VAR_XADD, index=0, func=FN_CIS),
                                  Term(Q @ Pl, var=VAR_XADD, index=1, func=FN_CIS, a=2.0, b=0.1)])
    W = np.zeros(d)
    for level, w in weights.items():
        W[level] = w
    x = np.random.default_rng(5).uniform(-1.0, 1.0, size=(ntimes, 3))[:, :nparam].copy()
    x[:, 0] = x0s
    return FidelityRobustGRAPEProblem(up, np.diag(W), target), np.concatenate([x.ravel(), np.asarray(x_add, float)])


def tiled_sixteen_weights(d):
    """Sixteen scattered projector weights, unequal, in both row tiles (0-63 and the remainder), on both sides of
    every 16-row fragment edge below d, on the last level and on d - 17 and d - 2."""
    mid = 50 if d < 100 else 65
    return {0: 1.0, 3: 0.5, 15: 2.0, 16: 1.5, 17: 0.25, 31: 1.0, 40: 1.0, 47: 0.75, 48: 1.25, mid: 1.0, 62: 1.0,
            63: 0.5, 64: 1.5, d - 17: 2.0, d - 2: 0.25, d - 1: 1.0}


TILED_X0S = (0.3, -0.8, 1.2, 0.5, -1.0)   # five steps of Taylor 12 / 16 / 16 / 12 / 16 with small = 0.1
SEAM_D, SEAM_NT, SEAM_EVALS = 65, 43, 24   # 1 032 steps in one pass: slabs of 1 024 + 8


def seam_batch():
    """(problem, X) of the slab-seam test: 24 evaluations of dense_problem(65, 43, rank 16)."""
    from robustgrape_amd import synthetic as S
    X = np.stack([S.dense_x(SEAM_NT, seed=700 + s) for s in range(SEAM_EVALS)])
    return S.dense_problem(SEAM_D, SEAM_NT, rank=16), X


def tiled_edge_case(name):
    """(problem, x, nparam) of a case of the fixture tests/golden/tiled_edges.npz (make_golden_tiled_edges.py)."""
    if name == "proj113":   # the sixteen weights at P = 128 != d, remainder tile of 49 live rows
        fp, x = tiled_rich_problem(113, TILED_X0S, tiled_sixteen_weights(113), 0.1)
        return fp, x, 3
    if name == "seam23":    # the last evaluation of the seam batch: the slab seam falls at its step 35
        fp, X = seam_batch()
        return fp, X[SEAM_EVALS - 1], 2
    raise KeyError(name)


def step_norms(fp, x, nparam):
    """|dt H(k, x_k, x_add)|_1 of every step of one control vector (the norms k_tctl computes)."""
    up = fp.unitary_problem
    na = up.nb_additional_param
    xm, xa = x[:len(x) - na].reshape(up.ntimes, nparam), x[len(x) - na:]
    dt = up.t0 / up.ntimes
    return np.array([dt * np.abs(np.asarray(up.H0(k + 1, xm[k], xa))).sum(axis=0).max() for k in range(up.ntimes)])


def weighted_indices(fp):
    """{sector size: the weighted level's in-sector index c, per sector of that size, by first level}:
    the sectors are the blocks of grape_symmetry_basis (host code), their levels in ascending order of the
    rotated basis, the weight the diagonal of V^dag W V; None for a sector that has not exactly one
    weighted level."""
    import ctypes
    from robustgrape_amd import _capi
    from robustgrape_amd.operators import DescriptorBuffers
    d = fp.unitary_problem.ndim
    buf = DescriptorBuffers(fp, nparam=1, max_batch=1)
    V = np.zeros(2 * d * d)
    blk = (ctypes.c_int * d)()
    rc = _capi.lib().grape_symmetry_basis(ctypes.byref(buf.desc), _capi.dptr(V), blk)
    assert rc in (0, 1), rc
    Vc = (V[0::2] + 1j * V[1::2]).reshape(d, d, order="F")
    w = np.real(np.diag(Vc.conj().T @ np.asarray(fp.projector, np.float64) @ Vc))
    blk = np.array(list(blk))
    out = {}
    for k in sorted(set(blk.tolist()), key=lambda k: int(np.flatnonzero(blk == k)[0])):
        levels = np.flatnonzero(blk == k)
        hit = [i for i, g in enumerate(levels) if abs(w[g]) > 1e-12]
        out.setdefault(len(levels), []).append(hit[0] if len(hit) == 1 else None)
    return out
