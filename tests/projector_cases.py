"""General projectors beyond the degenerate ones: generators, the case table of
tests/test_gpu_projector_paths.py and a numpy model of the heads' formulas (no GPU needed here;
tests/test_projector_cases_cpu.py checks all of it on the host).

tests/test_gpu_projector.py's dense_projector has every entry nonzero, so P (the pattern of ones) is
the all-ones matrix: B = P = B^dagger has rank one and A = P0 P has constant rows.  The heads of
grape_projector.hip and grape_unitary.hip (k_u_fid_head) hold B next to B^dagger and A next to
A^dagger in about a dozen products; with that projector a transposed operand changes nothing.
pattern_projector draws a masked, non-symmetric real matrix for which it does."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from robustgrape_amd import synthetic as S
from robustgrape_amd.operators import OPT_GENERAL_H0, OPT_NO_SECTORS
from tests import problems as P

T1 = 1e-12
T2, T2_FLOOR, T2_ABS = 1e-6, 1e-9, 1e-7   # F_dx against exact: T2 max|exact| + T2_FLOOR; F_d2err: T2 max|ref| + T2_ABS
T3, T3_ABS = 1e-5, 1e-7                   # F_d2err_dx


# ---------------------------------------------------------------------------------------------
# projectors
# ---------------------------------------------------------------------------------------------
def pattern_properties(P0):
    """What pattern_projector guarantees, measured: the mask's and A's asymmetry, rank(A), tr P0."""
    P0 = np.asarray(P0, np.float64)
    mask = P0 != 0
    A = P0 @ mask.astype(np.float64)
    return {"mask_asymmetric": bool(np.any(mask != mask.T)),
            "rank_A": int(np.linalg.matrix_rank(A)),
            "A_asymmetry": float(np.max(np.abs(A - A.T)) / max(np.max(np.abs(A)), 1e-300)),
            "trace": float(np.trace(P0))}


def _pattern_ok(P0):
    p = pattern_properties(P0)
    return p["mask_asymmetric"] and p["rank_A"] >= 2 and p["A_asymmetry"] > 1e-2 and p["trace"] >= 1.0


def _pattern_draw(d, seed, fill):
    rng = np.random.default_rng(seed)
    mask = rng.uniform(size=(d, d)) < fill
    P0 = np.where(mask, rng.uniform(-0.5, 0.5, size=(d, d)), 0.0)
    diag = rng.uniform(0.5, 1.0, size=d)
    diag[rng.uniform(size=d) < 0.25] = 0.0
    P0[np.diag_indices(d)] = diag
    return P0


def pattern_projector(d, seed, fill=0.4):
    """A real d x d projector matrix (the reference takes any, Types.jl:54): off-diagonal entries
    U[-0.5, 0.5] under a random 0/1 mask of density `fill`, diagonal U[0.5, 1] with about a quarter of
    its entries exactly 0.  Guaranteed (the next seed is drawn until they hold): the mask is not
    symmetric, so B = P differs from B^dagger; A = P0 P has rank >= 2 and is not symmetric; tr P0 >= 1, so
    DD = D (D + 1) >= 2 does not amplify F."""
    for s in range(seed, seed + 1000):
        P0 = _pattern_draw(d, s, fill)
        if _pattern_ok(P0):
            return P0
    raise ValueError(f"no pattern projector for d={d} from seed {seed}")


def weighted_diagonal(d, seed):
    """A diagonal projector with weights in {0, 0.5, 1} (each present for d >= 3, tr >= 1): the diagonal
    specialisation (gen_proj = 0) with weights that are not 0 / 1."""
    for s in range(seed, seed + 1000):
        w = np.random.default_rng(s).choice([0.0, 0.5, 1.0], size=d)
        if w.sum() >= 1.0 and (d < 3 or len(set(w.tolist())) == 3):
            return np.diag(w)
    raise ValueError(f"no weighted diagonal for d={d} from seed {seed}")


# ---------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------
# builder: "dims"       tests.test_gpu_dims.random_problem (fully coupled, np = 2, na = 1 target phase)
#          "xadd"       tests.problems.xadd_err_problem (d = 5 / 9 Rydberg, np = 1, na = 2, ne = 2, H0 reads x_add)
#          "dense"      synthetic.dense_problem / dense_error_problem (np = 2, na = 1 with phase)
#          "dense_xadd" tests.test_gpu_dense._xadd_h0_problem (np = 2, na = 2, H0 reads x_add)
# decay: tests.problems.with_decay (gamma = 0.4 on three levels); options: the plan's GRAPE_OPT_* flags;
# proj: "pattern" or "weighted"
Case = namedtuple("Case", "name group builder d nt nerr pseed xseed phase decay options proj")


def _case(name, group, builder, d, nt, nerr, pseed, xseed, phase=False, decay=False, options=0, proj="pattern"):
    return Case(name, group, builder, d, nt, nerr, pseed, xseed, phase, decay, options, proj)


# x seeds: where the oracle's own u / eps noise against the longdouble evaluation exceeded half of the tier
# (test_projector_cases_cpu.py: test_oracle_noise_stays_under_half_the_tier) the seed was moved on by tens
# to the first draw that keeps it (the noise is 2e-7 .. 8e-7 of max|F_dx| from draw to draw, the half tier 5e-7);
# d = 8 with error sources kept it at seed 50 with 0.73 of the half tier and moved to a draw with 0.10
_DIMS_XSEED = {(2, 0): 82, (2, 2): 74, (3, 0): 53, (3, 2): 45, (7, 0): 47, (7, 2): 49, (8, 0): 48, (8, 2): 68,
               (12, 0): 52, (12, 2): 64}
_TABLE = []
for _d in (2, 3, 7, 8, 12):   # a. the small engine's whole-matrix path (k_proj_fid / k_proj_err, row-major sources)
    for _ne, _nt in ((0, 9), (2, 5)):
        _TABLE.append(_case(f"dims{_d}_ne{_ne}", "a", "dims", _d, _nt, _ne, 100 + _d, _DIMS_XSEED[_d, _ne]))
_TABLE += [
    _case("xadd5_whole", "a", "xadd", 5, 9, 2, 105, 69, options=OPT_NO_SECTORS),
    _case("xadd9_whole", "a", "xadd", 9, 7, 2, 109, 86, options=OPT_NO_SECTORS),
    # b. the dense engine (register-file images: load_mat's image branch, store_image, k_dmc / k_dmce)
    _case("dense13", "b", "dense", 13, 3, 0, 213, 503),
    _case("dense17_ne2", "b", "dense", 17, 3, 2, 217, 503, phase=True),
    _case("dense33", "b", "dense", 33, 4, 0, 233, 504),
    _case("dense48_ne1", "b", "dense", 48, 3, 1, 248, 593),
    _case("dense64_ne2", "b", "dense", 64, 3, 2, 264, 723, phase=True),
    _case("dense16_xadd", "b", "dense_xadd", 16, 5, 0, 216, 505),
    # c. k_u_fid_head on a Hermitian problem (GRAPE_OPT_GENERAL_H0 forced): LDS tiles, global-scratch tiles
    _case("general9_xadd", "c", "xadd", 9, 7, 2, 109, 108, options=OPT_GENERAL_H0),
    _case("general16_ne2", "c", "dense", 16, 5, 2, 316, 405, phase=True, options=OPT_GENERAL_H0),
    # d. k_u_fid_head with a decay term
    _case("decay9_xadd", "d", "xadd", 9, 7, 2, 409, 67, decay=True, options=OPT_GENERAL_H0),
    _case("decay16_ne2", "d", "dense", 16, 5, 2, 416, 805, phase=True, decay=True, options=OPT_GENERAL_H0),
    _case("decay40_ne2", "d", "dense", 40, 4, 2, 440, 804, phase=True, decay=True, options=OPT_GENERAL_H0),
    _case("decay9_weighted", "d", "xadd", 9, 7, 2, 509, 67, decay=True, options=OPT_GENERAL_H0, proj="weighted"),
]
CASES = {c.name: c for c in _TABLE}
assert len(CASES) == len(_TABLE)
GAMMA = 0.4
# The d = 9 problem with H0 reading x_add takes long steps (|dt H|_1 about 12: squarings in every exponential), and
# the x_add[1] entry of F_dx, a sum over the steps of (E(x_add + eps) - E) / eps, carries up to 1.5e-7 of ABSOLUTE
# u / eps noise in any double implementation (the oracle and, through head_model, the C++ port, measured against
# exact over 20 draws), whatever the gradient's size.  The tier against exact is relative, 1e-6 max|F_dx|: its
# draws (the case's own and the closure batch's rows) are taken where max|F_dx| >= XADD9_MIN_SCALE, so that the
# tier is above that noise, and where the oracle keeps the half tier like every other case.
XADD9_MIN_SCALE = 0.19
BATCH_XSEEDS = {"xadd9_whole": (86, 108, 247)}


def nparam(c):
    return 1 if c.builder == "xadd" else 2


def decay_levels(c):
    return (1, c.d // 2, c.d - 1)


def projector(c):
    return pattern_projector(c.d, c.pseed) if c.proj == "pattern" else weighted_diagonal(c.d, c.pseed)


def base_problem(c, device=True, decay=None):
    """The case's problem before the projector is set (decay: the case's own, or forced off with False)."""
    if c.builder == "dims":
        from tests.test_gpu_dims import random_problem
        fp = random_problem(c.d, c.nt, c.nerr, device)
    elif c.builder == "xadd":
        fp = P.xadd_err_problem(c.d, c.nt, nerr=c.nerr, device=device)
    elif c.builder == "dense":
        rank = min(16, c.d - 3)
        if c.nerr == 0 and not c.phase:
            fp = S.dense_problem(c.d, c.nt, rank=rank)
        else:
            fp = S.dense_error_problem(c.d, c.nt, rank=rank, nerr=c.nerr, phase=c.phase)
    elif c.builder == "dense_xadd":
        from tests.test_gpu_dense import _xadd_h0_problem
        fp = _xadd_h0_problem(c.d, c.nt)
    else:
        raise KeyError(c.builder)
    if c.decay if decay is None else decay:
        fp = P.with_decay(fp, GAMMA, decay_levels(c), device)
    return fp


def problem(c, device=True, decay=None):
    """device=False: H0 / Herror / target as plain closures where the builder has that form (what the
    oracle is given); the synthetic dense family has the operator-basis form only (the oracle calls it)."""
    return base_problem(c, device, decay).replace(projector=projector(c))


def control(c, seed=None):
    """The case's control vector (seed: another draw of the same family, for the batches)."""
    seed = c.xseed if seed is None else seed
    if c.builder == "dims":
        rng = np.random.default_rng(seed)
        return np.concatenate([rng.uniform(-1, 1, size=2 * c.nt), [rng.uniform(0, 2 * np.pi)]])
    if c.builder == "xadd":
        return P.xadd_x(c.nt, seed)
    x = S.dense_x(c.nt, seed=seed)
    if c.builder == "dense_xadd":
        return np.concatenate([x, [0.7 + 0.01 * (seed - c.xseed), -0.3]])
    return np.concatenate([x, [0.7 + 0.01 * (seed - c.xseed)]]) if c.phase else x


def batch_controls(c, n):
    """n control vectors of the case, the first its own: the seeds of BATCH_XSEEDS, else xseed, xseed + 1, ..."""
    seeds = BATCH_XSEEDS.get(c.name, tuple(c.xseed + s for s in range(n)))[:n]
    assert len(seeds) == n and seeds[0] == c.xseed
    return np.stack([control(c, s) for s in seeds])


def exact_scope(c):
    """What oracle/grape_exact.py evaluates for the case: "all" (Hermitian generators that do not read x_add:
    F, F_dx and the sensitivities), "gradient" (H0 reads x_add: F and F_dx, fidelity_and_gradient_xadd) or
    None (a decay term: the evaluator takes C_k^-1 = C_k^dagger)."""
    if c.decay:
        return None
    return "all" if c.builder in ("dims", "dense") else "gradient"


def exact_in_scope(c):
    return exact_scope(c) is not None


def exact_outputs(c, x):
    """(F, F_dx, F_d2err or None, F_d2err_dx or None) in longdouble, or None outside the evaluator's scope."""
    from oracle import grape_exact as E
    scope = exact_scope(c)
    if scope is None:
        return None
    if scope == "all" and c.nerr:
        return _frozen(E.fidelity_and_derivatives(problem(c), x, nparam(c)))
    fn = E.fidelity_and_gradient if scope == "all" else E.fidelity_and_gradient_xadd
    return _frozen(fn(problem(c), x, nparam(c)) + (None, None))


def _frozen(out):
    res = []
    for a in out:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        res.append(a)
    return tuple(res)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(x, oracle outputs, exact outputs or None) of a case, evaluated once and read-only.  exact: (F, F_dx,
    F_d2err or None, F_d2err_dx or None) in longdouble."""
    from oracle import grape_oracle as O
    c = CASES[name]
    x = control(c)
    ref = O.calculate_fidelity_and_derivatives(problem(c, device=False), x)
    exact = exact_outputs(c, x)
    x.setflags(write=False)
    return x, _frozen(ref), exact


@functools.lru_cache(maxsize=None)
def fidelity_without_decay(name):
    """The oracle's F of a decay case with the decay term left out."""
    from oracle import grape_oracle as O
    c = CASES[name]
    return O.calculate_fidelity_and_derivatives(problem(c, device=False, decay=False), control(c))[0]


def oracle_distances(name, ref=None, exact=None):
    """The oracle's distance from the exact evaluation per quantity, with the half-tier the condition on
    the inputs allows it: {quantity: (distance, half tier)}.  Half of the tier the GPU test applies, so
    that a correct device result, whose own noise is of the oracle's kind, passes against exact.
    ref, exact: another evaluation of the case (a batch row) instead of the table's."""
    if ref is None:
        _, ref, exact = reference(name)
    c = CASES[name]
    out = {"F_dx": (float(np.max(np.abs(ref[1] - exact[1]))),
                    0.5 * (T2 * float(np.max(np.abs(exact[1]))) + T2_FLOOR))}
    if c.nerr and exact[2] is not None:
        out["F_d2err"] = (float(np.max(np.abs(ref[2] - exact[2]))),
                          0.5 * (T2 * float(np.max(np.abs(exact[2]))) + T2_ABS))
        out["F_d2err_dx"] = (float(np.max(np.abs(ref[3] - exact[3]))),
                             0.5 * (T3 * float(np.max(np.abs(exact[3]))) + T3_ABS))
    return out


# ---------------------------------------------------------------------------------------------
# numpy model of the heads' formulas
# ---------------------------------------------------------------------------------------------
def head_model(fp, x, swap_b=False):
    """F, F_dx, F_d2err, F_d2err_dx as the header comments of grape_projector.hip and of k_u_fid_head
    (grape_unitary.hip) state them, over the oracle's calculate_unitary_and_derivatives tensors:

        A = P0 P, B = P, K = U0^dag U, tau = tr(A K), DD = D (D + 1)
        F   = [Re tr(A K B K^dag) + |tau|^2] / DD
        G   = (B K^dag A + B^dag K^dag A^dag + 2 conj(tau) A) U0^dag / DD,   M = G U,   F_dx = Re tr(U_dx G)
        Ke = U0^dag Ue, te = tr(A Ke)
        F_d2err = 2 [Re tr(A Ke B Ke^dag) - (1 + D) Re tr(A Ue^dag Ue) + |te|^2] / DD
        G_e = 2 [(B Ke^dag A + B^dag Ke^dag A^dag + 2 conj(te) A) U0^dag - (1 + D)(A + A^dag) Ue^dag] / DD
        F_d2err_dx = Re tr(U_derr_dx G_e)
    and on the x_add entries the target parts with Kd = U0d^dag U, Kde = U0d^dag Ue.
    swap_b: B^dagger replaced by B (the transposed operand the degenerate projectors cannot see).
    Returns (F, F_dx_tot, F_d2err, F_d2err_dx_tot, G, M)."""
    from oracle import grape_oracle as O
    up = fp.unitary_problem
    U, U_dx, U_dx_add, U_derr, U_derr_dx, U_derr_dx_add = O.calculate_unitary_and_derivatives(up, x)
    x_main, x_add, npar = O._unpack(up, x)
    nt, na, ne = up.ntimes, up.nb_additional_param, len(up.error_sources)
    ct = lambda X: X.conj().T  # noqa: E731
    U0 = np.asarray(fp.target_unitary(x_add.copy()), np.complex128)
    U0d = []
    for q in range(na):
        xq = x_add.copy()
        xq[q] += up.eps
        U0d.append((1.0 / up.eps) * (np.asarray(fp.target_unitary(xq), np.complex128) - U0))
    P0 = np.asarray(fp.projector, np.float64)
    B = (P0 != 0).astype(np.complex128)
    A = P0.astype(np.complex128) @ B
    Bh = B if swap_b else ct(B)
    D = float(np.trace(P0))
    DD = D * (D + 1)
    retr = lambda X: float(np.real(np.trace(X)))  # noqa: E731

    K = ct(U0) @ U
    tau = np.trace(A @ K)
    F = (retr(A @ K @ B @ ct(K)) + abs(tau) ** 2) / DD
    G = (B @ ct(K) @ A + Bh @ ct(K) @ ct(A) + 2 * np.conj(tau) * A) @ ct(U0) / DD
    M = ((B @ ct(K) @ A + Bh @ ct(K) @ ct(A)) @ K + 2 * np.conj(tau) * A @ K) / DD
    F_dx = np.zeros(npar * nt + na)
    for k in range(nt):
        for p in range(npar):
            F_dx[k * npar + p] = retr(U_dx[:, :, p, k] @ G)
    for q in range(na):
        Kd = ct(U0d[q]) @ U
        tgt = (retr(A @ Kd @ B @ ct(K)) + retr(A @ K @ B @ ct(Kd)) + 2 * np.real(np.conj(tau) * np.trace(A @ Kd))) / DD
        F_dx[npar * nt + q] = retr(U_dx_add[:, :, q] @ G) + tgt
    F_d2err = np.zeros(ne)
    F_d2err_dx = np.zeros((npar * nt + na, ne))
    for e in range(ne):
        Ue = U_derr[:, :, e]
        Ke = ct(U0) @ Ue
        te = np.trace(A @ Ke)
        F_d2err[e] = 2 * (retr(A @ Ke @ B @ ct(Ke)) - (1 + D) * retr(A @ ct(Ue) @ Ue) + abs(te) ** 2) / DD
        Ge = 2 * ((B @ ct(Ke) @ A + Bh @ ct(Ke) @ ct(A) + 2 * np.conj(te) * A) @ ct(U0)
                  - (1 + D) * (A + ct(A)) @ ct(Ue)) / DD
        for k in range(nt):
            for p in range(npar):
                F_d2err_dx[k * npar + p, e] = retr(U_derr_dx[:, :, p, k, e] @ Ge)
        for q in range(na):
            Kde = ct(U0d[q]) @ Ue
            tgt = 2 * (retr(A @ Kde @ B @ ct(Ke)) + retr(A @ Ke @ B @ ct(Kde))
                       + 2 * np.real(np.conj(te) * np.trace(A @ Kde))) / DD
            F_d2err_dx[npar * nt + q, e] = retr(U_derr_dx_add[:, :, q, e] @ Ge) + tgt
    return F, F_dx, F_d2err, F_d2err_dx, G, M
