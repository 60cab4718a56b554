"""Cases at which the grid-stride loops of robustgrape_amd/csrc/grape_unitary.hip take a second item.

Above 12 levels (kMaxD) the kernels' d x d tiles live in global scratch and the launches are capped at
kResident workgroups that stride over the items (grid_for); k_u_fid_contract caps its grid at 4096 blocks of
four waves at every size (launch_fidelity).  Below those two counts every workgroup (wave) handles exactly one
item, whatever the loop does with the second.  The tables here name, per case, the kernels whose item count
exceeds its cap; tests/test_unitary_wrap_cases_cpu.py checks the counts (plain arithmetic, no GPU) and
tests/test_gpu_unitary_wrap.py runs the cases against the oracle.

Item counts of one evaluation (np controls per step, na additional parameters, ne error sources):
    k_u_vmats        N_t nslots,  nslots = np + na + ne + ne (np + na)
    k_u_assemble     N_t np (1 + ne)         (k_u_fid_contract: the same count, one wave per item)
    k_u_inverse      N_t                     (general H0 only)
    k_u_interaction, k_u_interaction_table   N_t ne
"""
from __future__ import annotations

import functools

import numpy as np

from robustgrape_amd import synthetic as S
from robustgrape_amd.operators import FN_LINEAR, VAR_X, OperatorBasisError, OperatorBasisHamiltonian, Term
from robustgrape_amd.types import ErrorSource
from tests import problems as P

MAX_LDS_DIM = 12                 # grape_unitary_api.hpp kMaxD: LDS tiles, one workgroup per item, up to here
RESIDENT = 256                   # grape_unitary_api.hpp kResident: the workgroups of a launch above kMaxD
FID_CONTRACT_ITEMS = 4096 * 4    # grape_unitary.hip launch_fidelity: min(.., 4096) blocks of BLOCK / 64 = 4 waves
NP = 2                           # the C5 family's controls per step


def item_counts(ntimes, nparam, na, ne):
    """(N_t nslots, N_t np (1 + ne), N_t, N_t ne): the items of k_u_vmats, of k_u_assemble and
    k_u_fid_contract, of k_u_inverse, and of k_u_interaction / k_u_interaction_table."""
    nslots = nparam + na + ne + ne * (nparam + na)
    return ntimes * nslots, ntimes * nparam * (1 + ne), ntimes, ntimes * ne


KERNEL_COUNT = {"k_u_vmats": 0, "k_u_assemble": 1, "k_u_fid_contract": 1, "k_u_inverse": 2, "k_u_interaction": 3,
                "k_u_interaction_table": 3}


def _rank(d):
    return min(16, d - 3)


def _dense(d, nt, nerr, phase, rank=None):
    rank = _rank(d) if rank is None else rank
    if nerr == 0 and not phase:
        return S.dense_problem(d, nt, rank=rank)
    return S.dense_error_problem(d, nt, rank=rank, nerr=nerr, phase=phase)


def dense_x(nt, phase, seed):
    x = S.dense_x(nt, seed=seed)
    return np.concatenate([x, [0.7]]) if phase else x


# ---- calculate_unitary_and_derivatives, Hermitian H0: (d, N_t, ne, phase) -> the kernels that wrap.
# (16, 48, 2, phase) also runs k_u_reduce over 5 outputs; (64, 6, 2, phase) wraps nothing: d = 64 (16 elements per
# thread and tile) with error sources and an additional parameter.
TENSOR_CASES = {
    (13, 140, 0, False): ("k_u_vmats", "k_u_assemble"),
    (16, 48, 2, True): ("k_u_vmats", "k_u_assemble"),
    (64, 130, 0, False): ("k_u_vmats", "k_u_assemble"),
    (64, 6, 2, True): (),
}


def tensor_case(d, nt, nerr, phase):
    """(unitary problem, x) of a TENSOR_CASES key."""
    return _dense(d, nt, nerr, phase).unitary_problem, dense_x(nt, phase, 1600 + nt)


# ---- analysis entry points and the general-H0 fidelity path: name -> (d, N_t, ne, phase, the kernels that wrap)
ANALYSIS_D, ANALYSIS_NT, ANALYSIS_PROJ_SEED = 20, 140, 1720
DECAY_D, DECAY_NT, DECAY_GAMMA, DECAY_LEVELS = 13, 260, 0.02, (1, 6, 12)
GENERAL_D, GENERAL_NT, GENERAL_GAMMA = 13, 90, 0.05
PLAN_CASES = {
    "analysis": (ANALYSIS_D, ANALYSIS_NT, 2, False, ("k_u_interaction", "k_u_interaction_table")),
    "decay": (DECAY_D, DECAY_NT, 1, False, ("k_u_inverse", "k_u_interaction", "k_u_vmats", "k_u_assemble")),
    "general": (GENERAL_D, GENERAL_NT, 2, True, ("k_u_vmats", "k_u_assemble")),
}


def dense_projector(d, rank, seed):
    """Orthogonal projector onto a random real subspace, every entry nonzero (tests/test_gpu_projector.py)."""
    Qm, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, rank)))
    return Qm @ Qm.T


@functools.lru_cache(maxsize=None)
def analysis_problem():
    """d = 20, N_t = 140, two error sources, a general (dense) projector: 280 k_u_interaction items, and
    k_u_expect's general-projector branch above 12 levels."""
    fp = S.dense_error_problem(ANALYSIS_D, ANALYSIS_NT, rank=12, nerr=2)
    return fp.replace(projector=dense_projector(ANALYSIS_D, 6, ANALYSIS_PROJ_SEED))


def analysis_x():
    return S.dense_x(ANALYSIS_NT, seed=1777)


@functools.lru_cache(maxsize=None)
def decay_problem(decay=True):
    """d = 13, N_t = 260, one error source, -i gamma / 2 on three levels: 260 k_u_inverse items, and
    k_u_interaction reading C_k^-1.  decay=False: the Hermitian problem it was built from."""
    fp = S.dense_error_problem(DECAY_D, DECAY_NT, rank=10, nerr=1)
    return P.with_decay(fp, DECAY_GAMMA, DECAY_LEVELS) if decay else fp


def decay_x():
    return S.dense_x(DECAY_NT, seed=1860)


@functools.lru_cache(maxsize=None)
def general_problem():
    """d = 13, N_t = 90, two error sources, one additional parameter, decay: 990 k_u_vmats items (about four per
    workgroup) and 540 k_u_assemble items on the general-H0 fidelity path."""
    fp = S.dense_error_problem(GENERAL_D, GENERAL_NT, rank=10, nerr=2, phase=True)
    return P.with_decay(fp, GENERAL_GAMMA, DECAY_LEVELS)


def general_x(seed=1990):
    return dense_x(GENERAL_NT, True, seed)


# ---- k_u_fid_contract past its grid cap: the d = 5 symmetric problem, two error sources, general path forced
LONG_NT, LONG_SEED, LONG_ERRORS = 5500, 5500, ("amp", "freq")
LONG_X_STRIDE = 50               # the fixture keeps x[::LONG_X_STRIDE]
# the bound of tests/test_gpu_unitary_wrap.py's long test: the tier plus this multiple of the fixture's recorded
# max|oracle - exact| of the same output (chosen from the device's measured distances, see that test's docstring)
LONG_NOISE_MULTIPLE = 1
LONG_OUTPUTS = ("F", "F_dx", "F_d2err", "F_d2err_dx")


def long_problem():
    return P.sym_problem(LONG_NT, errors=LONG_ERRORS)


def long_x():
    return P.random_x(LONG_NT, LONG_SEED)


def long_tiers(fp, x):
    """(relative, absolute) tier per output, as tests/test_gpu_general_h0.py: T1; fd_tier; T2 + T2_ABS; T3 + T3_ABS."""
    t, ta = P.fd_tier(fp, x)
    return {"F": (0.0, 1e-12), "F_dx": (t, ta), "F_d2err": (1e-6, 1e-7), "F_d2err_dx": (1e-5, 1e-7)}


def long_bounds(golden, fp, x):
    """{output: (bound, scale)}: tier(scale) + LONG_NOISE_MULTIPLE * the recorded max|oracle - exact|."""
    out = {}
    for name, (rel, ab) in long_tiers(fp, x).items():
        scale = float(np.max(np.abs(golden[name])))
        out[name] = (rel * scale + ab + LONG_NOISE_MULTIPLE * float(golden["noise_" + name]), scale)
    return out


def long_tail_rows():
    """The rows of F_d2err_dx that k_u_fid_contract's waves reach only on their second trip: items from
    FID_CONTRACT_ITEMS on, item = (1 + e) N_t np + k np + p -- the second error source at steps k >= 5384."""
    first = FID_CONTRACT_ITEMS - 2 * LONG_NT
    return slice(first, LONG_NT), 1


# ---- a chain that becomes exactly singular
# The C5 family with one error source, its last level cut off (row and column zeroed in every H0 and error
# operator) and given a decay that control 0 scales: H0 += -i (gamma / 2) x_0 |l><l|.  The level's entry of C_k is
# then prod_j exp(-(gamma dt / 2) x_{0,j}), real.  With the hot control x_0 = 1 and gamma dt / 2 = 41.5 it is
# e^-705.5 = 4e-307 at k = 17, the smallest it gets as a normal double (DBL_MIN = e^-708.4), and e^-747 at
# k = 18, below half the smallest subnormal (e^-745.1): exactly 0 under round-to-nearest and under flush-to-zero
# alike.  |dt H0|_1 = 41.5 is Pade 13 with three squarings (5.4 x 2^3 = 43.2), the regime the exponential tests
# cover at 30 (tests/test_gpu_dense_general.py NORMS); a step that skips the subnormal range has to be at least
# 36.7 = ln(DBL_MIN / (denorm_min / 2)) long, so none of the range below 30 can do it.
SING_NT, SING_STEP, SING_DIMS = 20, 41.5, (5, 13)
SING_ZERO_AT = 18                # 1-based: C_17 is the last invertible chain element


@functools.lru_cache(maxsize=None)
def singular_problem(d):
    fp = S.dense_error_problem(d, SING_NT, rank=min(16, d - 3), nerr=1)
    up = fp.unitary_problem
    dt = up.t0 / up.ntimes
    last = d - 1

    def cut(t):
        op = np.array(t.op, dtype=np.complex128)
        op[last, :] = 0.0
        op[:, last] = 0.0
        return Term(op, var=t.var, index=t.index, func=t.func, a=t.a, b=t.b, scale=t.scale)
    G = np.zeros((d, d), np.complex128)
    G[last, last] = 1.0
    gamma = 2.0 * SING_STEP / dt
    H0 = OperatorBasisHamiltonian([cut(t) for t in up.H0.terms]
                                  + [Term(G, var=VAR_X, index=0, func=FN_LINEAR, scale=-0.5j * gamma)])
    errs = [ErrorSource(OperatorBasisError([cut(t) for t in es.Herror.terms])) for es in up.error_sources]
    return fp.replace(unitary_problem=up.replace(H0=H0, error_sources=errs))


SING_DEEP_STEPS = 12             # the deep control: hot for this many steps, then cool


def singular_x(hot, seed=2100, deep=False):
    """Control 0: 1 at every step (hot: the chain underflows), or U[0.002, 0.02) (cool: the level decays by
    e^-0.08 .. e^-0.83 per step); control 1 ~ U[-1, 1).  deep: hot for the first SING_DEEP_STEPS steps and cool
    after them -- the level's entry of C_k falls to e^-498 = 5e-217 and stays a normal double, so the chain is
    invertible (Julia's inv returns 1 / it = 2e216), yet its squared modulus is far below DBL_MIN."""
    x = S.dense_x(SING_NT, seed=seed).reshape(SING_NT, NP)
    x[:, 0] = 1.0 if hot else np.random.default_rng(seed + 1).uniform(0.002, 0.02, size=SING_NT)
    if deep:
        x[:SING_DEEP_STEPS, 0] = 1.0
    return x.ravel()


def chain_diagonal(fp, x, level):
    """|C_k[level, level]|, k = 1 .. N_t, of the oracle's chain (oracle/grape_oracle.py julia_exp)."""
    from oracle import grape_oracle as O
    up = fp.unitary_problem
    xm = np.asarray(x[:up.ntimes * NP]).reshape(up.ntimes, NP)
    dt = up.t0 / up.ntimes
    C = np.eye(up.ndim, dtype=np.complex128)
    out = []
    for k in range(up.ntimes):
        C = O.julia_exp(-1j * dt * np.asarray(up.H0(k + 1, xm[k], np.zeros(0)), np.complex128)) @ C
        out.append(abs(C[level, level]))
    return np.array(out)
