"""Inputs of the small engine's exponential tests (d = 2 .. 12: grape_device.hpp's row-group exponential, the
kernels k_expm, k_expm_table, k_expm_grad, k_expm_high, k_grad_high and k_expm_raw): pure numpy builders, seeded by
d, and the properties that make each case bite, so that tests/test_small_expm_cases_cpu.py can pin them without a
GPU and tests/test_gpu_small_expm.py cannot pass vacuously.  The reference of exp is oracle.grape_exact.exp_ld
(longdouble Taylor 40).

Families, for each d:
  ginibre, decay   tests/test_gpu_dense_general.py _family (no symmetry; skew-Hermitian plus a negative real diagonal),
                   rescaled to the 1-norms NORMS
  interchange      that file's _interchange(d, ginibre) for ginibre 0.0 and 0.01: d // 2 pairs with A^2 = -pi^2 I, so
                   the diagonal of the Pade-13 denominator V - U vanishes there and zgetrf exchanges rows
  threshold        tests/test_gpu_tiled_edges.py _on_threshold (entries purely real or purely imaginary: the device's
                   column sums are the host's to the bit), rescaled onto THRESHOLDS
  diagonal         zero; a purely imaginary diagonal; a diagonal with negative real parts and 1-norm > 5.4; that
                   diagonal with one off-diagonal entry of 1e-300, which is not diagonal any more
  lastcol          a skew-Hermitian matrix whose 1-norm is carried by column d - 1 alone
  rankone          5.3 i v v^dagger with |v_k| = 1 / sqrt(d): every column sum and the spectral radius are 5.3, so
                   A^13 is as large as the norm allows and the top Pade-13 coefficient carries 4e-8 of the result
                   (in the random families the spectral radius is a fraction of the 1-norm and that term is below
                   the tier at most sizes)
"""
import functools
import math

import numpy as np

DIMS = tuple(range(2, 13))
NORMS = (0.01, 0.2, 0.6, 1.5, 4.0, 12.0, 30.0)
THRESHOLDS = (0.015, 0.25, 0.95, 2.1, 5.4, 10.8)
SLOT = {0: 0, 3: 0, 5: 1, 7: 2, 9: 3, 13: 4}  # stats slot of a degree; 0: the isdiag shortcut counts in slot 0
T0, T0_PADE13 = 1e-13, 1e-12


def gpw(d):
    """Matrices per 64-lane wave (grape_device.hpp Geo<D>::GPW)."""
    return 64 // d


def norm1(A):
    """|A|_1 in the kernels' order (expm_prologue): lane c adds sqrt(re re + im im) down column c, row after row."""
    cs = np.zeros(A.shape[1])
    for row in A:
        cs = cs + np.sqrt(row.real * row.real + row.imag * row.imag)
    return float(cs.max())


def is_diag(A):
    return not np.any(A - np.diag(np.diag(A)))


def degree(A):
    """(m, s) the device takes for A: (0, 0) for a diagonal matrix (the shortcut returns before any degree is
    chosen), else Julia's choice at the 1-norm in the kernels' order."""
    from oracle import grape_oracle as O
    return (0, 0) if is_diag(A) else O.pade_degree(norm1(A))


def tol(A):
    """T0 as tests/test_gpu_dense_general.py and tests/test_gpu_tiled_edges.py state it: relative max-entry error
    1e-13 max(1, |A|_1), 1e-12 max(1, |A|_1) where the degree is 13."""
    return (T0_PADE13 if degree(A)[0] == 13 else T0) * max(1.0, norm1(A))


def histogram(mats):
    h = [0] * 5
    for A in mats:
        h[SLOT[degree(A)[0]]] += 1
    return h


def pade_double(A):
    """The device's algorithm in double: Julia's U and V with no balancing, LAPACK gesv, squarings; a diagonal
    matrix by exp of its diagonal."""
    from scipy.linalg import lapack
    A = np.array(A, np.complex128)
    m, s = degree(A)
    if m == 0:
        return np.diag(np.exp(np.diag(A)))
    V, U = pade_uv(A / float(2 ** s), m)
    _, _, X, info = lapack.zgesv(np.asfortranarray(V - U), np.asfortranarray(V + U))
    assert info == 0
    for _ in range(s):
        X = X @ X
    return X


def pade_uv(A, m):
    """(V, U) of Julia's exp! at degree m: exp(A) ~ (V - U)^-1 (V + U)."""
    from oracle import grape_oracle as O
    I = np.eye(A.shape[0], dtype=np.complex128)
    A2 = A @ A
    if m <= 9:
        C = O._PADE[m]
        P, U, V = I.copy(), C[1] * I, C[0] * I
        for kk in range(1, len(C) // 2):
            P = P @ A2
            U = U + C[2 * kk + 1] * P
            V = V + C[2 * kk] * P
        return V, A @ U
    C = O._PADE13
    A4 = A2 @ A2
    A6 = A2 @ A4
    U = A @ (A6 @ (C[13] * A6 + C[11] * A4 + C[9] * A2) + C[7] * A6 + C[5] * A4 + C[3] * A2 + C[1] * I)
    V = A6 @ (C[12] * A6 + C[10] * A4 + C[8] * A2) + C[6] * A6 + C[4] * A4 + C[2] * A2 + C[0] * I
    return V, U


def denominator(A):
    """V - U of the case at the degree and scaling the device takes: the matrix its solve factorises."""
    m, s = degree(A)
    V, U = pade_uv(np.array(A, np.complex128) / float(2 ** s), m)
    return V - U


def rel_err(E, ref):
    return float(np.max(np.abs(E - ref)) / np.max(np.abs(ref)))


def _lastcol(d, rng):
    """tests/test_gpu_tiled_edges.py's construction: last column (and, skew-Hermitian, last row) of moduli
    3.55 / (d - 1), the rest a Hermitian Ginibre of norm 0.5.  At d = 2 the rest is one diagonal entry, which would
    add to column 0: it goes to the last diagonal entry instead."""
    G = rng.normal(size=(d, d)) + 1j * rng.normal(size=(d, d))
    H = (G + G.conj().T) / 2
    H[:, d - 1] = H[d - 1, :] = 0.0
    H = H / np.abs(H).sum(axis=0).max() * 0.5
    if d == 2:
        H[1, 1], H[0, 0] = H[0, 0], 0.0
    v = np.exp(2j * np.pi * rng.uniform(size=d - 1)) * (3.55 / (d - 1))
    H[:d - 1, d - 1] = v
    H[d - 1, :d - 1] = v.conj()
    return -1j * H


def _rankone(d, rng, norm=5.3):
    v = np.exp(2j * np.pi * rng.uniform(size=d)) / np.sqrt(d)
    return 1j * norm * np.outer(v, v.conj())


def _threshold(d, rng, target):
    """_on_threshold, then the largest entry of the norm's column moved by what is still missing (the rescaling
    alone can stop two doubles off): the norm ends on the target or a neighbouring double."""
    from tests.test_gpu_tiled_edges import _on_threshold
    A = _on_threshold(d, rng, target)
    for _ in range(20):
        n = norm1(A)
        if n == target:
            break
        c = int(np.argmax(np.abs(A).sum(axis=0)))
        r = int(np.argmax(np.abs(A[:, c])))
        A[r, c] *= 1.0 + (target - n) / abs(A[r, c])
    return A


def _diagonals(d, rng):
    im = rng.uniform(-3.0, 3.0, size=d)
    dec = -rng.uniform(0.5, 5.0, size=d) + 1j * rng.uniform(-3.0, 3.0, size=d)
    dec[d - 1] = -6.0 + 2.0j  # |A|_1 = 6.32 > 5.4: off the shortcut this would be Pade 13 with one squaring
    off = np.diag(dec)
    off[0, d - 1] = 1e-300
    return [("zero", np.zeros((d, d), complex)), ("diag_imag", np.diag(1j * im)), ("diag_decay", np.diag(dec)),
            ("diag_off1e-300", off)]


@functools.lru_cache(maxsize=None)
def cases(d):
    """Ordered (name, A) of every case at size d; deterministic."""
    from tests.test_gpu_dense_general import _family, _interchange
    out = []
    for kind, seed in (("ginibre", 7100), ("decay", 7200)):
        rng = np.random.default_rng(seed + d)
        out += [(f"{kind}{nm}", _family(kind, d, nm, rng)) for nm in NORMS]
    out += [(f"interchange{g}", _interchange(d, g)) for g in (0.0, 0.01)]
    rng = np.random.default_rng(7300 + d)
    out += [(f"on{t}", _threshold(d, rng, t)) for t in THRESHOLDS]
    out += _diagonals(d, np.random.default_rng(7400 + d))
    out.append(("lastcol", _lastcol(d, np.random.default_rng(7500 + d))))
    out.append(("rankone5.3", _rankone(d, np.random.default_rng(7600 + d))))
    for _, A in out:
        A.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case_map(d):
    return dict(cases(d))


@functools.lru_cache(maxsize=None)
def references(d):
    """name -> exp_ld(A) rounded to double, computed once per size and shared (read-only)."""
    from oracle import grape_exact as X
    refs = {}
    for name, A in cases(d):
        R = np.asarray(X.exp_ld(A.astype(np.clongdouble)), np.complex128)
        R.setflags(write=False)
        refs[name] = R
    return refs


def seam_names(d):
    """Ten cases alternating the shortcut, the in-kernel low degrees, row interchanges and norm-30 items: cycled
    through a batch, every wave mixes groups that return early, groups that finish in k_expm_raw and parked ones."""
    return ("diag_imag", "ginibre0.01", "interchange0.0", "ginibre30.0", "diag_decay", "decay0.2", "interchange0.01",
            "decay30.0", "zero", "ginibre0.2")


def parked_names(d):
    """Five cases that all park (m > 5) for k_expm_high."""
    return ("ginibre0.6", "decay1.5", "ginibre4.0", "interchange0.01", "decay30.0")


def ulps_from(v, target):
    """How many doubles v lies from target (0: equal)."""
    n, w = 0, v
    while w != target and n < 4:
        w = math.nextafter(w, target)
        n += 1
    return n
