"""The conditions that make the cases of tests/small_expm_cases.py bite, pinned without a GPU, and one cross-check
of the reference itself (oracle.grape_exact.exp_ld against mpmath at 40 digits)."""
import numpy as np
import pytest

from tests import small_expm_cases as C


def test_exp_ld_against_mpmath_at_40_digits():
    """exp_ld is the reference of every exponential test of d <= 128 here: three cases (no symmetry with seven
    squarings' worth of norm, row interchanges, decay) against mpmath.expm at 40 digits.  exp_ld's own error is
    about 1e-19 2^s relative (oracle.grape_exact.squarings); the bound is ten times that."""
    import mpmath

    from oracle import grape_exact as X
    for d, name in ((5, "ginibre30.0"), (12, "interchange0.01"), (7, "decay4.0")):
        A = C.case_map(d)[name]
        with mpmath.workdps(40):
            R = mpmath.expm(mpmath.matrix(A.tolist()))
            ref = np.array([[complex(R[i, j]) for j in range(d)] for i in range(d)])
            E = X.exp_ld(A.astype(np.clongdouble))
            # the difference in 40 digits, from the longdouble entries split into two doubles
            hi = np.asarray(E, np.complex128)
            lo = np.asarray(E - hi.astype(np.clongdouble), np.complex128)
            diff = max(abs(mpmath.mpc(hi[i, j]) + mpmath.mpc(lo[i, j]) - R[i, j]) for i in range(d) for j in range(d))
            scale = max(abs(R[i, j]) for i in range(d) for j in range(d))
        rel = float(diff / scale)
        bound = 1e-18 * 2 ** X.squarings(float(np.abs(A).sum(axis=0).max()))
        print(f"exp_ld vs mpmath d={d} {name}: rel {rel:.2e} bound {bound:.1e}")
        assert rel <= bound, (d, name, rel, bound)
        assert C.rel_err(np.asarray(E, np.complex128), ref) <= 4e-16


@pytest.mark.parametrize("d", C.DIMS)
def test_cases_are_deterministic_and_complete(d):
    first = C.cases(d)
    names = [n for n, _ in first]
    assert len(names) == len(set(names)) == 2 * len(C.NORMS) + 2 + len(C.THRESHOLDS) + 4 + 2
    again = C.cases.__wrapped__(d)  # built anew, past the cache
    assert again is not first and [n for n, _ in again] == names
    for (_, A), (_, B) in zip(again, first):
        assert np.array_equal(A, B)
    for n in C.seam_names(d) + C.parked_names(d):
        assert n in names
    for n in C.parked_names(d):
        assert C.degree(C.case_map(d)[n])[0] > 5, (d, n)
    kinds = [C.degree(C.case_map(d)[n])[0] for n in C.seam_names(d)]
    assert kinds.count(0) >= 3 and sum(1 for m in kinds if m in (3, 5)) >= 3 and sum(1 for m in kinds if m > 5) >= 4


@pytest.mark.parametrize("d", C.DIMS)
def test_family_norms_and_degrees(d):
    """ginibre and decay: the norm asked for (to rounding), hence m = 3, 5, 7, 9, 13 (s = 0), 13 (s = 2), 13 (s = 3);
    decay has a real part, ginibre no symmetry."""
    cm = C.case_map(d)
    want = [(3, 0), (5, 0), (7, 0), (9, 0), (13, 0), (13, 2), (13, 3)]
    for kind in ("ginibre", "decay"):
        for nm, ms in zip(C.NORMS, want):
            A = cm[f"{kind}{nm}"]
            assert abs(C.norm1(A) - nm) <= 1e-14 * nm and C.degree(A) == ms, (d, kind, nm)
            assert not np.allclose(A, -A.conj().T)
        assert np.min(np.diag(cm[f"{kind}1.5"]).real) < 0 if kind == "decay" else True


@pytest.mark.parametrize("d", C.DIMS)
def test_interchange_cases_exchange_rows(d):
    """zgetrf of the Pade-13 denominator V - U returns pivots that differ from the identity, and the denominator
    fails gesv_cols' dominance test (its diagonal is ~1e-16 c0 on the paired levels)."""
    from scipy.linalg import lapack
    for g in (0.0, 0.01):
        A = C.case_map(d)[f"interchange{g}"]
        assert C.degree(A) == (13, 0)
        Y = C.denominator(A)
        _, piv, info = lapack.zgetrf(np.asfortranarray(Y))
        assert info == 0 and not np.array_equal(piv, np.arange(d)), (d, g, piv)
        m1 = np.abs(Y.real) + np.abs(Y.imag)
        mx = np.maximum(np.abs(Y.real), np.abs(Y.imag))
        dominant = [mx[i, i] >= 1.5 * (m1[:, i].sum() - m1[i, i]) and mx[i, i] > 0 for i in range(d)]
        assert not all(dominant), (d, g)


def test_threshold_cases_sit_on_the_thresholds_and_fill_every_slot():
    """The norm obtained is the target or a neighbouring double; the expected degree follows from the norm read
    back; over d = 2 .. 12 every stats slot is hit by a threshold case."""
    slots = set()
    for d in C.DIMS:
        for t in C.THRESHOLDS:
            A = C.case_map(d)[f"on{t}"]
            assert np.all((A.real == 0) | (A.imag == 0))
            n = C.norm1(A)
            cs = np.zeros(d)
            for row in A:  # exact moduli: hypot, |.| and sqrt(re re + im im) agree, summed in the kernels' order
                cs = cs + np.abs(row)
            assert n == float(cs.max())
            assert C.ulps_from(n, t) <= 1, (d, t, n)
            slots.add(C.SLOT[C.degree(A)[0]])
    assert slots == {0, 1, 2, 3, 4}, slots


@pytest.mark.parametrize("d", C.DIMS)
def test_diagonal_and_lastcol_cases(d):
    cm = C.case_map(d)
    assert not np.any(cm["zero"]) and C.degree(cm["zero"]) == (0, 0)
    A = cm["diag_imag"]
    assert C.is_diag(A) and not np.any(A.real) and np.all(np.diag(A).imag != 0)
    A = cm["diag_decay"]
    assert C.is_diag(A) and np.all(np.diag(A).real < 0) and C.norm1(A) > 5.4
    B = cm["diag_off1e-300"]
    assert not C.is_diag(B) and np.count_nonzero(B - A) == 1 and B[0, d - 1] == 1e-300
    assert C.degree(B) == (13, 1)
    L = cm["lastcol"]
    cols = np.abs(L).sum(axis=0)
    assert np.array_equal(L, -L.conj().T)
    assert np.argmax(cols) == d - 1 and 3.3 < cols[d - 1] <= 4.1 and cols[d - 1] > 1.1 * cols[:d - 1].max(), (d, cols)
    assert C.degree(L) == (13, 0)
    R = cm["rankone5.3"]
    assert np.allclose(np.abs(R).sum(axis=0), 5.3, rtol=1e-14, atol=0) and C.degree(R) == (13, 0)
    assert abs(np.max(np.abs(np.linalg.eigvals(R))) - 5.3) < 1e-12  # spectral radius = 1-norm: A^13 at full size
    assert 5.3 ** 13 / 64764752532480000.0 > 1e3 * C.tol(R)  # the top Pade-13 term (4e-8) against the tier


@pytest.mark.parametrize("d", C.DIMS)
def test_double_restatement_is_within_a_tenth_of_the_tier(d):
    """Every case is well enough conditioned for its tier: the device's algorithm restated in double (Julia's U
    and V, no balancing, LAPACK gesv, squarings) lies within one tenth of the case's tolerance of exp_ld."""
    refs = C.references(d)
    worst = 0.0
    for name, A in C.cases(d):
        rel = C.rel_err(C.pade_double(A), refs[name])
        worst = max(worst, rel / C.tol(A))
        assert rel <= 0.1 * C.tol(A), (d, name, rel, C.tol(A))
    print(f"d={d}: worst restatement error / tier {worst:.3f}")


def test_probe_problem_steps_are_the_matrices_exactly():
    """tests/test_gpu_small_expm.py probe_problem: A_k = -i dt H0(k, x_k) is the matrix asked for, bit for bit, and
    the zero matrix on the other steps, for the closure and for the operator basis called as one."""
    from tests.test_gpu_small_expm import HOT, probe_problem
    d, steps = 5, [None, 3, 0, None, 5]
    mats = [C.case_map(d)[n] for n in HOT]
    for device in (False, True):
        up, x = probe_problem(d, mats, steps, device)
        assert up.t0 / up.ntimes == 1.0
        xm = x.reshape(len(steps), len(mats))
        for k, p in enumerate(steps):
            A = -1j * up.H0(k + 1, xm[k], np.zeros(0))
            assert np.array_equal(A, mats[p] if p is not None else np.zeros((d, d))), (device, k)
