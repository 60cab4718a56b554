"""The phase-covariant walks' test family on the CPU (tests/problems.py GAUGE_FAMILY, full9_family, relabel):
the fixtures of tests/test_gpu_gauge_family.py checked without a GPU.

* full9_family's operator-basis form equals rydberg_hamiltonian_full (RydbergTools.jl:118-130) with the om01 /
  d0r / a / b changes written out by hand here, and its closure form;
* a relabelled problem has the F and F_dx of the problem it was built from (the oracle,
  FidelityCalculations.jl:19-119 restated): F within 1e-13, F_dx within the two evaluations' summed distances
  from the exact forward difference (oracle/grape_exact.py);
* the symmetry-adapted basis (grape_symmetry_basis, host code) still splits the 4-level component 3 + 1 for
  every case, so the merged plans stay reachable; and the weighted level's in-sector index where the cases
  say it moves."""
import numpy as np
import pytest

from robustgrape_amd import rydberg as R
from tests import problems as P

CASES = list(P.GAUGE_FAMILY)
NT = 24


@pytest.mark.parametrize("kw", [dict(), dict(delta=0.7), dict(a=-2.5, b=0.7), dict(om01=0.8, d0r=0.4),
                                dict(a=0.5, b=-1.1, delta=0.3, om=0.6, B=0.0), dict(B=500.0, om=1.3, d0r=-0.2)])
def test_operator_basis_form_is_the_reference_hamiltonian(kw):
    rng = np.random.default_rng(11)
    dev, clo = P.full9_family(8, **kw), P.full9_family(8, device=False, **kw)
    om, a, b = kw.get("om", 1.0), kw.get("a", 1.0), kw.get("b", 0.0)
    delta, B = kw.get("delta", 0.0), kw.get("B", 10.0)
    worst = 0.0
    for _ in range(6):
        x, k = float(rng.uniform(-40.0, 40.0)), int(rng.integers(1, 9))
        phi = a * x + b
        H = R.rydberg_hamiltonian_full(phi, om, om, delta, delta, B)
        if "om01" in kw:
            H[1, 4], H[4, 1] = np.exp(-1j * phi) * kw["om01"] / 2, np.exp(1j * phi) * kw["om01"] / 2
        H[4, 4] += kw.get("d0r", 0.0)
        assert np.array_equal(H, H.conj().T)
        for f in (dev, clo):
            Hf = np.asarray(f.unitary_problem.H0(k, [x], [0.3]))
            err = float(np.max(np.abs(Hf - H)))
            worst = max(worst, err / (1e-15 * np.max(np.abs(H))))
            assert err <= 1e-15 * np.max(np.abs(H)), (x, err)
    print(f"full9_family {kw}: worst max|dH| / (1e-15 max|H|) = {worst:.2e}")
    assert np.array_equal(dev.target_unitary([0.3]), clo.target_unitary([0.3]))


def test_relabel_moves_operators_and_projector():
    perm = [8 - i for i in range(9)]
    fp = P.relabel(P.full9_problem(4, nerr=2), perm)
    base = P.full9_problem(4, nerr=2)
    H, Hb = fp.unitary_problem.H0(1, [0.4], [0.2]), base.unitary_problem.H0(1, [0.4], [0.2])
    E = fp.unitary_problem.error_sources[1].Herror(1, [0.4], [0.2], 0.5)
    Eb = base.unitary_problem.error_sources[1].Herror(1, [0.4], [0.2], 0.5)
    T, Tb = fp.target_unitary([0.2]), base.target_unitary([0.2])
    for i in range(9):
        for j in range(9):
            assert H[perm[i], perm[j]] == Hb[i, j] and E[perm[i], perm[j]] == Eb[i, j] and T[perm[i], perm[j]] == Tb[i, j]
            assert fp.projector[perm[i], perm[j]] == base.projector[i, j]
    clo = P.relabel(P.full9_problem(4, nerr=2, device=False), perm)
    assert np.array_equal(clo.unitary_problem.H0(1, [0.4], [0.2]), H)
    # (the closure's error term is a difference of two Hamiltonians: rounding)
    assert np.max(np.abs(clo.unitary_problem.error_sources[1].Herror(1, [0.4], [0.2], 0.5) - E)) <= 1e-15


@pytest.mark.parametrize("case", [c for c in CASES if P.GAUGE_FAMILY[c][1] is not None])
def test_relabelled_case_keeps_fidelity_and_gradient(case):
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    fp, base = P.gauge_family_problem(case, NT)
    for seed, small in ((3, False), (4, True)):
        x = P.random_x(NT, seed, small=small)
        F1, g1 = O.calculate_fidelity_and_derivatives(fp, x)[:2]
        F0, g0 = O.calculate_fidelity_and_derivatives(base, x)[:2]
        Fe1, e1 = E.fidelity_and_gradient(fp, x)
        Fe0, e0 = E.fidelity_and_gradient(base, x)
        g1, g0 = np.asarray(g1), np.asarray(g0)
        d1, d0 = float(np.max(np.abs(g1 - e1))), float(np.max(np.abs(g0 - e0)))
        err = float(np.max(np.abs(g1 - g0)))
        print(f"relabel {case} seed {seed}: |dF| {abs(F1 - F0):.2e} (bound 1e-13), exact |dF| {abs(Fe1 - Fe0):.2e}, "
              f"max|dF_dx| {err:.2e} (bound {d1:.2e} + {d0:.2e}), exact max|dF_dx| {float(np.max(np.abs(e1 - e0))):.2e}")
        assert abs(F1 - F0) <= 1e-13 and abs(Fe1 - Fe0) <= 1e-13
        assert err <= d1 + d0


@pytest.mark.parametrize("case", CASES)
def test_symmetry_basis_splits_the_four_level_component(case):
    from tests.test_symmetry_cpu import _basis, _check_block_diagonal, _used_ops
    fp, _ = P.gauge_family_problem(case, 8)
    rc, V, blk, _ = _basis(fp)
    assert rc == 1
    _check_block_diagonal(V, blk, _used_ops(fp))
    perm = P.GAUGE_FAMILY[case][1] or list(range(9))
    four = [perm[i] for i in (3, 6, 7, 8)]          # |11>, |1r>, |r1>, |rr>
    # the rotation mixes only |1r> and |r1>; |11> and |rr> keep their blocks' label, with one of the two mixed
    # columns (the bright state), the other (the dark state) a block of its own
    b11 = blk[perm[3]]
    assert blk[perm[8]] == b11 and sorted(np.bincount(blk)[np.bincount(blk) > 0].tolist()) == [1, 1, 2, 2, 3]
    assert sorted(np.flatnonzero(blk == b11).tolist())[0] in four and set(np.flatnonzero(blk == b11)) <= set(four)
    assert blk[perm[1]] == blk[perm[4]] and blk[perm[2]] == blk[perm[5]] and blk[perm[1]] != blk[perm[2]]


def test_weighted_level_moves_where_the_cases_say():
    c = {case: P.weighted_indices(P.gauge_family_problem(case, 8)[0]) for case in CASES}
    print(c)
    for case in ("detuned", "scaled", "mixed", "stiff", "unequal"):
        assert c[case][3] == [0] and c[case][2] == [0, 0], (case, c[case])
    assert c["swap-A"][3] == [2] and c["swap-A"][2] == [0, 0]
    assert c["swap-B2"][3] == [0] and c["swap-B2"][2] == [1, 1]
    assert c["swap-B1"][3] == [0] and c["swap-B1"][2] == [1, 0]
    assert None not in c["reversed"][3] + c["reversed"][2]
