"""Host checks of tests/projector_cases.py: the projector generators keep their guarantees on every
case of the table; a numpy model of the formulas the general heads implement (the header comments of
grape_projector.hip and of k_u_fid_head in grape_unitary.hip) reproduces the oracle; that model with
B^dagger replaced by B differs under pattern_projector and does not under dense_projector; and the
oracle's own noise on every Hermitian case leaves the device half of the tier it is held to."""
import numpy as np
import pytest

from tests import projector_cases as PC

PATTERN = [c.name for c in PC.CASES.values() if c.proj == "pattern"]
EXACT = [c.name for c in PC.CASES.values() if PC.exact_in_scope(c)]
MODEL = ["dims3_ne2", "xadd5_whole", "decay9_xadd"]   # np = 2 / na = 1; H0 reading x_add, na = ne = 2; the same with decay


def test_the_table_names_every_group_and_size():
    groups = {}
    for c in PC.CASES.values():
        groups.setdefault(c.group, []).append(c)
    assert sorted(groups) == ["a", "b", "c", "d"]
    assert sorted({c.d for c in groups["a"] if c.builder == "dims"}) == [2, 3, 7, 8, 12]
    assert {(c.nerr, c.nt) for c in groups["a"] if c.builder == "dims"} == {(0, 9), (2, 5)}
    assert {(c.d, c.nt, c.nerr, c.phase) for c in groups["b"] if c.builder == "dense"} == {
        (13, 3, 0, False), (17, 3, 2, True), (33, 4, 0, False), (48, 3, 1, False), (64, 3, 2, True)}
    assert all(c.nt <= 9 for c in PC.CASES.values())
    assert sum(c.d >= 48 for c in PC.CASES.values()) == 2   # the longdouble evaluator takes seconds there
    # the general path sees na >= 2 together with ne >= 2, with and without decay
    for g in "cd":
        assert any(PC.base_problem(c).unitary_problem.nb_additional_param >= 2 and c.nerr >= 2 for c in groups[g])


@pytest.mark.parametrize("name", PATTERN)
def test_pattern_projector_keeps_its_guarantees(name):
    c = PC.CASES[name]
    P0 = PC.projector(c)
    assert P0.shape == (c.d, c.d) and P0.dtype == np.float64
    p = PC.pattern_properties(P0)
    assert p["mask_asymmetric"] and p["rank_A"] >= 2 and p["A_asymmetry"] > 1e-2 and p["trace"] >= 1.0, p
    off = P0[~np.eye(c.d, dtype=bool)]
    assert np.all(np.abs(off) <= 0.5)
    dg = np.diag(P0)
    assert np.all((dg == 0.0) | ((dg >= 0.5) & (dg <= 1.0)))
    assert np.array_equal(P0, PC.pattern_projector(c.d, c.pseed))   # deterministic


def test_pattern_projector_statistics():
    """Density `fill` off the diagonal and about a quarter of the diagonal exactly zero, over many draws."""
    offs, zeros = [], []
    for seed in range(40):
        P0 = PC.pattern_projector(12, 1000 + 7 * seed)
        offs.append(np.mean(P0[~np.eye(12, dtype=bool)] != 0))
        zeros.append(np.mean(np.diag(P0) == 0))
    assert abs(np.mean(offs) - 0.4) < 0.03 and abs(np.mean(zeros) - 0.25) < 0.06
    assert abs(np.mean(PC.pattern_projector(33, 5, fill=0.1)[~np.eye(33, dtype=bool)] != 0) - 0.1) < 0.03


def test_weighted_diagonal_stays_diagonal_with_fractional_weights():
    for c in PC.CASES.values():
        if c.proj != "weighted":
            continue
        W = PC.projector(c)
        assert np.array_equal(W, np.diag(np.diag(W)))
        assert set(np.diag(W).tolist()) == {0.0, 0.5, 1.0} and np.trace(W) >= 1.0
    assert any(c.proj == "weighted" for c in PC.CASES.values())


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("name", MODEL)
def test_head_formulas_reproduce_the_oracle(name):
    """The formulas the kernels implement (F, G, G_e, the target parts) against the reference's literal
    trace expressions: F to 1e-14, everything else to 1e-12 relative."""
    from oracle import grape_oracle as O
    c = PC.CASES[name]
    fp, x = PC.problem(c, device=False), PC.control(c)
    up = fp.unitary_problem
    assert len(up.error_sources) == 2 and up.nb_additional_param >= 1
    F0, g0, e0, ed0 = O.calculate_fidelity_and_derivatives(fp, x)
    F, g, e, ed, G, M = PC.head_model(fp, x)
    assert abs(F - F0) <= 1e-14, (F, F0)
    assert _rel(g, g0) <= 1e-12 and _rel(e, e0) <= 1e-12 and _rel(ed, ed0) <= 1e-12, (_rel(g, g0), _rel(e, e0), _rel(ed, ed0))
    # the x_add entries carry a part of their own (not only relative to the largest entry)
    na = up.nb_additional_param
    assert np.max(np.abs(g[-na:] - g0[-na:])) <= 1e-12 * np.max(np.abs(g0[-na:]))
    assert np.max(np.abs(ed[-na:] - ed0[-na:])) <= 1e-12 * np.max(np.abs(ed0[-na:]))
    # grape_projector.hip's M is k_u_fid_head's G times U
    U = O.calculate_unitary_and_derivatives(up, x)[0]
    assert _rel(G @ U, M) <= 1e-13
    if c.decay:
        assert abs(abs(np.linalg.det(U)) - 1.0) > 1e-3   # not unitary


@pytest.mark.parametrize("name", ["dims7_ne2", "xadd9_whole", "dense33", "decay16_ne2"])
def test_b_dagger_matters_under_the_pattern_projector(name):
    c = PC.CASES[name]
    fp, x = PC.problem(c, device=False), PC.control(c)
    good, bad = PC.head_model(fp, x), PC.head_model(fp, x, swap_b=True)
    assert good[0] == bad[0]   # F holds no B^dagger
    assert _rel(bad[5], good[5]) > 1e-3 and _rel(bad[1], good[1]) > 1e-3, (_rel(bad[5], good[5]), _rel(bad[1], good[1]))
    if c.nerr:
        assert _rel(bad[3], good[3]) > 1e-3


@pytest.mark.parametrize("d,rank,seed", [(9, 4, 5), (13, 6, 43), (16, 6, 46)])
def test_b_dagger_is_invisible_under_the_dense_projector(d, rank, seed):
    """Why pattern_projector exists: with every entry nonzero P is the all-ones matrix, B = B^dagger, and the
    swap changes nothing at all."""
    from tests.test_gpu_projector import dense_projector
    c = PC.CASES["xadd9_whole" if d == 9 else "dense13" if d == 13 else "general16_ne2"]
    assert c.d == d
    P0 = dense_projector(d, rank, seed)
    assert np.all(P0 != 0)
    A = P0 @ np.ones((d, d))
    assert np.linalg.matrix_rank(A) == 1 and np.allclose(A, A[:, :1])   # constant rows
    fp, x = PC.base_problem(c, device=False).replace(projector=P0), PC.control(c)
    good, bad = PC.head_model(fp, x), PC.head_model(fp, x, swap_b=True)
    for a, b in zip(good, bad):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", EXACT)
def test_oracle_noise_stays_under_half_the_tier(name):
    """Condition on the inputs: the GPU test holds the device to the tier against the longdouble evaluation
    (F_dx: 1e-6 max|exact| + 1e-9; F_d2err, F_d2err_dx: T2, T3), and the device's own u / eps noise is of the
    oracle's kind -- so the oracle's distance from exact must leave half of the tier.  A case that does not
    gets another x seed (tests/projector_cases.py), never a wider tier."""
    x, ref, exact = PC.reference(name)
    assert abs(ref[0] - exact[0]) <= 1e-14
    for quantity, (dist, half) in PC.oracle_distances(name).items():
        print(f"{name} {quantity}: oracle - exact {dist:.2e}, half tier {half:.2e}")
        assert dist <= half, (name, quantity, dist, half)


def test_long_step_x_add_draws_keep_the_tier_above_their_noise():
    """The d = 9 draws with H0 reading x_add (tests/projector_cases.py XADD9_MIN_SCALE): the case's own and the rows
    of the closure batch have max|F_dx| >= 0.19, and the oracle keeps the half tier on every row."""
    from oracle import grape_oracle as O
    rows = 0
    for c in PC.CASES.values():
        if c.builder != "xadd" or c.d != 9 or c.decay:
            continue
        X = PC.batch_controls(c, 3) if c.name in PC.BATCH_XSEEDS else PC.control(c)[None, :]
        for x in X:
            ref = O.calculate_fidelity_and_derivatives(PC.problem(c, device=False), x)
            exact = PC.exact_outputs(c, x)
            assert np.max(np.abs(exact[1])) >= PC.XADD9_MIN_SCALE
            dist, half = PC.oracle_distances(c.name, ref, exact)["F_dx"]
            assert dist <= half, (c.name, dist, half)
            rows += 1
    assert rows == 4


def test_the_reference_is_shared_and_read_only():
    x, ref, exact = PC.reference("dims2_ne2")
    assert PC.reference("dims2_ne2")[1] is ref
    with pytest.raises(ValueError):
        ref[1][0] = 0.0
    with pytest.raises(ValueError):
        x[0] = 0.0


def test_decay_is_visible_in_every_decay_case():
    for c in PC.CASES.values():
        if c.decay and c.d <= 16:
            assert abs(PC.reference(c.name)[1][0] - PC.fidelity_without_decay(c.name)) > 1e-4, c.name


def test_exact_gradient_with_x_add_dependent_h0():
    """oracle/grape_exact.py fidelity_and_gradient_xadd: fidelity_and_gradient's value where H0 does not read
    x_add; with an H0 that does, the oracle's F_dx to its own u / eps noise, and the x_add entries against a
    central difference of the evaluator's own F (their H0 part is not small)."""
    from oracle import grape_exact as E
    c = PC.CASES["dims7_ne0"]
    x = PC.control(c)
    a, b = E.fidelity_and_gradient(PC.problem(c), x, 2), E.fidelity_and_gradient_xadd(PC.problem(c), x, 2)
    assert a[0] == b[0] and np.max(np.abs(a[1] - b[1])) <= 1e-15
    c = PC.CASES["xadd5_whole"]
    x, ref, exact = PC.reference(c.name)
    assert exact[2] is None and abs(ref[0] - exact[0]) <= 1e-14
    assert _rel(ref[1], exact[1]) <= 1e-6
    with pytest.raises(ValueError):
        E.fidelity_and_gradient(PC.problem(c).replace(unitary_problem=PC.problem(c).unitary_problem.replace(
            error_sources=[])), x, 1)   # the plain evaluator refuses this H0
    h = 1e-5
    for q in (1, 2):
        xp, xm = np.array(x), np.array(x)
        xp[-q] += h
        xm[-q] -= h
        fd = (E.fidelity_and_gradient_xadd(PC.problem(c), xp, 1)[0] - E.fidelity_and_gradient_xadd(PC.problem(c), xm, 1)[0]) / (2 * h)
        assert abs(fd - exact[1][-q]) <= 1e-6 * np.max(np.abs(exact[1])), (q, fd, exact[1][-q])
