"""The block-structure problems of tests/sector_problems.py and the sector layout rule, on the host.

* the generator does what it says: the union sparsity pattern has exactly the requested components, the fixed
  levels are fixed, the closure form returns the operator-basis matrices, scattering the labels changes no F;
* the layout table (sector_problems.CASES) and two refusals, through the library's own host logic: validate_desc,
  choose_route, setup_projector and idle_levels of grape_descriptor.hip, then grape_plan_setup.hpp find_sectors.
  tests/c/descriptor_check.cpp and grape_descriptor.hip are built as plain C++ by the host compiler under
  AddressSanitizer and UBSan and run as a child process, with levels ascending inside each component and padding
  slots last; the idle mask of idle_levels equals its restatement here (_idle) in every case;
* malformed descriptors: validate_desc returns an error code, with nothing for the sanitizers to report;
* the hidden-block cases: grape_symmetry_basis block-diagonalises them with the expected block sizes;
* the condition of tests/test_gpu_sector_shapes.py's comparison against the exact evaluator: the oracle's own
  distance from the exact F_dx lies inside fd_tier for every case, so the device test leans on no noisy checker."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import problems as P
from tests import sector_problems as SP
from tests.test_symmetry_cpu import _basis, _check_block_diagonal, _used_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or "/opt/rocm/llvm/bin/clang++"
OPT_NO_SYMMETRY = 1024
ERR_INVALID = -1  # GRAPE_ERR_INVALID
NT = 5


def _components(ops, d):
    """Connected components of the union pattern (ascending levels, by first level) and the levels with a
    nonzero diagonal: a restatement of find_sectors' first half."""
    adj = np.zeros((d, d), bool)
    for o in ops:
        adj |= (o != 0) | (o != 0).T
    seen, comps = np.zeros(d, bool), []
    for i in range(d):
        if seen[i]:
            continue
        todo, comp = [i], {i}
        while todo:
            for j in np.flatnonzero(adj[todo.pop()]):
                if j not in comp:
                    comp.add(int(j))
                    todo.append(int(j))
        seen[list(comp)] = True
        comps.append(sorted(comp))
    return comps, np.diag(adj)


@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_generator_components_fixed_levels_and_closures(name):
    comps, nfixed, kw, _ = SP.CASES[name]
    kw = {k: v for k, v in kw.items() if k != "err_couples"}
    fp = SP.block_problem(comps, nfixed, NT, **dict(kw, nparam=2, nerr=max(3, kw.get("nerr", 0)), xadd_h0=True))
    d = fp.unitary_problem.ndim
    perm, labels, fixed = SP.block_layout(comps, nfixed, kw["seed"])
    got, diag = _components(_used_ops(fp), d)
    want = sorted([lv.tolist() for lv in labels] + [[int(f)] for f in fixed])
    assert sorted(got) == want
    for f in fixed:  # a zero row and column in every used operator
        assert all(not np.any(o[f, :]) and not np.any(o[:, f]) for o in _used_ops(fp))
    for lv in labels:
        if len(lv) > 1:  # not contiguous (the components interleave) and fully coupled in every block operator
            assert lv[-1] - lv[0] > len(lv) - 1
            assert np.all(fp.unitary_problem.H0.terms[0].op[np.ix_(lv, lv)] != 0)
        else:            # the lone level: a diagonal entry of its own
            assert diag[lv[0]]
    # projector: diagonal, non-negative, non-uniform, with zeros; no weighted level in its component's first slot
    w = np.diag(fp.projector)
    assert np.count_nonzero(fp.projector - np.diag(w)) == 0 and np.all(w >= 0)
    assert np.any(w == 0) or max(comps) == 1  # (all-diagonal H0: an unweighted lone level would be idle)
    assert len(set(w[w > 0].tolist())) > 1
    assert all(w[lv[0]] == 0 for lv in labels if len(lv) > 1)
    # the closure form: the same matrices
    fc = SP.block_problem(comps, nfixed, NT, **dict(kw, nparam=2, nerr=max(3, kw.get("nerr", 0)), xadd_h0=True,
                                                    device=False))
    x = SP.block_x(NT, kw["seed"], 2, 2)[1]
    xm, xa = x[:2 * NT].reshape(NT, 2), x[2 * NT:]
    up, uc = fp.unitary_problem, fc.unitary_problem
    assert not hasattr(uc.H0, "terms") and not hasattr(fc.target_unitary, "terms")
    np.testing.assert_array_equal(uc.H0(3, xm[2], xa), up.H0(3, xm[2], xa))
    np.testing.assert_array_equal(fc.target_unitary(xa), fp.target_unitary(xa))
    for e in range(3):
        np.testing.assert_array_equal(uc.error_sources[e].Herror(3, xm[2], xa, 1e-4),
                                      up.error_sources[e].Herror(3, xm[2], xa, 1e-4))
    # the step norm the tiers go by
    assert abs(P.max_step_norm(fp, SP.block_x(NT, kw["seed"], 2, 2), 2) - 0.2) < 1e-12


@pytest.mark.parametrize("name", ["c431", "c4321f", "c3221"])
def test_scattering_the_labels_changes_no_fidelity(name):
    from oracle import grape_oracle as O
    x = SP.case_x(name, NT)[0]
    F = [O.calculate_fidelity_and_derivatives(SP.case_problem(name, NT, device=False, scatter=s, target="dense"), x)[0]
         for s in (True, False)]
    assert abs(F[0] - F[1]) <= 1e-12 and 1e-3 < F[0] < 1 - 1e-3


# ---------------------------------------------------------------------------------------------------------------
# the layout rule
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not shutil.which(CXX):
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("sectors") / "descriptor_check")
    csrc = os.path.join(ROOT, "robustgrape_amd", "csrc")
    subprocess.run([CXX, "-O1", "-std=c++17", "-fsanitize=address,undefined", "-I" + csrc,
                    "-I" + os.path.join(ROOT, "include"), "-x", "c++", os.path.join(ROOT, "tests", "c", "descriptor_check.cpp"),
                    os.path.join(csrc, "grape_descriptor.hip"), "-o", exe], check=True, capture_output=True)
    return exe


def _idle(fp):
    """grape_descriptor.hip idle_levels restated: no projector weight and no target entry beside the diagonal."""
    d = fp.unitary_problem.ndim
    W = np.asarray(fp.projector)
    if np.count_nonzero(W - np.diag(np.diag(W))):
        return np.zeros(d, bool)
    idle = np.diag(W) == 0
    for t in fp.target_unitary.terms:
        off = (t.op != 0) & ~np.eye(d, dtype=bool)
        idle &= ~(off.any(axis=0) | off.any(axis=1))
    return idle


def _run(checker, fp, tmp_path, options, broken="ok"):
    """tests/c/descriptor_check.cpp on the problem: its output lines."""
    up = fp.unitary_problem
    d = up.ndim
    ops, index = [], {}

    def op_id(m):
        if id(m) not in index:
            index[id(m)] = len(ops)
            ops.append(np.asarray(m, np.complex128))
        return index[id(m)]
    h0 = [op_id(t.op) for t in up.H0.terms]
    errs = [[op_id(t.op) for t in es.Herror.terms] for es in up.error_sources]
    tgt = [op_id(t.op) for t in fp.target_unitary.terms]
    lines = [f"{d} {len(ops)} {len(h0)} {len(errs)} {options}", " ".join(map(str, h0))]
    lines += [" ".join(map(str, [len(e)] + e)) for e in errs + [tgt]]
    lines.append(f"{up.ntimes} 1 {up.nb_additional_param}")
    W = np.asarray(fp.projector, np.complex128)
    if np.count_nonzero(W - np.diag(np.diag(W))) or np.any(np.diag(W).imag):
        lines.append("full " + " ".join(f"{float(v.real)!r} {float(v.imag)!r}" for v in W.flatten(order="F")))
    else:
        lines.append("diag " + " ".join(repr(float(v.real)) for v in np.diag(W)))
    lines.append(broken)
    for o in ops:
        nz = np.argwhere(o != 0)
        lines.append(str(len(nz)))
        lines += [f"{r} {c} {float(o[r, c].real)!r} {float(o[r, c].imag)!r}" for r, c in nz]
    path = tmp_path / "problem.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([checker, str(path)], check=True, capture_output=True, text=True)
    assert run.stderr == ""  # no sanitizer report
    return run.stdout.splitlines()


def _layout(checker, fp, tmp_path, options=OPT_NO_SYMMETRY):
    """find_sectors on the problem's operators, with the idle levels of idle_levels: ([(S, nsec, sidx (nsec, S))],
    fixed levels)."""
    out = _run(checker, fp, tmp_path, options)
    assert out[0].split()[:2] == ["validate", "0"] and out[1] == "route 0"
    assert [int(v) for v in out[2].split()] == _idle(fp).astype(int).tolist()  # idle_levels and its restatement
    out = out[3:]
    ncls, nfixed = (int(v) for v in out[0].split())
    cls = []
    for c in range(ncls):
        S, nsec = (int(v) for v in out[1 + 2 * c].split())
        cls.append((S, nsec, np.array(out[2 + 2 * c].split(), int).reshape(nsec, S)))
    fixed = [int(v) for v in out[1 + 2 * ncls].split()] if len(out) > 1 + 2 * ncls else []
    assert len(fixed) == nfixed
    return cls, fixed


def _check_slots(cls, fixed, fp):
    """Every level that evolves and can reach F sits in exactly one slot; inside a sector the components follow
    each other whole, levels ascending, and the padding slots come last."""
    d = fp.unitary_problem.ndim
    comps, diag = _components(_used_ops(fp), d)
    idle = _idle(fp)
    want_fixed = sorted(c[0] for c in comps if len(c) == 1 and not diag[c[0]])
    assert sorted(fixed) == want_fixed and fixed == sorted(fixed)
    left_out = [c[0] for c in comps if len(c) == 1 and diag[c[0]] and idle[c[0]]]
    slots = []
    for S, nsec, sidx in cls:
        for row in sidx:
            live = row[row >= 0]
            assert len(live) >= 1 and np.all(row[len(live):] == -1)  # padding last
            slots += live.tolist()
            at = 0
            while at < len(live):  # one whole component after the other
                comp = next(c for c in comps if live[at] in c)
                assert live[at:at + len(comp)].tolist() == comp  # ascending, complete
                at += len(comp)
    assert sorted(slots + fixed + left_out) == list(range(d))


@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_layout_table(checker, name, tmp_path):
    fp = SP.case_problem(name, NT)
    cls, fixed = _layout(checker, fp, tmp_path)
    assert tuple((S, nsec) for S, nsec, _ in cls) == SP.CASES[name][3]
    assert len(fixed) == SP.CASES[name][1]
    _check_slots(cls, fixed, fp)
    if name == "merge":  # without the error source that couples two of H0's components
        f0 = SP.case_problem(name, NT, nerr=0)
        cls0, fixed0 = _layout(checker, f0, tmp_path)
        assert tuple((S, nsec) for S, nsec, _ in cls0) == SP.MERGE_WITHOUT and fixed0 == []
        _check_slots(cls0, fixed0, f0)
    if name == "c3221-idle":  # the lone level is in no slot and not fixed
        lone = SP.block_layout(*SP.CASES[name][:2], SP.CASES[name][2]["seed"])[1][3][0]
        assert fixed == [] and all(lone not in sidx for _, _, sidx in cls)


@pytest.mark.parametrize("nerr", [0, 2])
def test_layout_with_error_sources_and_two_controls_is_the_table(checker, nerr, tmp_path):
    """Error sources with the same blocks and a second control change no layout."""
    for name in ("c431", "c4321f", "c532f"):
        fp = SP.case_problem(name, NT, nerr=nerr, nparam=2, xadd_h0=True)
        cls, fixed = _layout(checker, fp, tmp_path)
        assert tuple((S, nsec) for S, nsec, _ in cls) == SP.CASES[name][3]
        _check_slots(cls, fixed, fp)


def test_layout_refusals(checker, tmp_path):
    # one component of 5 and one fixed level at d = 6: 2 * 125 > 216
    assert _layout(checker, SP.block_problem((5,), 1, NT, seed=41), tmp_path) == ([], [])
    # the same component at d = 7 (two fixed levels) passes: 250 <= 343
    cls, fixed = _layout(checker, SP.block_problem((5,), 2, NT, seed=41), tmp_path)
    assert [(S, n) for S, n, _ in cls] == [(5, 1)] and len(fixed) == 2
    # one class with one sector and no fixed level: a single component, and two lone levels sharing the one sector
    assert _layout(checker, SP.block_problem((4,), 0, NT, seed=42), tmp_path) == ([], [])
    w = [1.0, 0.5, 0.0, 0.0]
    assert _layout(checker, SP.block_problem((1, 1, 1, 1), 0, NT, seed=43, weights=w), tmp_path) == ([], [])
    w[2] = 2.0  # a third live level: two sectors
    cls, _ = _layout(checker, SP.block_problem((1, 1, 1, 1), 0, NT, seed=43, weights=w), tmp_path)
    assert [(S, n) for S, n, _ in cls] == [(2, 2)]
    # GRAPE_OPT_NO_SECTORS
    assert _layout(checker, SP.case_problem("c431", NT), tmp_path, options=1) == ([], [])


@pytest.mark.parametrize("broken, message", [("op", "H0: op out of range"),
                                             ("offsets", "each error source needs at least one term")])
def test_malformed_descriptors_are_refused(checker, broken, message, tmp_path):
    """A term whose op is n_ops, and err_term_offsets that decrease: validate_desc claims both and returns
    GRAPE_ERR_INVALID before anything indexes with them.  (nerr > 0 with a null err_terms is not among its claims:
    it checks err_term_offsets alone, so that case is not run.)"""
    fp = SP.case_problem("c431", NT, nerr=2)
    assert _run(checker, fp, tmp_path, OPT_NO_SYMMETRY)[0].split()[:2] == ["validate", "0"]
    assert _run(checker, fp, tmp_path, OPT_NO_SYMMETRY, broken) == [f"validate {ERR_INVALID} {message}"]


# ---------------------------------------------------------------------------------------------------------------
# hidden blocks
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SP.HIDDEN))
@pytest.mark.parametrize("nerr", [0, 1])
def test_hidden_blocks_are_found(name, nerr):
    comps, _, layout = SP.HIDDEN[name]
    fp = SP.case_problem(name, NT, nerr=nerr)
    d = fp.unitary_problem.ndim
    got, _ = _components(_used_ops(fp), d)
    assert got == [list(range(d))]  # no permutation sectors
    rc, V, blk, _ = _basis(fp)
    assert rc == 1
    _check_block_diagonal(V, blk, _used_ops(fp))
    assert sorted(np.bincount(blk)[np.bincount(blk) > 0].tolist()) == sorted(comps)
    assert sorted((S, n) for S, n in layout) == sorted((S, comps.count(S)) for S in set(comps))


# ---------------------------------------------------------------------------------------------------------------
# the checker's own noise
# ---------------------------------------------------------------------------------------------------------------
EXACT_NT = 37


def exact_case(name, nt=EXACT_NT):
    """(device-form problem, closure form, controls) of the comparison against the exact evaluator: the table
    case without error sources."""
    return (SP.case_problem(name, nt, nerr=0, err_couples=None),
            SP.case_problem(name, nt, nerr=0, err_couples=None, device=False), SP.case_x(name, nt))


@pytest.mark.parametrize("nt", [EXACT_NT, 1])
@pytest.mark.parametrize("name", sorted(SP.CASES))
def test_oracle_is_within_the_tier_of_the_exact_gradient(name, nt):
    """Rows 0 and 3 at 37 steps and at one step: the rows tests/test_gpu_sector_shapes.py compares with the oracle
    (row 0 at 37 steps also with the exact evaluator).  The seeds of sector_problems.CASES were chosen for this."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    fp, fo, X = exact_case(name, nt)
    for b in (0, 3):
        t2, t2a = P.fd_tier(fp, X[b])
        assert (t2, t2a) == (1e-7, 1e-9)
        F, g = E.fidelity_and_gradient(fp, X[b])
        F0, g0 = O.calculate_fidelity_and_derivatives(fo, X[b])[:2]
        err, scale = np.max(np.abs(np.asarray(g0) - g)), np.max(np.abs(g))
        print(f"{name} nt {nt} row {b}: oracle - exact F {abs(F - F0):.1e} F_dx {err:.2e} (scale {scale:.2e}, "
              f"tier {t2 * scale + t2a:.2e})")
        assert abs(F - F0) <= 1e-12
        assert err <= t2 * scale + t2a, (err, scale)


@pytest.mark.parametrize("projector", [None, "dense"])
@pytest.mark.parametrize("name", sorted(SP.HIDDEN))
def test_oracle_is_within_the_tier_on_the_hidden_cases(name, projector):
    """The same condition for the hidden-block cases as the device test runs them (13 steps, rows 0 and 3, the
    diagonal and the dense projector)."""
    from oracle import grape_exact as E
    from oracle import grape_oracle as O
    fp, X = SP.case_problem(name, 13), SP.case_x(name, 13)
    if projector:
        fp = fp.replace(projector=SP.dense_projector(fp.unitary_problem.ndim, seed=fp.unitary_problem.ndim))
    for b in (0, 3):
        t2, t2a = P.fd_tier(fp, X[b])
        F, g = E.fidelity_and_gradient(fp, X[b])
        F0, g0 = O.calculate_fidelity_and_derivatives(fp, X[b])[:2]
        err, scale = np.max(np.abs(np.asarray(g0) - g)), np.max(np.abs(g))
        assert (t2, t2a) == (1e-7, 1e-9) and abs(F - F0) <= 1e-12
        assert err <= t2 * scale + t2a, (err, scale)
