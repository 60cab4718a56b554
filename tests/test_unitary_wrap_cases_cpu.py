"""The case table of tests/test_gpu_unitary_wrap.py (tests/unitary_wrap_cases.py), checked without a GPU: every
case exceeds the launch cap of the kernels it names, and the oracle-side conditions the GPU tests rely on hold.

The two caps restate C++ constants: W.RESIDENT is grape_unitary_api.hpp kResident (the workgroups of a launch
above kMaxD = 12 levels, grape_unitary.hip grid_for) and W.FID_CONTRACT_ITEMS the 4096 blocks x 4 waves of
k_u_fid_contract (grape_unitary.hip launch_fidelity).  Whoever retunes either learns here that the GPU cases no
longer take a second item."""
import os
import re

import numpy as np
import pytest

from tests import problems as P
from tests import unitary_wrap_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robustgrape_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "general_long.npz")


def _src(name):
    with open(os.path.join(CSRC, name)) as fh:
        return fh.read()


def test_caps_are_the_sources_constants():
    api = _src("grape_unitary_api.hpp")
    assert int(re.search(r"constexpr int kResident = (\d+);", api).group(1)) == W.RESIDENT
    assert int(re.search(r"constexpr int kMaxD = (\d+);", api).group(1)) == W.MAX_LDS_DIM
    hip = _src("grape_unitary.hip")
    assert int(re.search(r"constexpr int BLOCK = (\d+);", hip).group(1)) // 64 == 4
    m = re.search(r"k_u_fid_contract, dim3\(\(unsigned\)std::min<long>\(\(items \+ per - 1\) / per, (\d+)\)\)", hip)
    assert int(m.group(1)) * 4 == W.FID_CONTRACT_ITEMS


def _assert_wraps(d, counts, kernels, label):
    assert d > W.MAX_LDS_DIM, label
    for k in kernels:
        assert counts[W.KERNEL_COUNT[k]] > W.RESIDENT, (label, k, counts)


@pytest.mark.parametrize("case", list(W.TENSOR_CASES))
def test_tensor_cases_wrap_where_they_claim(case):
    d, nt, ne, phase = case
    up, x = W.tensor_case(*case)
    counts = W.item_counts(nt, W.NP, int(phase), ne)
    assert (up.ndim, up.ntimes, len(up.error_sources), up.nb_additional_param) == (d, nt, ne, int(phase))
    assert x.shape == (nt * W.NP + int(phase),)
    _assert_wraps(d, counts, W.TENSOR_CASES[case], case)
    if not W.TENSOR_CASES[case]:  # the d = 64 case with error sources: one item per workgroup
        assert max(counts) <= W.RESIDENT and d == 64 and ne == 2 and phase


def test_tensor_case_counts_are_the_documented_ones():
    got = {c: W.item_counts(c[1], W.NP, int(c[3]), c[2])[:2] for c in W.TENSOR_CASES}
    assert got == {(13, 140, 0, False): (280, 280), (16, 48, 2, True): (528, 288), (64, 130, 0, False): (260, 260),
                   (64, 6, 2, True): (66, 36)}
    na, ne = 1, 2
    assert na + ne + na * ne == 5  # k_u_reduce's outputs in the (16, 48) case


@pytest.mark.parametrize("name", list(W.PLAN_CASES))
def test_plan_cases_wrap_where_they_claim(name):
    d, nt, ne, phase, kernels = W.PLAN_CASES[name]
    fp = {"analysis": W.analysis_problem, "decay": W.decay_problem, "general": W.general_problem}[name]()
    up = fp.unitary_problem
    assert (up.ndim, up.ntimes, len(up.error_sources), up.nb_additional_param) == (d, nt, ne, int(phase))
    counts = W.item_counts(nt, W.NP, int(phase), ne)
    _assert_wraps(d, counts, kernels, name)
    if name == "analysis":
        assert counts[3] == 280
        P0 = np.asarray(fp.projector)
        assert np.count_nonzero(P0) == d * d and abs(np.trace(P0) - 6.0) < 1e-12  # k_u_expect's gen_proj branch
    if name == "decay":
        assert counts[2] == 260 and counts[3] == 260
    if name == "general":
        assert counts[:2] == (990, 540)


def test_decay_is_visible_in_the_decay_case():
    """The oracle-side condition of the non-Hermitian analysis case: gamma = 0.02 over 260 steps moves F by
    far more than any tier (as tests/test_gpu_dense_general.py test_decay_plans_match_live_oracle asserts)."""
    from oracle import grape_oracle as O
    x = W.decay_x()
    F = O.calculate_fidelity_and_derivatives(W.decay_problem(), x)[0]
    F_plain = O.calculate_fidelity_and_derivatives(W.decay_problem(decay=False), x)[0]
    assert abs(F - F_plain) > 1e-4, (F, F_plain)


def test_long_case_passes_the_contract_cap_and_its_fixture_is_current():
    fp, x = W.long_problem(), W.long_x()
    up = fp.unitary_problem
    counts = W.item_counts(W.LONG_NT, 1, up.nb_additional_param, len(up.error_sources))
    assert up.ndim <= W.MAX_LDS_DIM  # LDS tiles: only k_u_fid_contract strides here
    assert counts[1] == 16500 > W.FID_CONTRACT_ITEMS
    rows, e = W.long_tail_rows()
    assert (rows.start, rows.stop, e) == (5384, 5500, 1)
    assert (1 + e) * W.LONG_NT + rows.start == W.FID_CONTRACT_ITEMS
    g = dict(np.load(GOLDEN, allow_pickle=False))
    assert os.path.getsize(GOLDEN) < 169 * 1024  # below the largest fixture, expm.npz
    assert list(g["params"]) == [W.LONG_NT, W.LONG_SEED, W.LONG_X_STRIDE]
    assert np.array_equal(g["x_sample"], x[::W.LONG_X_STRIDE])
    assert g["F_dx"].shape == (W.LONG_NT + 1,) and g["F_d2err_dx"].shape == (W.LONG_NT + 1, 2)
    # every bound stays below 1e-2 of the output's scale: a skipped or stale item is off by about the scale
    for name, (bound, scale) in W.long_bounds(g, fp, x).items():
        assert bound < 1e-2 * scale, (name, bound, scale)
    # ... also on the rows the second trip writes alone
    tail = g["F_d2err_dx"][rows, e]
    assert W.long_bounds(g, fp, x)["F_d2err_dx"][0] < 1e-2 * np.max(np.abs(tail))


@pytest.mark.parametrize("d", W.SING_DIMS)
def test_singular_case_underflows_to_an_exact_zero(d):
    """Hot control: the cut-off level's entry of C_k is a normal double until it is exactly 0 (never subnormal,
    so the device's pivot test sees the same zero whatever its denormal mode), the step norm stays in Pade 13
    with three squarings, and the oracle raises from all three entry points.  Cool control: nothing underflows."""
    from oracle import grape_oracle as O
    fp = W.singular_problem(d)
    up = fp.unitary_problem
    hot, cool = W.singular_x(True), W.singular_x(False)
    tiny = np.finfo(np.float64).tiny
    diag = W.chain_diagonal(fp, hot, d - 1)
    assert np.all((diag == 0.0) | (diag >= tiny)), diag
    assert np.all(diag[:W.SING_ZERO_AT - 1] >= tiny) and np.all(diag[W.SING_ZERO_AT - 1:] == 0.0), diag
    norm = P.max_step_norm(fp, hot, W.NP)
    assert abs(norm - W.SING_STEP) < 1e-9 and O.pade_degree(norm * (1 + 1e-6)) == (13, 3)
    for fn, arg in ((O.calculate_fidelity_and_derivatives, fp), (O.calculate_unitary_and_derivatives, up),
                    (O.calculate_interaction_error_operators, up)):
        with pytest.raises(np.linalg.LinAlgError):
            fn(arg, hot)
    assert W.chain_diagonal(fp, cool, d - 1)[-1] > 1e-8
    assert P.max_step_norm(fp, cool, W.NP) < 5.4
    assert np.isfinite(O.calculate_fidelity_and_derivatives(fp, cool)[0])


@pytest.mark.parametrize("d", W.SING_DIMS)
def test_deep_case_is_invertible_with_an_underflowing_squared_pivot(d):
    """The deep control: every chain entry of the cut-off level is a normal double, the smallest has a finite
    reciprocal but a squared modulus of exactly 0, and the oracle returns finite values from all three entry
    points (nothing for a device to refuse)."""
    from oracle import grape_oracle as O
    fp = W.singular_problem(d)
    up = fp.unitary_problem
    x = W.singular_x(False, deep=True)
    diag = W.chain_diagonal(fp, x, d - 1)
    assert np.all(diag >= np.finfo(np.float64).tiny)
    assert diag.min() ** 2 == 0.0 and np.isfinite(1.0 / diag.min())
    assert abs(P.max_step_norm(fp, x, W.NP) - W.SING_STEP) < 1e-9
    outs = (list(O.calculate_fidelity_and_derivatives(fp, x)) + list(O.calculate_unitary_and_derivatives(up, x))
            + [O.calculate_interaction_error_operators(up, x)])
    assert all(np.all(np.isfinite(a)) for a in outs)
