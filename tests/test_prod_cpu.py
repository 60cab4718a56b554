"""Product coefficients in the operator basis (include/grape.h GRAPE_OP_FACTOR), everything that needs no
GPU: the descriptor's validation (grape_plan_create validates before it looks for a device), the refusal
above GRAPE_MAX_SMALL_DIM, the Python operator basis against plain closures, the order of the packed
terms, and the unchanged C layout."""
import ctypes
import math

import numpy as np
import pytest

from robustgrape_amd import _capi
from robustgrape_amd.operators import (FN_CIS, FN_COS, FN_LINEAR, FN_ONE, FN_SIN, MAX_FACTORS, OP_FACTOR, VAR_ONE,
                                       VAR_TSTEP, VAR_X, VAR_XADD, CTerm, DescriptorBuffers, Factor,
                                       OperatorBasisHamiltonian, OperatorBasisTarget, Term)
from tests import prod_problems as PP

INVALID, UNSUPPORTED, NO_DEVICE = -1, -2, -6


def _create_desc(desc):
    h = ctypes.c_void_p()
    rc = _capi.lib().grape_plan_create(ctypes.byref(desc), 0, ctypes.byref(h))
    msg = _capi.lib().grape_last_error().decode()
    if rc == 0:
        _capi.lib().grape_plan_destroy(h)
    return rc, msg


def _buffers(errors=("amp", "freq")):
    return DescriptorBuffers(PP.sym_problem(6, errors=errors), nparam=PP.NPARAM, max_batch=1)


def _terms(arr, n):
    return [(arr[i].op, arr[i].var, arr[i].index, arr[i].func) for i in range(n)]


def test_a_valid_product_problem_passes_validation():
    for errors in ((), ("amp", "freq")):
        rc, msg = _create_desc(_buffers(errors).desc)
        assert rc in (0, NO_DEVICE), (rc, msg)


def test_the_packed_terms_hold_each_factor_directly_after_its_term():
    buf = _buffers()
    d = buf.desc
    # H0: cos(phi) Hc, its amplitude factor, sin(phi) Hs, its amplitude factor
    assert d.n_h0_terms == 4
    assert _terms(d.h0_terms, 4) == [(0, VAR_X, 1, FN_COS), (OP_FACTOR, VAR_X, 0, FN_LINEAR),
                                     (1, VAR_X, 1, FN_SIN), (OP_FACTOR, VAR_X, 0, FN_LINEAR)]
    # the offsets count the factor rows: the amplitude error has 2 terms + 2 factors, the frequency error 1 term
    assert [d.err_term_offsets[i] for i in range(3)] == [0, 4, 5]
    got = _terms(d.err_terms, 5)
    assert [g[0] == OP_FACTOR for g in got] == [False, True, False, True, False]
    f = d.h0_terms[1]
    assert (f.a, f.b, f.scale_re, f.scale_im) == (1.0, 0.0, 1.0, 0.0)
    # two factors keep their order
    fp = PP.twice_problem()
    d2 = DescriptorBuffers(fp, nparam=2, max_batch=1).desc
    assert d2.n_h0_terms == 6
    assert _terms(d2.h0_terms, 6)[1:5] == [(OP_FACTOR, VAR_X, 0, FN_LINEAR), (1, VAR_X, 1, FN_COS),
                                          (OP_FACTOR, VAR_XADD, 1, FN_LINEAR), (OP_FACTOR, VAR_X, 0, FN_LINEAR)]
    # a problem without factors packs as before
    from tests import problems as P
    d0 = DescriptorBuffers(P.sym_problem(6, errors=("amp",)), nparam=1, max_batch=1).desc
    assert d0.n_h0_terms == 2 and all(d0.h0_terms[i].op >= 0 for i in range(2))


def _set(term, **kw):
    for k, v in kw.items():
        setattr(term, k, v)


def test_a_factor_that_starts_the_h0_list_is_invalid():
    buf = _buffers(())
    buf.desc.h0_terms[0].op = OP_FACTOR
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "must follow an operator term" in msg and msg.startswith("H0"), (rc, msg)


def test_a_factor_that_starts_an_error_sources_range_is_invalid():
    buf = _buffers()
    # the frequency error's only row (index 4) follows the amplitude error's last factor: as a factor it
    # would start the second source's range
    _set(buf.desc.err_terms[4], op=OP_FACTOR, var=VAR_X, index=0, func=FN_LINEAR)
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "must follow an operator term" in msg and msg.startswith("error source"), (rc, msg)


def test_a_third_factor_on_one_term_is_invalid():
    base = PP.twice_problem()
    up = base.unitary_problem
    t = up.H0.terms[1]
    assert len(t.factors) == MAX_FACTORS
    with pytest.raises(ValueError):
        Term(t.op, factors=t.factors + (Factor(VAR_X, 0),))
    buf = DescriptorBuffers(base, nparam=2, max_batch=1)
    # rows: term, f | term, f, f | term -> turn the last operator term into a third factor
    _set(buf.desc.h0_terms[5], op=OP_FACTOR, var=VAR_X, index=0, func=FN_LINEAR, scale_im=0.0)
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "GRAPE_MAX_FACTORS" in msg, (rc, msg)


def test_a_cis_or_complex_factor_is_invalid():
    buf = _buffers(())
    buf.desc.h0_terms[1].func = FN_CIS
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "ONE, LINEAR, COS or SIN" in msg, (rc, msg)
    buf = _buffers(())
    buf.desc.h0_terms[1].scale_im = 0.25
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "scale must be real" in msg, (rc, msg)
    with pytest.raises(ValueError):
        Factor(VAR_X, 0, FN_CIS)
    with pytest.raises(ValueError):
        Factor(VAR_X, 0, scale=1j)


def test_a_factor_validates_var_and_index_like_any_term():
    buf = _buffers(())
    buf.desc.h0_terms[1].index = PP.NPARAM
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "control index out of range" in msg, (rc, msg)
    buf = _buffers(())
    buf.desc.h0_terms[1].var = 7
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "bad var" in msg, (rc, msg)


def test_a_factor_in_the_target_is_invalid():
    buf = _buffers(())
    assert buf.desc.n_target_terms == 3
    _set(buf.desc.target_terms[1], op=OP_FACTOR, var=VAR_XADD, index=0, func=FN_COS, scale_im=0.0)
    rc, msg = _create_desc(buf.desc)
    assert rc == INVALID and "not allowed in target terms" in msg, (rc, msg)
    with pytest.raises(ValueError):
        OperatorBasisTarget([Term(np.eye(2, dtype=complex), factors=(Factor(VAR_XADD, 0),))])


@pytest.mark.parametrize("d", [13, 65])
def test_product_problems_above_the_small_engine_are_unsupported(d):
    buf = DescriptorBuffers(PP.wide_problem(d), nparam=PP.NPARAM, max_batch=1)
    rc, msg = _create_desc(buf.desc)
    assert rc == UNSUPPORTED and "product" in msg, (rc, msg)


def test_a_five_level_product_problem_is_never_unsupported():
    rc, msg = _create_desc(DescriptorBuffers(PP.sym_problem(5), nparam=PP.NPARAM, max_batch=1).desc)
    assert rc in (0, NO_DEVICE), (rc, msg)
    rc, msg = _create_desc(DescriptorBuffers(PP.wide_problem(12), nparam=PP.NPARAM, max_batch=1).desc)
    assert rc in (0, NO_DEVICE), (rc, msg)


FACTORS = [Factor(VAR_ONE, 0, FN_ONE, scale=0.75),
           Factor(VAR_X, 0),
           Factor(VAR_X, 1, FN_COS, a=1.3, b=0.2, scale=-0.5),
           Factor(VAR_X, 0, FN_SIN, a=-0.7, b=1.1),
           Factor(VAR_XADD, 1, FN_LINEAR, a=2.0, b=-0.3),
           Factor(VAR_XADD, 0, FN_COS),
           Factor(VAR_TSTEP, 0, FN_SIN, a=math.pi / 9, b=-0.5 * math.pi / 9),
           Factor(VAR_TSTEP, 0, FN_LINEAR, a=0.1, b=1.0, scale=2.0)]


def _closure_value(f, nt, x, xa):
    v = {VAR_ONE: 1.0, VAR_X: x[f.index] if f.var == VAR_X else 0.0, VAR_XADD: xa[f.index] if f.var == VAR_XADD else 0.0,
         VAR_TSTEP: float(nt)}[f.var]
    t = f.a * v + f.b
    return f.scale * {FN_ONE: lambda u: 1.0, FN_LINEAR: lambda u: u, FN_COS: math.cos, FN_SIN: math.sin}[f.func](t)


@pytest.mark.parametrize("i", range(len(FACTORS)))
def test_term_coefficient_multiplies_every_kind_of_factor(i):
    f = FACTORS[i]
    g = FACTORS[(i + 3) % len(FACTORS)]
    op = np.array([[0.0, 1.0], [1.0, 0.0]], complex)
    x, xa, nt = np.array([0.8, -2.1]), np.array([0.4, 1.7]), 4
    base = Term(op, var=VAR_X, index=1, func=FN_SIN, a=0.9, b=0.1, scale=1.5)
    c0 = 1.5 * math.sin(0.9 * x[1] + 0.1)
    assert base.coefficient(nt, x, xa) == pytest.approx(c0, rel=1e-15)
    one = Term(op, var=VAR_X, index=1, func=FN_SIN, a=0.9, b=0.1, scale=1.5, factors=(f,))
    assert one.coefficient(nt, x, xa) == pytest.approx(c0 * _closure_value(f, nt, x, xa), rel=1e-14, abs=1e-300)
    two = Term(op, var=VAR_X, index=1, func=FN_SIN, a=0.9, b=0.1, scale=1.5, factors=[f, g])
    assert two.factors == (f, g)
    want = c0 * _closure_value(f, nt, x, xa) * _closure_value(g, nt, x, xa)
    assert two.coefficient(nt, x, xa) == pytest.approx(want, rel=1e-14, abs=1e-300)
    H = OperatorBasisHamiltonian([two])
    np.testing.assert_allclose(H(nt, x, xa), want * op, rtol=1e-14, atol=0)
    assert H.depends_on_xadd() == (VAR_XADD in (f.var, g.var))


def test_the_rydberg_builders_with_an_amplitude_control_equal_the_scaled_closures():
    from robustgrape_amd import rydberg as R
    x, xa = np.array([0.83, 2.4]), np.array([0.0])
    H = R.rydberg_symmetric_blockaded_operator_basis(delta=0.3, param=1, amplitude_param=0)
    want = R.rydberg_hamiltonian_symmetric_blockaded(x[1], x[0] - 1.0, 0.3)  # (1 + eps) = Omega
    np.testing.assert_allclose(H(1, x, xa), want, atol=1e-15)
    H7 = R.rydberg_full_blockaded_operator_basis(param=1, amplitude_param=0)
    np.testing.assert_allclose(H7(1, x, xa), R.rydberg_hamiltonian_full_blockaded(x[1], x[0] - 1.0, 0.0), atol=1e-15)
    H9 = R.rydberg_full_operator_basis(1.0, 0.8, 0.1, 0.2, 10.0, param=1, amplitude_param=0)
    np.testing.assert_allclose(H9(1, x, xa), R.rydberg_hamiltonian_full(x[1], x[0], 0.8 * x[0], 0.1, 0.2, 10.0), atol=1e-15)
    E = R.symmetric_amplitude_error(param=1, amplitude_param=0)
    unit = R.rydberg_hamiltonian_symmetric_blockaded(x[1], 0.0, 0.0)
    np.testing.assert_allclose(E(1, x, xa, 1e-3), 1e-3 * x[0] * unit, atol=1e-18)
    E9 = R.full_rabi_error(2, param=1, amplitude_param=0)
    want9 = R.rydberg_hamiltonian_full(x[1], 0.0, x[0], 0, 0, 0.0)
    np.testing.assert_allclose(E9(1, x, xa, 1.0), want9, atol=1e-15)
    # the defaults build the objects they built before: no factors anywhere
    for obj in (R.rydberg_symmetric_blockaded_operator_basis(), R.rydberg_full_blockaded_operator_basis(),
                R.rydberg_full_operator_basis(), R.symmetric_amplitude_error(), R.full_blockaded_amplitude_error(),
                R.full_rabi_error(1)):
        assert all(t.factors == () for t in obj.terms)


def test_the_symmetry_basis_ignores_factor_terms():
    """grape_symmetry_basis (host code) of the d = 9 product problem is that of the phase-only problem:
    factor terms carry no operator."""
    from tests import problems as P
    V = []
    for fp, nparam in ((PP.full9_problem(4), PP.NPARAM), (P.full9_problem(4), 1)):
        buf = DescriptorBuffers(fp, nparam=nparam, max_batch=1)
        v = np.zeros(2 * 81)
        blk = (ctypes.c_int * 9)()
        rc = _capi.lib().grape_symmetry_basis(ctypes.byref(buf.desc), _capi.dptr(v), blk)
        assert rc == 1, _capi.lib().grape_last_error()
        V.append((v, list(blk)))
    assert np.array_equal(V[0][0], V[1][0]) and V[0][1] == V[1][1]


# sizeof / offsetof printed by tests/c/abi_check.c for ABI 12 before GRAPE_OP_FACTOR existed
LAYOUT_ABI12 = {
    "sizeof.grape_term": 48, "grape_term.op": 0, "grape_term.var": 4, "grape_term.index": 8, "grape_term.func": 12,
    "grape_term.a": 16, "grape_term.b": 24, "grape_term.scale_re": 32, "grape_term.scale_im": 40,
    "sizeof.grape_desc": 144, "grape_desc.ndim": 0, "grape_desc.ntimes": 4, "grape_desc.nparam": 8,
    "grape_desc.nadd": 12, "grape_desc.nerr": 16, "grape_desc.n_ops": 20, "grape_desc.t0": 24, "grape_desc.eps": 32,
    "grape_desc.eps2": 40, "grape_desc.projector_diag": 48, "grape_desc.ops": 56,
    "grape_desc.n_h0_terms": 64, "grape_desc.h0_terms": 72, "grape_desc.err_term_offsets": 80,
    "grape_desc.err_terms": 88, "grape_desc.n_target_terms": 96, "grape_desc.target_terms": 104,
    "grape_desc.max_batch": 112, "grape_desc.reserved": 116, "grape_desc.projector": 136,
}


def test_the_c_layout_and_the_abi_version_are_unchanged():
    from tests.test_c_abi import _layout
    lay = _layout()
    assert lay["abi_version"] == 12 and _capi.lib().grape_abi_version() == 12
    for key, want in LAYOUT_ABI12.items():
        assert lay[key] == want, (key, lay[key], want)
    assert ctypes.sizeof(CTerm) == 48
    hdr = open(_capi.os.path.join(_capi.os.path.dirname(_capi.HERE), "include", "grape.h")).read()
    assert "#define GRAPE_OP_FACTOR (-1)" in hdr and "#define GRAPE_MAX_FACTORS 2" in hdr
    assert "#define GRAPE_ABI_VERSION 12" in hdr
