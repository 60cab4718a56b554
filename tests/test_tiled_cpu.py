"""CPU-side checks of the tiled engine's boundary (64 < ndim <= 128): what plan creation
accepts and what it refuses is decided on the host, before any device work, so a machine without a GPU
sees GRAPE_ERR_UNSUPPORTED (with its message) for every refused case and GRAPE_ERR_NO_DEVICE -- never
UNSUPPORTED -- for a problem the engine serves."""
import os
import re

import numpy as np
import pytest

from robustgrape_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED, NO_DEVICE = -2, -6


def _create(fp, **kw):
    """Status code and message of grape_plan_create for the problem (0: created, and destroyed again)."""
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    try:
        GrapePlan(fp, nparam=2, max_batch=1, **kw).close()
    except _capi.GrapeError as e:
        return e.code, str(e)
    return 0, ""


def test_a_65_level_operator_basis_problem_is_not_refused():
    code, msg = _create(S.dense_problem(65, 3, rank=16))
    assert code in (0, NO_DEVICE), (code, msg)
    code, msg = _create(S.dense_error_problem(128, 2, rank=16, nerr=0, phase=True))  # the x_add target, d = 128
    assert code in (0, NO_DEVICE), (code, msg)


def _with_h0(fp, terms):
    from robustgrape_amd.operators import OperatorBasisHamiltonian
    return fp.replace(unitary_problem=fp.unitary_problem.replace(H0=OperatorBasisHamiltonian(terms)))


def test_what_the_tiled_engine_does_not_serve_is_refused_on_the_host():
    from robustgrape_amd.operators import FN_LINEAR, OPT_GENERAL_H0, VAR_XADD, Term
    from tests import problems as P
    fp = S.dense_problem(65, 3, rank=16)
    h0 = list(fp.unitary_problem.H0.terms)
    full = np.full((65, 65), 0.01) + np.diag([1.0] * 16 + [0.0] * 49)  # a full, non-diagonal projector
    xadd = S.dense_error_problem(65, 3, rank=16, nerr=0, phase=True)   # (one additional parameter)
    cases = {
        "ndim > GRAPE_MAX_TILED_DIM": (S.dense_problem(129, 2, rank=16), {}),
        "error sources": (S.dense_error_problem(65, 3, rank=16, nerr=1), {}),
        "x_add": (_with_h0(xadd, list(xadd.unitary_problem.H0.terms) +
                           [Term(S._hermitian(65, 70), var=VAR_XADD, index=0, func=FN_LINEAR)]), {}),
        "projector": (fp.replace(projector=full), {}),
        "GRAPE_OPT_GENERAL_H0": (fp, {"options": OPT_GENERAL_H0}),
        "Hermitian": (_with_h0(fp, h0 + [Term(np.triu(np.ones((65, 65), complex)))]), {}),
        "closures": (P.as_closures(fp), {}),
    }
    for needle, (prob, kw) in cases.items():
        code, msg = _create(prob, **kw)
        assert code == UNSUPPORTED and needle in msg, (needle, code, msg)


def test_the_header_declares_the_tiled_limit_and_keeps_the_abi():
    from robustgrape_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "grape.h")).read()
    assert int(re.search(r"#define GRAPE_MAX_TILED_DIM (\d+)", hdr).group(1)) == 128
    assert int(re.search(r"#define GRAPE_MAX_DENSE_DIM (\d+)", hdr).group(1)) == 64
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 12 == _capi.ABI_VERSION
    assert _capi.lib().grape_abi_version() == 12


def test_the_tiled_unit_is_built_and_hashed():
    from robustgrape_amd import build
    names = [os.path.basename(s) for s in build.SOURCES]
    assert "grape_tiled.hip" in names
    assert "grape_tiled.hip" in [os.path.basename(u[0]) for u in build._units(())[1]]
    deps = {os.path.basename(d) for d in build.DEPS}
    assert {"grape_tiled.hip", "grape_tiled.hpp", "grape_tiled_api.hpp"} <= deps
