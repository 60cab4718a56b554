"""CPU-side checks of the tiled engine's error-source option (GRAPE_OPT_TILED_ERR, 64 < ndim <= 128,
DESIGN.md 7.3 "Error sources"): the option lets error sources through on the host, the default plan refuses
them exactly as before, and everything the error path does not serve keeps a refusal of its own -- all
decided before any device work, so a machine without a GPU sees GRAPE_ERR_NO_DEVICE for what is served and
GRAPE_ERR_UNSUPPORTED with its key word for what is not."""
import os
import re

import numpy as np

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


def _with_errors(fp, sources):
    return fp.replace(unitary_problem=fp.unitary_problem.replace(error_sources=sources))


def _source(terms):
    from robustgrape_amd.operators import OperatorBasisError
    from robustgrape_amd.types import ErrorSource
    return ErrorSource(OperatorBasisError(terms))


def test_the_option_lets_error_sources_through_at_65_levels():
    from robustgrape_amd.operators import OPT_TILED_ERR
    code, msg = _create(S.dense_error_problem(65, 3, rank=16, nerr=1), options=OPT_TILED_ERR)
    assert code in (0, NO_DEVICE), (code, msg)
    code, msg = _create(S.dense_error_problem(128, 2, rank=16, nerr=2, phase=True), options=OPT_TILED_ERR)
    assert code in (0, NO_DEVICE), (code, msg)


def test_without_the_option_the_refusal_is_unchanged():
    code, msg = _create(S.dense_error_problem(65, 3, rank=16, nerr=1))
    assert code == UNSUPPORTED, (code, msg)
    assert "ndim > GRAPE_MAX_DENSE_DIM: error sources are served up to GRAPE_MAX_DENSE_DIM levels" in msg


def test_with_the_option_the_rest_is_still_refused_on_the_host():
    from robustgrape_amd.operators import FN_LINEAR, OPT_GENERAL_H0, OPT_TILED_ERR, VAR_XADD, Term
    from tests import problems as P
    fp = S.dense_error_problem(65, 3, rank=16, nerr=1)
    xadd = S.dense_error_problem(65, 3, rank=16, nerr=1, phase=True)  # (one additional parameter)
    full = np.full((65, 65), 0.01) + np.diag([1.0] * 16 + [0.0] * 49)  # a full, non-diagonal projector
    cases = {
        "x_add": (_with_errors(xadd, [_source([Term(S._hermitian(65, 70), var=VAR_XADD, index=0, func=FN_LINEAR)])]),
                  OPT_TILED_ERR),
        "Hermitian": (_with_errors(fp, [_source([Term(np.triu(np.ones((65, 65), complex)))])]), OPT_TILED_ERR),
        "projector": (fp.replace(projector=full), OPT_TILED_ERR),
        "GRAPE_OPT_GENERAL_H0": (fp, OPT_TILED_ERR | OPT_GENERAL_H0),
        "closures": (P.as_closures(fp), OPT_TILED_ERR),
        "ndim > GRAPE_MAX_TILED_DIM": (S.dense_error_problem(129, 2, rank=16, nerr=1), OPT_TILED_ERR),
    }
    for needle, (prob, opts) in cases.items():
        code, msg = _create(prob, options=opts)
        assert code == UNSUPPORTED and needle in msg, (needle, code, msg)


def test_the_header_defines_the_option_and_keeps_the_abi():
    from robustgrape_amd import _capi
    from robustgrape_amd.operators import OPT_TILED_ERR
    hdr = open(os.path.join(ROOT, "include", "grape.h")).read()
    assert int(re.search(r"#define GRAPE_OPT_TILED_ERR (\d+)", hdr).group(1)) == 262144 == OPT_TILED_ERR
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 12 == _capi.ABI_VERSION
    assert _capi.lib().grape_abi_version() == 12
    jl = open(os.path.join(ROOT, "julia", "RobustGRAPEMI355X.jl")).read()
    assert re.search(r"const GRAPE_OPT_TILED_ERR = Int32\(262144\)", jl)
