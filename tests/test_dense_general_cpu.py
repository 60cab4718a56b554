"""CPU-side checks of the general dense path's boundary: ABI 12 and its new symbol agree between
the header, the Python binding and the Julia shim, and GrapePlan's general_fallback retries a
refused creation only where it should (a stub library stands in for the device)."""
import os
import re

import numpy as np
import pytest

from robustgrape_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_12_and_the_general_exponential_are_declared_everywhere():
    from robustgrape_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "grape.h")).read()
    jl = open(os.path.join(ROOT, "julia", "RobustGRAPEMI355X.jl")).read()
    assert int(re.search(r"#define GRAPE_ABI_VERSION (\d+)", hdr).group(1)) == 12
    assert _capi.ABI_VERSION == 12
    assert int(re.search(r"const GRAPE_ABI_VERSION = (\d+)", jl).group(1)) == 12
    assert re.search(r"\bint grape_expm_batch_general\(int device, int ndim, int n, const double \*A, double \*E, "
                     r"int \*stats\);", hdr)
    assert "grape_expm_batch_general" in _capi.EXPORTED


class _StubLib:
    """grape_plan_create refuses (UNSUPPORTED) unless the descriptor carries OPT_GENERAL_H0."""

    def __init__(self):
        self.created, self.destroyed = [], 0

    def grape_plan_create(self, desc_ref, device, handle_ref):
        from robustgrape_amd.operators import OPT_GENERAL_H0
        opts = int(desc_ref._obj.reserved[1])
        self.created.append(opts)
        if not opts & OPT_GENERAL_H0:
            return -2
        handle_ref._obj.value = 0x1000 + len(self.created)
        return 0

    def grape_plan_destroy(self, handle):
        self.destroyed += 1

    def grape_last_error(self):
        return b"stub: refused"


@pytest.fixture
def stub(monkeypatch):
    from robustgrape_amd import _capi
    lib = _StubLib()
    monkeypatch.setattr(_capi, "lib", lambda: lib)
    return lib


def test_refused_creation_is_retried_only_above_12_levels_and_only_when_asked(stub):
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    fp = S.dense_problem(16, 3)
    with pytest.raises(_capi.GrapeError, match="UNSUPPORTED"):  # the default: the refusal stands
        GrapePlan(fp, nparam=2)
    assert stub.created == [0]
    plan = GrapePlan(fp, nparam=2, general_fallback=True)  # asked: once more, with the option
    assert stub.created == [0, 0, OPT_GENERAL_H0] and plan.options & OPT_GENERAL_H0
    plan.close()
    small = S.dense_problem(8, 3, rank=4)  # 12 levels or fewer: the C side decides by itself
    with pytest.raises(_capi.GrapeError, match="UNSUPPORTED"):
        GrapePlan(small, nparam=2, general_fallback=True)
    assert stub.created[3:] == [0]


def test_get_plan_asks_for_the_fallback(stub):
    from robustgrape_amd import engine
    from robustgrape_amd.operators import OPT_GENERAL_H0
    fp = S.dense_problem(16, 3)
    try:
        plan = engine.get_plan(fp, 2)
        assert plan.options & OPT_GENERAL_H0 and plan.general_fallback
        assert not getattr(engine._plan_defaults, "general_fallback", False)  # the request does not leak
    finally:
        engine.clear_plans()


def test_closure_tables_above_12_levels_recreate_the_plan_only_when_asked(stub, monkeypatch):
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_GENERAL_H0
    from tests import problems as P
    stub.grape_plan_create = lambda d, dev, h: (stub.created.append(int(d._obj.reserved[1])), h._obj.__setattr__(
        "value", 0x2000 + len(stub.created)), 0)[2]  # host-table plans are accepted as they are
    fpc = P.as_closures(S.dense_problem(16, 3))
    herm = np.eye(16, dtype=complex)[None]
    bad = herm - 0.2j * np.diag([0.0] * 15 + [1.0])[None]
    plan = GrapePlan(fpc, nparam=2, max_batch=1)
    plan.general_h0_for(herm)
    assert stub.created == [0]
    with pytest.raises(ValueError, match="Hermitian"):  # the default: refused as before
        plan.general_h0_for(bad)
    plan.close()
    plan = GrapePlan(fpc, nparam=2, max_batch=1, general_fallback=True)
    plan.general_h0_for(herm)
    assert stub.created == [0, 0]
    plan.general_h0_for(bad)  # recreated with the option, no exception
    assert stub.created == [0, 0, OPT_GENERAL_H0] and plan.options & OPT_GENERAL_H0 and stub.destroyed == 2
    plan.general_h0_for(bad)  # already general: nothing more
    assert stub.created == [0, 0, OPT_GENERAL_H0]
    plan.close()
    forced = GrapePlan(fpc, nparam=2, max_batch=1, options=OPT_GENERAL_H0)  # the caller's option: any table
    forced.general_h0_for(bad)
    assert stub.created[3:] == [OPT_GENERAL_H0]
    forced.close()
