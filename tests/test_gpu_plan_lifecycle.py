"""Plan lifecycle on every route of plan construction: a small plan is created, evaluates one batch of two
x and the unitary derivatives of one (so that the lazily allocated single-evaluation workspace exists when
the plan releases its device memory), is closed, and is created and evaluated again.  The second results equal
the first bit for bit, and both agree with the oracle at the tolerance of the route's own parity test (the
helpers are imported from those tests).  N_t = 8, max_batch = 2.

x: tests.problems.random_x for the Rydberg problems it was written for (one control per step and the
target's phase).  The dense family has two amplitude controls per step and no additional parameter, and its
parity test's fixed tier (tests/test_gpu_dense.py: no step-norm scaling) holds for the family's own
robustgrape_amd.synthetic.dense_x in [-1, 1) -- with random_x's [0, 2 pi) the steps reach squaring and F_dx
measured 1.0e-8 from the exact forward difference against that tier's 2.0e-9, on unchanged kernels -- so
those two problems take dense_x.  The x_add problem has two additional parameters: its own xadd_x.

One more case covers a creation that is refused after device allocation has begun (the plan's stream and
status word exist): the code and message are the engine's, and a valid creation on the same device
afterwards succeeds and evaluates correctly."""
import numpy as np
import pytest

from robustgrape_amd import synthetic as S
from tests import problems as P

pytestmark = pytest.mark.gpu
NT = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _rydberg_check(fp, label):  # tests/test_gpu_parity.py: F_dx at fd_tier, the error outputs at T3
    from tests import test_gpu_parity as T

    def check(got, ref, x):
        T._assert_fid(got[0], got[1], ref[0], ref[1], P.fd_tier(fp, x), test=label)
        if len(fp.unitary_problem.error_sources):
            T._assert_err(fp, got[2], got[3], ref[2], ref[3], test=label, x=x)
    return check


def _x(seed):
    return np.stack([P.random_x(NT, seed + s) for s in range(2)])


def _dense_x(seed):
    return np.stack([S.dense_x(NT, seed=seed + s) for s in range(2)])


def _full9(nerr=0, options=0):
    fp = P.full9_problem(NT, nerr=nerr)
    return dict(fp=fp, fpo=P.full9_problem(NT, nerr=nerr, device=False), options=options, X=_x(900),
                check=_rydberg_check(fp, f"lifecycle_full9_ne{nerr}_opt{options}"))


def _no_sectors():
    from robustgrape_amd.operators import OPT_NO_SECTORS
    return _full9(options=OPT_NO_SECTORS)


def _sym_amp():
    fp = P.sym_problem(NT, errors=("amp",))
    return dict(fp=fp, fpo=P.sym_problem(NT, errors=("amp",), device=False), X=_x(910),
                check=_rydberg_check(fp, "lifecycle_sym_amp"))


def _xadd():
    from tests import test_gpu_xadd_err as T
    X = np.stack([P.xadd_x(NT, 920 + s) for s in range(2)])
    return dict(fp=P.xadd_err_problem(5, NT), fpo=P.xadd_err_problem(5, NT, device=False), X=X,
                check=lambda got, ref, x: T._check(got, ref, "lifecycle_xadd"))


def _decay():
    from tests import test_gpu_general_h0 as T
    fpo = P.with_decay(P.sym_problem(NT, device=False), device=False)
    return dict(fp=P.with_decay(P.sym_problem(NT)), fpo=fpo, X=_x(930),
                check=lambda got, ref, x: T._check(got, ref, "lifecycle_decay", 0, P.fd_tier(fpo, x)))


def _closures():
    from tests import test_gpu_tables as T
    fp = P.as_closures(P.sym_problem(NT))
    return dict(fp=fp, fpo=P.sym_problem(NT, device=False), X=_x(940),
                check=lambda got, ref, x: T._assert_fid(got[0], got[1], ref[0], ref[1]))


def _dense():  # tests/test_gpu_dense.py test_dense_fidelity_gradient_matches_live_oracle at d = 16
    from oracle import grape_exact as E
    from tests import test_gpu_dense as T
    fp = S.dense_problem(16, NT, rank=13, scale=1.0)
    return dict(fp=fp, fpo=fp, nparam=2, X=_dense_x(950),
                check=lambda got, ref, x: T._assert_fid(got[0], got[1], ref[0], ref[1], "lifecycle_dense",
                                                        E.fidelity_and_gradient(fp, x, nparam=2)))


def _pivot():  # tests/test_gpu_dense_general.py CASES[0]: d = 13, decay on three levels
    from robustgrape_amd.operators import OPT_GENERAL_H0
    from tests import test_gpu_dense_general as T
    fpo = T._decay(13, NT, 0, False, 2.0, False)
    return dict(fp=T._decay(13, NT, 0, False, 2.0, True), fpo=fpo, nparam=2, options=OPT_GENERAL_H0,
                X=_dense_x(960),
                check=lambda got, ref, x: T._check(got, ref, "lifecycle_pivot", 0, fpo, x, T._spread(fpo, x, ref[1])))


def _projector():  # tests/test_gpu_projector.py test_small_d_operator_basis, the dense projector
    from tests import test_gpu_projector as T
    P0 = T.dense_projector(5, 2, 4)
    return dict(fp=P.sym_problem(NT).replace(projector=P0), fpo=P.sym_problem(NT, device=False).replace(projector=P0),
                X=_x(970), check=lambda got, ref, x: T._cmp(got, ref, "lifecycle_projector", errors=False))


ROUTES = {"merged_gauge_eval1": _full9, "whole_matrix": _no_sectors, "error_walks": lambda: _full9(nerr=4),
          "sym_amp": _sym_amp, "xadd_err": _xadd, "general_h0": _decay, "tables": _closures, "dense": _dense,
          "pivot": _pivot, "general_projector": _projector}


def _run(r):
    """One plan's life: create, evaluate the batch, the unitary derivatives of its first x, close."""
    from robustgrape_amd.engine import GrapePlan
    plan = GrapePlan(r["fp"], nparam=r.get("nparam", 1), max_batch=2, options=r.get("options", 0))
    try:
        out = plan.fidelity_grad(r["X"])
        plan.unitary_derivs(r["X"][0])
    finally:
        plan.close()
    return out


@pytest.mark.parametrize("route", list(ROUTES))
def test_create_evaluate_close_and_again(route):
    from oracle import grape_oracle as O
    r = ROUTES[route]()
    refs = [O.calculate_fidelity_and_derivatives(r["fpo"], x) for x in r["X"]]
    first, second = _run(r), _run(r)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    for out in (first, second):
        for b, x in enumerate(r["X"]):
            r["check"](tuple(o[b] for o in out), refs[b], x)


def test_refused_creation_frees_and_the_device_serves_the_next_plan():
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OperatorBasisError, Term
    from robustgrape_amd.types import ErrorSource
    fp0 = S.dense_problem(16, NT, rank=13)
    decay = np.diag([0.0] * 15 + [1.0]).astype(complex)  # a decay-rate error: -i e/2 |r><r|
    errs = (ErrorSource(OperatorBasisError([Term(decay, scale=-0.5j)])),)
    bad = fp0.replace(unitary_problem=fp0.unitary_problem.replace(error_sources=errs))
    with pytest.raises(_capi.GrapeError) as info:
        GrapePlan(bad, nparam=2, max_batch=2)
    assert str(info.value) == ("GRAPE_ERR_UNSUPPORTED: error source (dense engine): scale * operator is not "
                               "Hermitian (non-unitary propagators are not supported)")
    from oracle import grape_oracle as O
    r = _dense()
    out = _run(r)
    for b, x in enumerate(r["X"]):
        r["check"](tuple(o[b] for o in out), O.calculate_fidelity_and_derivatives(r["fpo"], x), x)
