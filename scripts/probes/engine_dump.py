#!/usr/bin/env python3
"""Outputs of the dense engine (grape_dense.hip, 13-64 levels) and the tiled engine (grape_tiled.hip, 65-128
levels) on a fixed list of problems, for a bit-for-bit comparison of two builds.

    python scripts/probes/engine_dump.py OUT.npz [--root TREE]     evaluate with TREE's in-tree library, save
    python scripts/probes/engine_dump.py --compare A.npz B.npz     numpy.array_equal of every array

The problems are those of the tests named beside them, at the smallest shapes that reach every kernel of the two
units; every plan case gives its four outputs in a batch of 1 and of 3 evaluations (row 1 is the test's x, rows 2
and 3 take their controls from dense_x with seeds 1 and 2, as the batch-equals-single tests of these files draw theirs):
  * tests/test_gpu_dense.py: no error sources at (d, N_t) = (13, 1), (24, 17), (64, 5); H0 reading x_add at
    (16, 7) (k_dgrad's x_add variants, k_dadd); error sources at (16, 5, 2, phase) and (13, 1, 1); H0 and Herror
    reading x_add with error sources at (16, 6, 2) (k_dadd's second use);
  * a general projector at d = 13 (scripts/probes/head_dump.py) and the decay problem (16, 5, 2, phase) of
    tests/test_gpu_dense_general.py (k_dexp<true>);
  * tests/test_gpu_tiled.py at d = 65 (N_t = 3, x_add target) and d = 128 (N_t = 3); tests/test_gpu_tiled_err.py
    at (65, 1, 1), (65, 5, 2, phase) (na > 0: the target rows) and the 81-level case of tests/golden/tiled_err.npz;
  * grape_expm_batch at d = 16 (plain and general) and d = 80 on the matrices of the exponential tests;
  * a two-slice time-sharded evaluation at d = 16 (tests/test_gpu_timeshard.py: k_img_cols, k_cols_img), the
    closure fallback at d = 13 (tests/test_gpu_dense_tables.py: k_tab_images) and the unitary-derivative table of
    tests/test_gpu_dense.py test_dense_unitary_derivatives_match_oracle at (13, 3, no error sources) (k_img_rows).
Which kernels ran is read from a kernel trace of this script, not from here.  --root lets one file serve two
checkouts.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from head_dump import compare, dense_projector  # noqa: E402


def _rows(x, more):
    """the test's x, then two more rows: other controls, the test's x_add"""
    return np.stack([x] + [np.concatenate([m, x[len(m):]]) for m in more])


def plan_cases():
    """(label, problem, X of three rows, plan options)"""
    from robustgrape_amd import synthetic as S
    from robustgrape_amd.operators import OPT_GENERAL_H0, OPT_TILED_ERR
    from tests import test_gpu_dense as TD
    from tests import test_gpu_dense_general as TG
    from tests import test_gpu_dense_tables as TT
    from tests import test_gpu_tiled as TL
    from tests import test_gpu_tiled_err as TE
    out = []

    def add(label, fp, x, nt, opts=0):
        out.append((label, fp, _rows(x, [S.dense_x(nt, seed=s) for s in (1, 2)]), opts))

    for d, nt, scale in ((13, 1, 1.0), (24, 17, 0.3), (64, 5, 1.0)):
        add(f"dense-d{d}-nt{nt}", S.dense_problem(d, nt, rank=min(16, d - 3), scale=scale),
            S.dense_x(nt, seed=300 + nt), nt)
    add("dense-xadd-d16-nt7", TD._xadd_h0_problem(16, 7), np.concatenate([S.dense_x(7, seed=507), [0.7, -0.3]]), 7)
    for d, nt, nerr, phase in ((16, 5, 2, True), (13, 1, 1, False)):
        x = S.dense_x(nt, seed=400 + nt)
        add(f"dense-err-d{d}-nt{nt}-ne{nerr}", S.dense_error_problem(d, nt, rank=min(16, d - 3), nerr=nerr, phase=phase),
            np.concatenate([x, [0.7]]) if phase else x, nt)
    add("dense-xadd-err-d16-nt6", TD._xadd_err_problem(16, 6, 2),
        np.concatenate([S.dense_x(6, seed=906), [0.7, -0.3]]), 6)
    add("dense-projector-d13", S.dense_problem(13, 4, rank=10).replace(projector=dense_projector(13, 6, 43)),
        S.dense_x(4, seed=504), 4)
    add("dense-general-d16", TG._decay(16, 5, 2, True, 1.0, True), TG._x(5, True, 805), 5, OPT_GENERAL_H0)
    fp = TT._fp(13, 5, 0, True)
    add("dense-closures-d13", fp, TT._x(fp, 900), 5)
    for d in (65, 128):
        fp, x = TL._problem(d, 3, 1.0, d == 65)
        add(f"tiled-d{d}-nt3", fp, x, 3)
    for d, nt, nerr, phase in ((65, 1, 1, False), (65, 5, 2, True)):
        fp, x = TE._problem(d, nt, nerr, phase)
        add(f"tiled-err-d{d}-nt{nt}-ne{nerr}", fp, x, nt, OPT_TILED_ERR)
    g = TE._golden()
    d, nt, nerr, phase = (int(v) for v in g["cases"][0])
    fp, x = TE._problem(d, nt, nerr, bool(phase), float(g["scales"][0]))
    add(f"tiled-err-golden-d{d}-nt{nt}", fp, x, nt, OPT_TILED_ERR)
    return out


def other_entry_points(arrays):
    from robustgrape_amd import calculate_unitary_and_derivatives
    from robustgrape_amd import synthetic as S
    from robustgrape_amd.timeshard import time_sharded_fidelity_grad
    from tests import test_gpu_dense as TD
    from tests import test_gpu_dense_general as TG
    norms = (0.04, 0.6, 1.5, 4.0, 30.0)
    for d, general in ((16, False), (16, True), (80, False)):
        rng = np.random.default_rng(1000 + d)
        A = np.stack([TG._family("ginibre", d, nm, rng) if general else TD._skew_hermitian(d, nm, rng) for nm in norms])
        E, stats = TG._expm(A, general=general)
        arrays[f"expm-d{d}-{'general' if general else 'plain'}/E"] = np.ascontiguousarray(E)
        arrays[f"expm-d{d}-{'general' if general else 'plain'}/stats"] = np.asarray(stats)
        print(f"expm d={d} general={general} stats={stats}")
    fp, x = S.dense_problem(d=16, ntimes=48, dt=0.3, rank=6), S.dense_x(ntimes=48, seed=5)
    F, Fdx = time_sharded_fidelity_grad(fp, x, nparam=2, nslices=2)
    arrays["timeshard-d16-s2/F"], arrays["timeshard-d16-s2/F_dx"] = np.asarray(F), np.asarray(Fdx)
    print(f"timeshard d=16 two slices F={float(F):.17g}")
    d, nt = 13, 3  # test_dense_unitary_derivatives_match_oracle's first case: rank min(16, d - 3), seed 600 + nt
    got = calculate_unitary_and_derivatives(S.dense_problem(d, nt, rank=min(16, d - 3)).unitary_problem,
                                            S.dense_x(nt, seed=600 + nt))
    for name, a in zip(("U", "U_dx", "U_dx_add", "U_derr", "U_derr_dx", "U_derr_dx_add"), got):
        arrays[f"unitary-table-d13/{name}"] = np.asarray(a)
    print(f"unitary table d=13 |U_dx| = {np.max(np.abs(got[1])):.17g}")


def dump(path):
    from robustgrape_amd import build
    from robustgrape_amd.engine import GrapePlan
    arrays = {}
    for label, fp, X, opts in plan_cases():
        for nb in (1, 3):
            pl = GrapePlan(fp, nparam=2, device=0, max_batch=nb, options=opts)  # a refusal ends the dump
            try:
                res = pl.fidelity_grad(X[:nb])
            finally:
                pl.close()
            for key, a in zip(("F", "F_dx", "F_d2err", "F_d2err_dx"), res):
                arrays[f"{label}/b{nb}/{key}"] = np.asarray(a)
            print(f"{label} nb={nb} F={np.asarray(res[0]).ravel()[0]:.17g}", flush=True)
    other_entry_points(arrays)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path} (library build id {build.source_id()})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="+")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.paths))
    sys.path.insert(0, os.path.abspath(args.root))
    dump(args.paths[0])
