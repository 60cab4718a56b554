#!/usr/bin/env python3
"""Outputs of the projector heads (grape_projector.hip) on a fixed list of problems, for a bit-for-bit
comparison of two builds.

    python scripts/probes/head_dump.py OUT.npz [--root TREE]     evaluate with TREE's in-tree library, save
    python scripts/probes/head_dump.py --compare A.npz B.npz     numpy.array_equal of every array

The list holds the smallest shapes that reach every branch of the four general heads, each in a batch of 1
and of 3 evaluations:
  * tests/test_gpu_projector.py: d = 5, N_t = 13, sparse and dense projector, 0 and 2 error sources; the
    x_add-dependent problems (d = 5 and 9, operator basis and closures: the U0tab path, the x_add target
    parts); the dense engine (images) at d = 13 (0 and 2 error sources) and d = 16 (2 error sources);
  * the three general-projector problems of tests/test_gpu_sectors.py (the last with both sector layouts);
  * the six diagonal problems of tests/test_gpu_walk.py::test_diagonal_head_matches_general_head with
    GRAPE_OPT_GENERAL_HEAD (two sector classes, fixed levels, padding slots), and with their own
    diagonal heads (k_sec_head_diag, k_sec_err_head_rows).
Every small-engine problem runs with options 0 (sector heads k_sec_head / k_sec_err_head where the problem
has sectors) and with GRAPE_OPT_NO_SECTORS (k_proj_fid / k_proj_err).  Which kernels ran is read from a
kernel trace of this script, not from here.  --root lets one file serve two checkouts.
"""
import argparse
import os
import sys

import numpy as np


def sparse_projector(W, seed):  # tests/test_gpu_projector.py
    rng = np.random.default_rng(seed)
    P0 = np.array(W, dtype=np.float64)
    d = P0.shape[0]
    for _ in range(3):
        i, j = rng.integers(0, d, 2)
        if i != j:
            P0[i, j] = rng.uniform(-0.5, 0.5)
    return P0


def dense_projector(d, rank, seed):
    Qm, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((d, rank)))
    return Qm @ Qm.T


def cases():
    """(label, problem, X of three rows, tuple of plan options)"""
    from robustgrape_amd import synthetic as S
    from robustgrape_amd.operators import OPT_GENERAL_HEAD, OPT_NO_SECTORS, OPT_NO_SYMMETRY
    from tests import problems as P
    both = (0, OPT_NO_SECTORS)
    out = []
    for kind in ("sparse", "dense"):
        for nerr in (0, 2):
            P0 = sparse_projector(P.W_SYM, 3) if kind == "sparse" else dense_projector(5, 2, 4)
            fp = P.sym_problem(13, errors=("amp", "freq")[:nerr]).replace(projector=P0)
            out.append((f"sym5-{kind}-ne{nerr}", fp, np.stack([P.random_x(13, 11 + s) for s in range(3)]), both))
    for device in (True, False):
        for d, nt in ((5, 9), (9, 7)):
            P0 = dense_projector(d, 3, 20 + d) + sparse_projector(np.zeros((d, d)), 21)
            fp = P.xadd_err_problem(d, nt, device=device).replace(projector=P0)
            X = np.stack([P.xadd_x(nt, 60 + nt + s) for s in range(3)])
            out.append((f"xadd-d{d}-{'ob' if device else 'closures'}", fp, X, both))
    for d, ntimes, nerr, phase in ((13, 4, 0, False), (13, 4, 2, False), (16, 5, 2, True)):
        fp = (S.dense_error_problem(d, ntimes, rank=min(16, d - 3), nerr=nerr, phase=phase) if nerr
              else S.dense_problem(d, ntimes, rank=min(16, d - 3)))
        X = np.stack([S.dense_x(ntimes, seed=500 + ntimes + s) for s in range(3)])
        if phase:
            X = np.concatenate([X, np.full((3, 1), 0.7)], axis=1)
        out.append((f"dense-d{d}-ne{nerr}", fp.replace(projector=dense_projector(d, 6, 30 + d)), X, (0,)))
    for d in (5, 9):  # tests/test_gpu_sectors.py
        Qm, _ = np.linalg.qr(np.random.default_rng(d).standard_normal((d, 3)))
        fp = P.xadd_err_problem(d, 12, nerr=2).replace(projector=Qm @ Qm.T)
        out.append((f"sectors-xadd-d{d}", fp, np.stack([P.xadd_x(12, 400 + s) for s in range(3)]), both))
    Qm, _ = np.linalg.qr(np.random.default_rng(9).standard_normal((9, 3)))
    fp = P.full9_problem(20).replace(projector=Qm @ Qm.T)
    out.append(("sectors-full9-mixing", fp, np.stack([P.random_x(20, 90 + s) for s in range(3)]),
                (0, OPT_NO_SYMMETRY, OPT_NO_SECTORS)))
    for name, fp in (("full9", P.full9_problem(64)), ("sym5", P.sym_problem(40)), ("fullblk7", P.fullblk_problem(40)),
                     ("c3", P.full9_problem(40, nerr=4)), ("sym5-amp-freq", P.sym_problem(30, errors=("amp", "freq"))),
                     ("fullblk7-amp", P.fullblk_problem(30, errors=("amp",)))):
        nt = fp.unitary_problem.ntimes
        X = np.stack([P.random_x(nt, 4000 + s, small=(s % 2 == 0)) for s in range(3)])
        out.append((f"diag-{name}", fp, X, (OPT_GENERAL_HEAD, 0)))
    return out


def dump(path):
    from robustgrape_amd import build
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.types import split_x
    arrays = {}
    for label, fp, X, options in cases():
        nparam = split_x(fp.unitary_problem, X[0])[2]
        for opts in options:
            for nb in (1, 3):
                try:
                    pl = GrapePlan(fp, nparam=nparam, device=0, max_batch=nb, options=opts)
                except Exception as exc:  # a problem this build does not serve: recorded, compared as such
                    print(f"{label} opts={opts:#x} nb={nb}: no plan ({exc})")
                    arrays[f"{label}/o{opts:x}/b{nb}/noplan"] = np.zeros(1)
                    continue
                try:
                    res = pl.fidelity_grad(X[:nb])
                    sec = pl.sectors()
                finally:
                    pl.close()
                for key, a in zip(("F", "F_dx", "F_d2err", "F_d2err_dx"), res):
                    arrays[f"{label}/o{opts:x}/b{nb}/{key}"] = np.asarray(a)
                print(f"{label} opts={opts:#x} nb={nb} sectors={sec} F={np.asarray(res[0]).ravel()[0]:.17g}")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **arrays)
    print(f"{len(arrays)} arrays -> {path} (library build id {build.source_id()})")


def compare(a, b):
    A, B = np.load(a), np.load(b)
    bad = sorted(set(A.files) ^ set(B.files))
    for k in sorted(set(A.files) & set(B.files)):
        if not (A[k].shape == B[k].shape and np.array_equal(A[k], B[k])):
            bad.append(k)
            print(f"DIFFERS {k}: max |a - b| = {np.max(np.abs(A[k] - B[k])) if A[k].shape == B[k].shape else 'shape'}")
    n = len(set(A.files) & set(B.files))
    nonempty = sum(A[k].size > 0 for k in A.files)
    print(f"{a} vs {b}: {n} arrays in common ({nonempty} non-empty), {len(bad)} differ or are missing"
          + ("" if bad else ": numpy.array_equal is True for every array"))
    return 1 if bad else 0


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
