"""Probe: what the product-coefficient path (include/grape.h GRAPE_OP_FACTOR, csrc/grape_prod.hpp) costs.

Three rates in one call, all at d = 9, N_t = 512 (bench.py's C2 model), written to
profiles/prod/prod_probe.json:

  product   the amplitude x phase problem (two controls per step), 4 096 device-resident evaluations per
            call through the stored pipeline with k_expm_prod / k_expm_grad_prod;
  closures  the same problem as plain closures (the host-table fallback it would otherwise take), host arrays;
  forced    the phase-only C2 problem (one control per step) forced onto the same stored pipeline
            (OPT_NO_WALK | OPT_NO_LANE | OPT_NO_CHAIN | OPT_NO_GAUGE): the yardstick for the builder's overhead.
            The product problem runs two eps-variants per step where this one runs one, so its
            k_expm_grad items double; the per-item figures below are the like-for-like comparison.

Then one profiled call of the product plan and of the forced plan (set_profiling / kernel_times): where
the time goes.  The outputs of the product plan are checked against the closure plan's on eight rows.

    python scripts/probes/prod_probe.py [--evals 4096] [--calls 300] [--out profiles/prod/prod_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from robustgrape_amd import rydberg as R  # noqa: E402
from robustgrape_amd.engine import GrapePlan  # noqa: E402
from robustgrape_amd.operators import OPT_NO_CHAIN, OPT_NO_GAUGE, OPT_NO_LANE, OPT_NO_WALK  # noqa: E402
from robustgrape_amd.types import FidelityRobustGRAPEProblem, UnitaryRobustGRAPEProblem  # noqa: E402

FORCED = OPT_NO_WALK | OPT_NO_LANE | OPT_NO_CHAIN | OPT_NO_GAUGE


def product_problem(device=True):
    """bench.problem() with both Rabi frequencies scaled by a second control: Omega_k (cos phi_k Hc + sin phi_k Hs)."""
    if device:
        H0 = R.rydberg_full_operator_basis(1.0, 1.0, 0.0, 0.0, 10.0, param=1, amplitude_param=0)
        target = R.cz_full_target()
    else:
        H0 = lambda t, p, xa: R.rydberg_hamiltonian_full(p[1], p[0], p[0], 0.0, 0.0, 10.0)  # noqa: E731
        target = lambda xa: R.cz_with_1q_phase_full(xa[0])  # noqa: E731
    up = UnitaryRobustGRAPEProblem(t0=bench.T0, ntimes=bench.NT, ndim=bench.D, H0=H0, nb_additional_param=1)
    return FidelityRobustGRAPEProblem(up, np.diag([1.0] * 4 + [0.0] * 5), target)


def product_inputs(count, seed=0):
    """Amplitudes 0.5 + U[0, 1), phases 2 pi U, theta 2 pi U; x[p + 2 k] = control p at step k."""
    rng = np.random.default_rng(seed)
    xm = np.empty((count, bench.NT, 2))
    xm[..., 0] = 0.5 + rng.uniform(size=(count, bench.NT))
    xm[..., 1] = 2 * np.pi * rng.uniform(size=(count, bench.NT))
    return np.concatenate([xm.reshape(count, -1), 2 * np.pi * rng.uniform(size=(count, 1))], axis=1)


def device_rate(fp, nparam, X, calls, options=0):
    """evals/s of `calls` device-resident calls (after two warm-up calls), the kernel times of one more
    profiled call, and the first eight rows of the outputs."""
    dev = torch.device("cuda:0")
    B = len(X)
    plan = GrapePlan(fp, nparam=nparam, device=0, max_batch=B, options=options)
    try:
        Xd = torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        F = torch.empty(B, dtype=torch.float64, device=dev)
        G = torch.empty(B, X.shape[1], dtype=torch.float64, device=dev)
        call = lambda: plan.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), G.data_ptr(), B)  # noqa: E731
        for _ in range(2):
            call()
        plan.synchronize()
        t = time.perf_counter()
        for _ in range(calls):
            call()
        plan.synchronize()
        dt = time.perf_counter() - t
        plan.set_profiling(True)
        call()
        plan.synchronize()
        kt = {k: {"ms": v[0], "launches": v[1]} for k, v in plan.kernel_times(reset=True).items() if v[1]}
        plan.set_profiling(False)
        return {"evals_per_s": calls * B / dt, "ms_per_call": dt / calls * 1e3, "evals_per_call": B, "calls": calls,
                "sectors": plan.sectors(), "kernel_ms_one_call": kt}, F[:8].cpu().numpy(), G[:8].cpu().numpy()
    finally:
        plan.close()


def closure_rate(fp, X, chunk=128):
    plan = GrapePlan(fp, nparam=2, device=0, max_batch=chunk)
    try:
        plan.fidelity_grad(X[:chunk])  # warm-up (starts the table workers)
        t = time.perf_counter()
        F, G, _, _ = plan.fidelity_grad(X)
        dt = time.perf_counter() - t
        return {"evals_per_s": len(X) / dt, "evals": len(X), "evals_per_chunk": chunk, "seconds": dt}, F[:8], G[:8]
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--evals", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=300)  # about half a second per timed window
    ap.add_argument("--closure-evals", type=int, default=2048)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prod", "prod_probe.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    Xp = product_inputs(args.evals)
    prod, Fp, Gp = device_rate(product_problem(), 2, Xp, args.calls)
    print("product", json.dumps(prod), flush=True)
    forced, _, _ = device_rate(bench.problem(), 1, bench.restart_inputs(0, args.evals), args.calls, FORCED)
    print("forced phase-only", json.dumps(forced), flush=True)
    clo, Fc, Gc = closure_rate(product_problem(device=False), Xp[:args.closure_evals])
    print("closures", json.dumps(clo), flush=True)
    agree = {"F": float(np.max(np.abs(Fp - Fc))), "F_dx": float(np.max(np.abs(Gp - Gc))),
             "F_dx_scale": float(np.max(np.abs(Gc)))}
    nt = bench.NT
    per_item = {  # ns per (evaluation, step, variant) item of the two kernels that build generators
        "product": {"k_expm": prod["kernel_ms_one_call"]["k_expm"]["ms"] * 1e6 / (args.evals * nt),
                    "k_expm_grad": prod["kernel_ms_one_call"]["k_expm_grad"]["ms"] * 1e6 / (args.evals * nt * 2)},
        "forced": {"k_expm": forced["kernel_ms_one_call"]["k_expm"]["ms"] * 1e6 / (args.evals * nt),
                   "k_expm_grad": forced["kernel_ms_one_call"]["k_expm_grad"]["ms"] * 1e6 / (args.evals * nt)}}
    out = {"problem": "Rydberg CZ d=9 N_t=512 (bench.py C2 model)", "product": prod, "forced_phase_only": forced,
           "closures": clo, "product_over_closures": prod["evals_per_s"] / clo["evals_per_s"],
           "product_over_forced": prod["evals_per_s"] / forced["evals_per_s"],
           "ns_per_item_all_sectors": per_item, "product_vs_closure_plan_first_8_rows": agree,
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: out[k] for k in ("product_over_closures", "product_over_forced", "ns_per_item_all_sectors",
                                          "product_vs_closure_plan_first_8_rows")}), flush=True)


if __name__ == "__main__":
    main()
