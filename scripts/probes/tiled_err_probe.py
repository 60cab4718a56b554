"""The tiled engine's error path (64 < d <= 128, GRAPE_OPT_TILED_ERR, DESIGN.md 7.3 "Error sources") measured
against the same engine without error sources, in one call.

    python scripts/probes/tiled_err_probe.py [--out DIR] [--ntimes N]

d = 128, np = 2 (the C5 family with error sources, robustgrape_amd/synthetic.py dense_error_problem), N_t = 1 024,
with ne = 0 and ne = 1 on plans of the same max_batch (1 and 2 device-resident evaluations per call: two is what
the byte budget holds at ne = 1, where the local-frame images of every step are stored): warm-up calls, then timed
calls -- a host clock around calls that end in a stream synchronise, HIP events beside it -- and, in passes of
their own with the plan's profiling on, the per-stage times of kernel_times.  The yardstick is the ratio of the
ne = 1 figure to the ne = 0 figure of the same call; the work ratio follows from the counts per step that the
output states (exponentials and products).
Prints one JSON object; --out DIR also writes it to DIR/tiled_err_probe.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

D, NP = 128, 2
STAGES = ("k_dexp", "k_dscan", "k_dcarry", "k_dmc", "k_dgrad", "k_grad/k_err_local", "k_err_scan", "k_err_grad")


def measure(nt, ne, nb, warm, reps):
    import torch

    from robustgrape_amd import _capi
    from robustgrape_amd import synthetic as S
    from robustgrape_amd.engine import GrapePlan
    from robustgrape_amd.operators import OPT_TILED_ERR
    fp = S.dense_error_problem(D, nt, rank=16, nerr=ne)
    X = np.stack([S.dense_x(nt, seed=67 + b) for b in range(nb)])
    dev = torch.device("cuda", 0)
    Xd = torch.as_tensor(X, device=dev)
    F = torch.empty((nb,), dtype=torch.float64, device=dev)
    Fdx = torch.empty(X.shape, dtype=torch.float64, device=dev)
    d2 = torch.empty((nb, max(ne, 1)), dtype=torch.float64, device=dev)
    d2dx = torch.empty((nb, max(ne, 1), X.shape[1]), dtype=torch.float64, device=dev)
    plan = GrapePlan(fp, nparam=NP, max_batch=nb, options=OPT_TILED_ERR)
    side = torch.cuda.Stream(device=dev)
    plan.set_stream(side.cuda_stream)
    call = lambda: plan.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), Fdx.data_ptr(), nb,
                                                   d2.data_ptr() if ne else 0, d2dx.data_ptr() if ne else 0)
    names = [n for n in STAGES if n in _capi.KERNEL_NAMES]
    try:
        for _ in range(warm):
            call()
        plan.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(side)
        for _ in range(reps):
            call()
        e1.record(side)
        plan.synchronize()
        host_s = time.perf_counter() - t0
        ev_s = e0.elapsed_time(e1) * 1e-3
        plan.set_profiling(True)
        plan.kernel_times(reset=True)
        call()
        plan.synchronize()
        kt = plan.kernel_times(reset=True)
        plan.set_profiling(False)
        Fh = F.cpu().numpy()
        d2h = d2.cpu().numpy() if ne else np.zeros((nb, 0))
    finally:
        plan.close()
    return {"ne": ne, "evaluations_per_call": nb, "warmup_calls": warm, "timed_calls": reps,
            "s_per_call_host_clock": host_s / reps, "s_per_call_events": ev_s / reps,
            "evals_per_s": nb * reps / host_s, "F": [float(v) for v in Fh], "F_d2err": d2h.tolist(),
            "stage_ms_per_call": {k: kt[k][0] for k in names if kt[k][1]}}


def counts(ne):
    """Per step: variant exponentials, and pipeline products beside them."""
    if ne == 0:
        return {"exponentials": 1 + NP, "products": 1 + 2}  # the prefix, Y (two)
    nz = NP + ne + ne * NP
    return {"exponentials": 1 + 2 * NP + ne * (2 + NP), "products": 1 + 2 * nz + 2 * ne}  # prefix, images, walk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ntimes", type=int, default=1024)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tiled_err_probe.py needs a GPU: nothing is measured without one")
    out = {"probe": "tiled_err", "d": D, "ntimes": args.ntimes, "nparam": NP, "device": torch.cuda.get_device_name(0),
           "per_step": {"ne0": counts(0), "ne1": counts(1)}}
    for nb in (1, 2):
        a = measure(args.ntimes, 0, nb, warm=1, reps=3)
        b = measure(args.ntimes, 1, nb, warm=1, reps=3)
        out[f"nb{nb}"] = {"ne0": a, "ne1": b, "ratio_ne1_to_ne0": b["evals_per_s"] / a["evals_per_s"]}
    # an exponential at degree 16 without squarings is 6 products (3 powers, 3 Horner steps)
    w = [6 * c["exponentials"] + c["products"] for c in (counts(0), counts(1))]
    out["work_ratio_products"] = w[0] / w[1]
    print(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "tiled_err_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
