"""The tiled engine (64 < d <= 128) measured on its own: bench.py has no tiled workload.

    python scripts/probes/tiled_probe.py [--out DIR] [--no-c5]

1. d = 128, N_t = 1024, np = 2 (the C5 family, robustgrape_amd/synthetic.py) at 1 and at 8 device-resident
   evaluations per call: warm-up calls, then timed calls -- a host clock around calls that end in a stream
   synchronise, and HIP events on the plan's stream beside it -- and, in passes of their own with the plan's
   profiling on, the per-stage times of kernel_times (the dense slots k_dexp .. k_dgrad).
2. The product kernel alone at P = 128 over 1 024 items, credited 8 P^3 per product
   (scripts/probes/tiled_product_probe.hip, built beforehand; its header has the command).
3. The yardsticks on the same box in the same call: `python bench.py --workload c5` (evals/s and k_dexp's
   credited fraction of the FP64 peak) and the d^3 scaling of the C5 value (d = 128 costs 8 x C5 per
   evaluation at equal efficiency).
Prints one JSON object; --out DIR also writes it to DIR/tiled_probe.json.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

D, NT, NP = 128, 1024, 2
STAGES = ("k_dexp", "k_dscan", "k_dcarry", "k_dmc", "k_dgrad")


def clock_mhz():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        return [ln.strip() for ln in out.splitlines() if "sclk" in ln or "mclk" in ln][:4]
    except Exception as e:  # (the box's clock is a note beside the numbers, not a measurement)
        return [f"unavailable: {e}"]


def measure(nb, warm, reps):
    import torch

    from robustgrape_amd import synthetic as S
    from robustgrape_amd.engine import GrapePlan
    fp = S.dense_problem(D, NT, rank=16)
    X = np.stack([S.dense_x(NT, seed=67 + b) for b in range(nb)])
    dev = torch.device("cuda", 0)
    Xd = torch.as_tensor(X, device=dev)
    F = torch.empty((nb,), dtype=torch.float64, device=dev)
    Fdx = torch.empty(X.shape, dtype=torch.float64, device=dev)
    plan = GrapePlan(fp, nparam=NP, max_batch=nb)
    side = torch.cuda.Stream(device=dev)
    plan.set_stream(side.cuda_stream)
    call = lambda: plan.fidelity_grad_device_async(Xd.data_ptr(), F.data_ptr(), Fdx.data_ptr(), nb)
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
        for _ in range(2):
            call()
        plan.synchronize()
        kt = plan.kernel_times(reset=True)
        plan.set_profiling(False)
        Fh = F.cpu().numpy()
    finally:
        plan.close()
    return {"evaluations_per_call": nb, "warmup_calls": warm, "timed_calls": reps,
            "s_per_call_host_clock": host_s / reps, "s_per_call_events": ev_s / reps,
            "evals_per_s": nb * reps / host_s, "F": [float(v) for v in Fh],
            "stage_ms_per_call": {k: kt[k][0] / 2 for k in STAGES},
            "stage_launch_groups_per_call": {k: kt[k][1] // 2 for k in STAGES}}


def product_probe():
    exe = os.path.join(ROOT, "scripts", "probes", "tiled_product_probe")
    if not os.path.exists(exe):
        return {"error": "scripts/probes/tiled_product_probe is not built (see the header of its .hip)"}
    r = subprocess.run([exe, str(D), "1024", "20"], capture_output=True, text=True, timeout=300)
    rows = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    return {"rc": r.returncode, "rows": rows, "stderr": r.stderr[-400:]}


def c5_yardstick():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c5", "--steps", "3",
                        "--warmup", "1"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith("{"):
            j = json.loads(ln)
            return {"evals_per_s": j["value"], "k_dexp_frac": j.get("kernels_frac", {}).get("k_dexp"),
                    "kernels_frac": j.get("kernels_frac"), "whole_eval_frac": j["roofline"]["whole_eval"]["frac"]}
    return {"error": r.stderr[-400:], "rc": r.returncode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-c5", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("tiled_probe.py needs a GPU: nothing is measured without one")
    out = {"probe": "tiled", "d": D, "ntimes": NT, "nparam": NP, "device": torch.cuda.get_device_name(0),
           "clocks": clock_mhz()}
    out["one"] = measure(1, warm=2, reps=5)
    out["eight"] = measure(8, warm=2, reps=4)
    out["product"] = product_probe()
    if not args.no_c5:
        out["c5"] = c5_yardstick()
        if "evals_per_s" in out["c5"]:
            out["c5"]["d3_scaled_to_128"] = out["c5"]["evals_per_s"] / 8.0
    # the algorithmic work of one evaluation in products (8 P^3 each): per step the nominal and the np variants'
    # exponentials (3 powers + the Horner steps + the squarings of the step's degree), one prefix product and
    # two for Y: reported as a rate over the measured time with the degree-16, no-squaring count (6 per exponential)
    prods = NT * ((1 + NP) * 6 + 3)
    out["credited_tflops_eight"] = prods * 8.0 * D ** 3 * out["eight"]["evals_per_s"] / 1e12
    print(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "tiled_probe.json"), "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
