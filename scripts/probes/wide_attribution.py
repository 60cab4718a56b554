"""Where the wide walks' idle cycles are: the in-kernel stamps of the diagnostic build, read after the C2 wide pass
has run back to back on the bench's inputs.

    python scripts/build_variants.py stamps=GRAPE_WIDE_STAMPS=1
    GRAPE_LIB=abvar/libgrape_stamps.so python scripts/probes/wide_attribution.py [--seconds 2] [--out FILE]

(csrc/grape_walk_merged.hpp WideStamp: per wave the shader clock and the 100 MHz clock before its first tile and
after its last, the shader clocks spent in tile seams, HW_ID and XCC_ID.)  Reports, per kernel (forward, gradient):
  1. the in-kernel clock: d(shader clock) / d(100 MHz clock) x 100 MHz, median over waves
  2. per SIMD the finish times of its waves, oldest first, as fractions of the kernel's length (first start to last
     finish on the 100 MHz clock), median over the SIMDs that held four waves; how long the last wave of a SIMD is
     alone; and the issue share of the wave that finishes first over its whole life (steps x VALU instructions per
     step x 4 cycles over its life).  That wave shares the SIMD with three others for most of its life, so this is
     a lower bound on what a wave issues when age-ordered arbitration prefers it, not the rate of a wave running
     alone: the stamps hold no per-tile times, so the last wave's rate while alone cannot be read from them
  3. the share of a wave's life spent in seams (end of a tile's steps to the barrier behind the next load)
  4. the drain seen from the host: the bench's own kernel events against the median wave's life
The stamps are those of the last launch of the run.  One JSON line at the end.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WAVES, WORDS = 8192, 8
VALU_PER_STEP = {"fwd": 93.5, "grad": 233.0}  # profiles/r14/isa_counts.txt (the fast paths)


def read_stamps():
    from robustgrape_amd import _capi
    lib = _capi.lib()
    buf = np.zeros((2, WAVES, WORDS), np.uint64)
    fn = lib.grape_diag_wide_stamps
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_size_t], ctypes.c_int
    rc = fn(buf.ctypes.data, buf.nbytes)
    if rc != 0:
        raise RuntimeError(f"grape_diag_wide_stamps: {rc}")
    return buf


def attribute(name, st, nt, event_ms):
    st = st[st[:, 7] == 1]
    t0, r0, t1, r1, seam, where = (st[:, i].astype(np.int64) for i in range(6))
    life, life_r = t1 - t0, r1 - r0
    clock = float(np.median(life / np.maximum(life_r, 1))) * 100e6
    R0, R1 = int(r0.min()), int(r1.max())
    span = R1 - R0
    hw, xcc = where & 0xFFFFFFFF, (where >> 32) & 0xF
    simd = (xcc << 16) | (hw & 0xFF30)  # XCC, SE, SH, CU, SIMD (HW_ID bits 4-5 and 8-15)
    fin, start, alone = [], [], []
    for key in np.unique(simd):
        m = simd == key
        if m.sum() != 4:
            continue
        f = np.sort((r1[m] - R0) / span)
        fin.append(f)
        start.append(np.sort((r0[m] - R0) / span))
        alone.append(f[3] - f[2])
    fin, start = np.array(fin), np.array(start)
    first = np.array([life[simd == k].min() for k in np.unique(simd)])
    share_first = nt * VALU_PER_STEP[name] * 4.0 / float(np.median(first))
    out = {
        "kernel": name, "waves": int(len(st)), "simds": int(len(np.unique(simd))), "simds_with_4": int(len(fin)),
        "clock_ghz": round(clock / 1e9, 4),
        "kernel_span_ms": round(span / 100e6 * 1e3, 4), "event_ms": round(event_ms, 4),
        "median_wave_life_ms": round(float(np.median(life_r)) / 100e6 * 1e3, 4),
        "finish_fractions_median": [round(float(x), 4) for x in np.median(fin, axis=0)] if len(fin) else None,
        "start_fractions_median": [round(float(x), 4) for x in np.median(start, axis=0)] if len(fin) else None,
        "last_wave_alone_median": round(float(np.median(alone)), 4) if len(fin) else None,
        "issue_share_first_finisher": round(share_first, 4),
        "issue_share_simd": round(4 * nt * VALU_PER_STEP[name] * 4.0 / (span / 100e6 * clock), 4),
        "seam_share_median": round(float(np.median(seam / np.maximum(life, 1))), 4),
        "drain_event_over_median_life": round(event_ms / (float(np.median(life_r)) / 100e6 * 1e3), 4),
    }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=262144)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import bench
    from robustgrape_amd import _capi
    from robustgrape_amd.engine import GrapePlan
    if "GRAPE_WIDE_STAMPS=1" not in _capi.build_defines():
        sys.exit("wide_attribution.py needs the diagnostic build: GRAPE_LIB=abvar/libgrape_stamps.so (see the docstring)")
    fp = bench.problem()
    n = args.batch
    plan = GrapePlan(fp, nparam=1, device=0, max_batch=min(n, 32768))
    X = torch.from_numpy(bench.restart_inputs(0, n)).cuda()
    F = torch.empty(n, dtype=torch.float64, device="cuda")
    G = torch.empty(n, X.shape[1], dtype=torch.float64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.set_stream(stream)
    plan.set_stream(stream.cuda_stream)
    step = lambda: plan.fidelity_grad_device_async(X.data_ptr(), F.data_ptr(), G.data_ptr(), n)  # noqa: E731
    for _ in range(3):
        step()
    plan.synchronize()
    info = plan.sector_info()
    t0, steps = time.perf_counter(), 0
    while time.perf_counter() - t0 < args.seconds:
        for _ in range(50):
            step()
        plan.synchronize()
        steps += 50
    dt = time.perf_counter() - t0
    stamps = read_stamps()
    plan.kernel_times(reset=True)
    plan.set_profiling(True)
    for _ in range(20):
        step()
    plan.synchronize()
    kt = {k: v[0] / 20 for k, v in plan.kernel_times().items() if v[1]}
    plan.set_profiling(False)
    plan.close()
    res = {"build": _capi.build_id(), "defines": list(_capi.build_defines()), "wide": info.get("wide"), "steps": steps,
           "ms_per_step": round(dt / steps * 1e3, 4), "events_ms_per_step": {k: round(v, 4) for k, v in kt.items()},
           "kernels": [attribute("fwd", stamps[0], bench.NT, kt.get("k_walk_fwd", 0.0)),
                       attribute("grad", stamps[1], bench.NT, kt.get("k_walk_grad", 0.0))]}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
