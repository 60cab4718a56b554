"""bench.py's plain run and `--dump-outputs`.

A plain run (`--gpus 1 --steps K --warmup W`) times its K steps and prints one line with
`ms_per_step`; the legs that take runs of their own appear only with `--full`.
`--dump-outputs DIR` writes what the last timed step computed as DIR/<name>.npy (float64), cut
to a fixed seeded sample of restarts when the whole output would not fit the dump budget.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FULL_ONLY = ("c4_strong", "whole_matrix_path", "host_path", "single_eval", "c4_points", "cpu_baseline",
             "cpu_baseline_allcores", "vs_cpu")


def test_dump_rows_are_fixed_and_fit_the_budget():
    import bench
    row = 8 * (1 + 513)  # F and F_dx of one C2 restart
    small = bench.dump_rows(100, row)
    assert np.array_equal(small, np.arange(100))  # everything when it fits
    count = 262144  # the default C2 step: 1.08 GB of F_dx
    rows = bench.dump_rows(count, row)
    assert np.array_equal(rows, bench.dump_rows(count, row))  # the same sample every time
    assert len(rows) == bench.DUMP_BUDGET // row and len(rows) * row <= 64e6
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < count
    assert rows[-1] - rows[0] > count // 2  # spread over the step, not its head


def test_dump_outputs_writes_float64_npy(tmp_path, monkeypatch):
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)  # a small budget keeps the arrays small
    rng = np.random.default_rng(5)
    n = 3 * bench.DUMP_BUDGET // (8 * 1001)  # three times the budget
    F = rng.uniform(size=n)
    G = torch.from_numpy(rng.uniform(size=(n, 1000)))
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), {"F": F, "F_dx": G})
    rows = bench.dump_rows(n, 8 * 1001)
    f, g = np.load(out / "F.npy"), np.load(out / "F_dx.npy")
    assert f.dtype == np.float64 and g.dtype == np.float64
    assert f.shape == (len(rows),) and g.shape == (len(rows), 1000)
    assert np.array_equal(f, F[rows]) and np.array_equal(g, G.numpy()[rows])
    assert f.nbytes + g.nbytes <= bench.DUMP_BUDGET
    assert sorted(os.listdir(out)) == ["F.npy", "F_dx.npy"]


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """96 restarts in device passes of 64 (one whole pass and a partial one), 2 timed steps: the line
    holds the contract's keys and none of the --full legs; the dumped F / F_dx are those of a plan of
    the same pass size evaluated here on the same seeded inputs (same library, same kernels: only the
    summation order inside a kernel could differ, so a few ulp of the values' scale)."""
    import torch
    import bench
    from robustgrape_amd.engine import GrapePlan
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "96", "--chunk", "64", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "gradient-evals/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 96 / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    assert sorted(os.listdir(out)) == ["F.npy", "F_dx.npy"]
    F, G = np.load(out / "F.npy"), np.load(out / "F_dx.npy")
    assert F.dtype == np.float64 and G.dtype == np.float64
    assert F.shape == (96,) and G.shape == (96, bench.NT + 1)

    X = bench.restart_inputs(0, 96)
    dev = torch.device("cuda", 0)
    plan = GrapePlan(bench.problem(), nparam=1, device=0, max_batch=64)
    Xd = torch.from_numpy(X).to(dev)
    Fd = torch.empty(96, dtype=torch.float64, device=dev)
    Gd = torch.empty(96, X.shape[1], dtype=torch.float64, device=dev)
    plan.fidelity_grad_device_async(Xd.data_ptr(), Fd.data_ptr(), Gd.data_ptr(), 96, 0, 0)
    plan.synchronize()
    torch.cuda.synchronize()
    F0, G0 = Fd.cpu().numpy(), Gd.cpu().numpy()
    plan.close()
    eF, eG = np.max(np.abs(F - F0)), np.max(np.abs(G - G0))
    print(f"dump vs in-process plan: max|dF| = {eF:.3e}, max|dF_dx| = {eG:.3e} (scale {np.max(np.abs(G0)):.3e})")
    assert 0.0 < F0.min() and F0.max() <= 1.0 + 1e-12
    assert eF <= 16 * np.finfo(float).eps
    assert eG <= 16 * np.finfo(float).eps * np.max(np.abs(G0))
