"""The wide gradient walk's difference weights (robustgrape_amd/csrc/grape_fd_weight.hpp: a per-plan base plus a
first-order term) on the host: built with hipcc as host code (the same source the device code includes) and held
against the per-step form (cis_m1 and the recurrence) with x87 long double as the reference.  The yardstick is the
per-step form's own worst error on the same inputs, in units of 2^-52 |rho(m)|: the new form may exceed it by at
most one unit.  Wherever fl(x + eps) - x == eps the two forms agree bit for bit, and wherever x + eps rounds far
from x + eps the guard hands the step to the per-step form (tests/c/fd_weight_check.cpp lists the inputs)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="no hipcc")
def test_fd_weights_against_long_double(tmp_path):
    exe = str(tmp_path / "fd_weight_check")
    subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "robustgrape_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "fd_weight_check.cpp"), "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {k: float(v) for k, v in (line.split() for line in out.splitlines())}
    print(got)
    assert got["new_err"] <= got["parent_err"] + 1.0, got
    assert got["n_exact"] > 1000 and got["exact_mismatch"] == 0, got
    assert got["n_refuse"] > 1000 and got["refuse_wrong"] == 0, got
    assert got["n_fast"] > got["n_slow"] > 0, got
