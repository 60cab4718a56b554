"""The merged walks' table-driven e^{i t} (robustgrape_amd/csrc/grape_cis.hpp cis_tab, grape_cis_table.hpp) on the
host: built with hipcc as host code (the same source the device code includes) and checked against x87 long double
sinl / cosl -- at most 1 unit of 2^-52 absolute up to the fast-path bound (the figure cis_fast is held to,
tests/test_cis_cpu.py), exact at 0, every table index met, every table entry within half a unit of its last place
(exactly 0 and +-1 at the multiples of pi / 2), and the committed table is what scripts/gen_cis_table.py writes."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="no hipcc")
def test_cis_tab_against_long_double(tmp_path):
    exe = str(tmp_path / "cis_tab_check")
    subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "robustgrape_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "cis_tab_check.cpp"), "-o", exe], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {k: float(v) for k, v in (line.split() for line in out.splitlines())}
    print(got)
    assert got["sin_err"] <= 1.0 and got["cos_err"] <= 1.0, got
    assert got["sin0"] == 0.0 and got["cos0"] == 1.0
    assert got["indices"] == 128
    assert got["table_ulp"] <= 0.5 and got["table_axes_exact"] == 1, got


def test_committed_table_is_the_generated_one():
    gen = os.path.join(ROOT, "scripts", "gen_cis_table.py")
    assert subprocess.run([sys.executable, gen, "--check"]).returncode == 0
