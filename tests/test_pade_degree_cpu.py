"""The small engine's degree choice (robustgrape_amd/csrc/grape_pade_degree.hpp pade_degree: the lines k_expm,
k_expm_high and k_expm_raw run) on the host: built with hipcc as host code (the same header the device code
includes) and checked by tests/c/pade_degree_check.cpp against a counting restatement over the whole range of the
format.  pade_degree is total: a norm of +inf or NaN returns m = 13 with no squarings (before, (int)ceil(+inf)
saturated and expm_high would have squared about 2^31 times, a kernel that does not return).  Non-finite norms are
checked here only, never on a GPU.  Every finite case is Julia's expression unchanged: DBL_MAX keeps s = 1022, and
the degrees and counts at the thresholds and their neighbouring doubles are the oracle's own
(oracle.grape_oracle.pade_degree, what julia_exp takes)."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="no hipcc")
def test_pade_degree_against_a_counting_restatement_and_total(tmp_path):
    from oracle import grape_oracle as O
    exe = str(tmp_path / "pade_degree_check")
    subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "robustgrape_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "pade_degree_check.cpp"), "-o", exe], check=True, capture_output=True)
    norms = [0.0, 5e-324, 1e-300, 1.0, 30.0, 1e300, 1.7976931348623157e308]
    for t in (0.015, 0.25, 0.95, 2.1, 5.4, 10.8, 5.4 * 2 ** 20):
        norms += [math.nextafter(t, 0.0), t, math.nextafter(t, math.inf)]
    out = subprocess.run([exe] + [v.hex() for v in norms], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    got, degrees = {}, []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "degree":
            degrees.append((float.fromhex(f[1]), int(f[2]), int(f[3])))
        else:
            got[f[0]] = f[1]
    assert int(got["checked"]) >= 1000000 + 140 and int(got["mismatches"]) == 0, got
    # the double log2 of a quotient a few ulps above 2^k is k: only the constructed upper neighbours, few in all
    assert int(got["log2_rounded"]) <= 64, got
    assert (int(got["m_inf"]), int(got["s_inf"])) == (13, 0) and (int(got["m_nan"]), int(got["s_nan"])) == (13, 0), got
    assert (int(got["m_dbl_max"]), int(got["s_dbl_max"])) == (13, 1022) and int(got["largest_s"]) == 1022, got
    assert [v for v, _, _ in degrees] == norms
    for v, m, s in degrees:
        assert (m, s) == O.pade_degree(v), (v, m, s)
