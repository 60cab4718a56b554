"""The tiled engine's control word (robustgrape_amd/csrc/grape_tiled_ctl.hpp: make_ctl, taylor_top, julia_m_index,
the scalar lines of k_tctl) on the host: built with hipcc as host code (the same header the device code includes)
and checked by tests/c/tiled_ctl_check.cpp against a counting restatement over the whole range of the format.
make_ctl is total: a norm of +inf or NaN returns, with no squarings (before, the search for s never ended at +inf
and a k_tctl workgroup would have spun for ever: the program runs under a time limit, which is the test of that).
Non-finite controls are checked here only, never on a GPU.  Julia's degree slots are compared with
the oracle's own choice (oracle.grape_oracle.pade_degree, what julia_exp takes) at the four thresholds and their
neighbouring doubles."""
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SLOT = {3: 0, 5: 1, 7: 2, 9: 3, 13: 4}


@pytest.mark.skipif(not os.path.exists(HIPCC) and not shutil.which("hipcc"), reason="no hipcc")
def test_make_ctl_against_a_counting_restatement_and_total(tmp_path):
    from oracle import grape_oracle as O
    exe = str(tmp_path / "tiled_ctl_check")
    subprocess.run([HIPCC, "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "robustgrape_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "tiled_ctl_check.cpp"), "-o", exe], check=True, capture_output=True)
    norms = [0.0, 1e-300, 1.0, 5.4, 30.0, 1e300]
    for t in (0.015, 0.25, 0.95, 2.1):
        norms += [math.nextafter(t, 0.0), t, math.nextafter(t, math.inf)]
    out = subprocess.run([exe] + [v.hex() for v in norms], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    got, slots = {}, []
    for line in out.splitlines():
        f = line.split()
        if f[0] == "m_index":
            slots.append((float.fromhex(f[1]), int(f[2])))
        else:
            got[f[0]] = f[1]
    assert int(got["checked"]) >= 1000000 + 600 and int(got["mismatches"]) == 0, got
    assert int(got["s_inf"]) == 0 and int(got["s_nan"]) == 0, got
    assert int(got["s_dbl_max"]) == int(got["largest_s"]) == 1025, got   # DBL_MAX = (1 - 2^-53) 2^1024; <= 1 075
    assert [v for v, _ in slots] == norms
    for v, slot in slots:
        assert slot == SLOT[O.pade_degree(v)[0]], (v, slot)
