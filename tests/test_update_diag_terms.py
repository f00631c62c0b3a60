"""CPU check of the per-row terms of the PPO update diagnostics
(dependence_free_rl_amd/csrc/xh_diag.h, compiled by the sum kernel and by
this test alike): tests/update_diag_check.cc built with the host compiler
compares them with a long double restatement at p_new == p_old, at a ratio of
exactly 1 +- eps and one ulp either side of each, at p_new = 0, with a
subnormal p_old, with A < 0 (where the min picks the other product), with NaN
inputs, and over a pseudo-random sweep."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_update_diag_terms(tmp_path):
    exe = str(tmp_path / "update_diag_check")
    # no -ffast-math, no x87: the doubles are IEEE doubles
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "update_diag_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "update diag terms: ok" in out.stdout
