"""CPU check of the rollout logit table's index arithmetic
(dependence_free_rl_amd/csrc/xh_logit_table.h, which policy_kernels.hip's
table builds are written on): tests/rollout_table_index_check.cc built with
the host compiler verifies that the index is a bijection from [-8, 8]^2 onto
0..288, that the enumeration the table is filled by is its inverse and writes
every entry of both items exactly once, and that every index stays inside the
table's 578 floats."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_table_index(tmp_path):
    exe = str(tmp_path / "rollout_table_index_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "rollout_table_index_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rollout table index: ok" in out.stdout
