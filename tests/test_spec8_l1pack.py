"""CPU checks for the config-3 train kernel's packed layer 1 and fused pair
split (dependence_free_rl_amd/csrc/policy_spec8_kernels.hip):
tests/l1pack_check.cc compiled with the host compiler checks, from
spec8_l1_layout.h alone, that the K slots 0..14 hit every (part, input) pair
once and slot 15 is zero in both operands; that the A and X fragments built by
the helpers the kernel uses sum, in double, to exactly sum_parts part . input
for random W1 rows (wide exponents, negatives, zeros), both item kinds and
every x in {-16 .. 16} / 8; that the per-half view is k = 8 h + e; and, for the
two-scale f16 pair split restated on doubles, that hi is the exact product
rounded once to f16 and hi + lo is within 2^-22 relative of h g wherever the
form it replaces is."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_l1pack_and_split(tmp_path):
    exe = str(tmp_path / "l1pack_check")
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "l1pack_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "slots: ok" in out.stdout
    assert "halves: ok" in out.stdout
    assert "fragments: ok" in out.stdout
    assert "split: ok" in out.stdout
