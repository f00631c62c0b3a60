"""CPU check of the relu-mask record that the rollout writes for PPO's first
policy epoch (dependence_free_rl_amd/csrc/spec8_e0_layout.h):
tests/e0_layout_check.cc compiled with the host compiler checks that (row,
output) <-> (word, bit) is a bijection over 64 x 128, and that the rollout
lane's view (the row of its r-tile, the 64 outputs of its lane half) and the
train kernel's matrix lane's view (its wave's 32 outputs, one aligned dword)
address the same bits, from the 32x32 MFMA C layout restated in the check."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_e0_layout(tmp_path):
    exe = str(tmp_path / "e0_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "e0_layout_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bijection: ok (8192 bits)" in out.stdout
    assert "rollout view: ok" in out.stdout
    assert "train view: ok" in out.stdout
    assert "same bits: ok" in out.stdout
