"""CPU check of the device row rings' index arithmetic
(dependence_free_rl_amd/csrc/xh_ring.h, which xh_host.h's ring_read -- behind
xh_trainer_get_stats, xh_trainer_get_update_diag and xh_venv_get_episode_rows
-- is written on): tests/ring_span_check.cc built with the host compiler
compares the two-run split with a brute-force walk of the ring for every
history in 1..5, rows in 0..12 and request inside the readable window, count 0
included, and checks that negative, past-the-end and overwritten requests are
refused with the right reason."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ring_span(tmp_path):
    exe = str(tmp_path / "ring_span_check")
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "ring_span_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ring span: ok" in out.stdout
