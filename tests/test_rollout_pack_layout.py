"""CPU check of the packed table rollout's lane layout
(dependence_free_rl_amd/csrc/rollout_pack_layout.h, which
rollout_pack_kernels.hip is written on): tests/rollout_pack_layout_check.cc,
built with the host compiler and contraction off, verifies for 16, 8 and 4
lanes per env that the lanes map one to one onto the wave's envs and bins, that
a tail wave masks whole segments, and that the packed order of the softmax sum
(in the lane first, then over the segment's lanes) gives the bits of the
64-lane order the one-env-per-wave kernel uses, over 4000 vectors per layout
with denormals and dominant terms among them."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_pack_layout(tmp_path):
    exe = str(tmp_path / "rollout_pack_layout_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "rollout_pack_layout_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rollout pack layout: ok" in out.stdout
