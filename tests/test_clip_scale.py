"""CPU check of the gradient-clipping scale formula
(dependence_free_rl_amd/csrc/xh_clip.h, compiled by the clip-and-step kernel
and by this test alike): tests/clip_scale_check.cc built with the host
compiler compares it with a long double restatement at ss = 0, a subnormal,
inf and NaN, at a norm exactly equal to max_norm (scale 1), one ulp above and
below it, with r != 1, and over a pseudo-random sweep."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clip_scale(tmp_path):
    exe = str(tmp_path / "clip_scale_check")
    # no -ffast-math, no x87: the doubles are IEEE doubles
    subprocess.run(["g++", "-O1", "-std=c++17",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "clip_scale_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "clip scale: ok" in out.stdout
