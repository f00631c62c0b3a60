"""CPU check of the compaction pass's duplicate search on lane masks (DESIGN.md
§3.0e, "the duplicate search"): tests/pack_dedup_check.cc, built with the host
compiler on dependence_free_rl_amd/csrc/spec8_pack_layout.h.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_dedup(tmp_path):
    exe = str(tmp_path / "pack_dedup_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "pack_dedup_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "pack dedup: ok" in out.stdout
