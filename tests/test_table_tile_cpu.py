"""CPU check of the lean table kernels' tile layout ("the
epoch on the table"): tests/table_tile_check.cc, built with the host compiler
on dependence_free_rl_amd/csrc/table_tile_layout.h, for the shipped tile height
and for both heights the header builds at (16 and 32 rows).
"""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("rows", [None, 16, 32])
def test_table_tiles(tmp_path, rows):
    exe = str(tmp_path / "table_tile_check")
    cmd = ["g++", "-O1", "-std=c++17", "-Wall",
           "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc")]
    if rows is not None:
        cmd.append("-DXH_TT_ROWS=%d" % rows)
    subprocess.run(cmd + [os.path.join(REPO, "tests", "table_tile_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "table tiles: ok" in out.stdout
    if rows is not None:
        assert "R = %d," % rows in out.stdout
