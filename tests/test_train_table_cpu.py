"""CPU checks of the train epoch on the table ("the epoch on
the table").

- tests/train_table_batch_check.cc, built with the host compiler on
  dependence_free_rl_amd/csrc/spec8_table_layout.h: the table batch covers each
  of the 578 entries exactly once, the tail rows have count 0, and the
  enumeration and lt::entry are inverses.
- the formula the kernels implement, in float64: at activations that depend on
  a row's table entry alone, every parameter gradient is a sum over rows of
  g_row times a per-entry feature, which equals the sum over entries of G_s
  times that feature, G_s the sum of g over the rows with entry s.
"""
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = 578


def test_table_batch_layout(tmp_path):
    exe = str(tmp_path / "train_table_batch_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall",
                    "-I" + os.path.join(REPO, "dependence_free_rl_amd", "csrc"),
                    os.path.join(REPO, "tests", "train_table_batch_check.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "train table batch: ok" in out.stdout


def test_row_sum_equals_entry_sum():
    rng = np.random.RandomState(7)
    rows, H = 4099, 128
    s = rng.randint(0, ENTRIES, rows)
    s[:5] = (0, ENTRIES - 1, 288, 289, 0)      # both ends of both items, a repeat
    g = rng.standard_normal(rows) * np.exp(rng.uniform(-12, 2, rows))
    # per-entry features: H2(s) for dW3, H1(s)^T (w3 * relu'(Z2(s))) for dW2, 1 for db3
    h2 = np.maximum(rng.standard_normal((ENTRIES, H)), 0.0)
    h1 = np.maximum(rng.standard_normal((ENTRIES, H)), 0.0)
    dz = rng.standard_normal(H)[None, :] * (rng.standard_normal((ENTRIES, H)) > 0)
    G = np.zeros(ENTRIES)
    np.add.at(G, s, g)
    assert G.dtype == np.float64
    # dW3
    by_row = (g[:, None] * h2[s]).sum(0)
    by_entry = (G[:, None] * h2).sum(0)
    np.testing.assert_allclose(by_entry, by_row, rtol=1e-11, atol=1e-11 * np.abs(g).sum())
    # dW2
    by_row = np.einsum("r,ri,ro->oi", g, h1[s], dz[s])
    by_entry = np.einsum("s,si,so->oi", G, h1, dz)
    np.testing.assert_allclose(by_entry, by_row, rtol=1e-11, atol=1e-11 * np.abs(g).sum())
    # db3
    np.testing.assert_allclose(G.sum(), g.sum(), rtol=1e-11, atol=1e-12 * np.abs(g).sum())
    # an entry no row carries contributes nothing
    assert (G[np.setdiff1d(np.arange(ENTRIES), s)] == 0).all()
