"""Pins tests/venv_loss_ref.py, the host restatement the GPU tests of
xh_venv_policy_loss compare against (CPU only):
  the one-hot Jacobian form of the logits gradient equals the full (linear -
    quadratic) matrix times the backprop row, bit for bit;
  the clipped-loss gradient agrees with its float64 evaluation within 4 *
    2^-24 (relative): the ratio, one product and one division round once each,
    and 1.0f +- eps is the f32 bound on both sides;
  on every clipped-loss input set of the GPU tests no row has to be left out
    of a float64 comparison, every ratio is at least 0.009 away from a clip
    boundary, and every (clip regime, sign of A) pair holds at least 10% of
    the rows."""
import numpy as np
import pytest

import venv_loss_ref as vr

f32 = np.float32
# the GPU tests' input sets: each shape's T * N rows, the 8-bin case of 600
# rows (several workgroups) and the 16-bin case of 72 (more than one wave)
SETS = [(c, None) for c in vr.CASES] + [(vr.CASES[0], 600),
                                            (vr.CASES[4], 72)]
SET_IDS = ["B%d-n%s" % (c[0], n or vr.T * c[2]) for c, n in SETS]


@pytest.mark.parametrize("B", [8, 16, 128])
def test_one_hot_jacobian_equals_full_matrix(B):
    """g_k = ((k == ch ? p_k : 0) - p_k p_ch) d against the B x B matrix times
    the one-hot row [0 .. d .. 0], accumulated from 0.0f in k order: the other
    B - 1 products are exact zeros and adding them changes no bit (no entry of
    these rows is zero, so no result is a negative zero)."""
    inp = vr.clipped_inputs((B, 1, 6), total=24)
    p, ch = inp["probs"], inp["ch"]
    assert (p > 0).all()
    d = vr.d_clipped_f32(p[np.arange(24), ch], inp["p_old"], inp["adv"], vr.EPS)
    got = vr.grad_f32(p, ch, inp["p_old"], inp["adv"], "logits", "clipped")
    assert (got != 0).all()
    for i in range(24):
        bp = np.zeros(B, f32)
        bp[ch[i]] = d[i]
        want = vr.jacobian_full_f32(p[i], bp)
        np.testing.assert_array_equal(got[i].view(np.uint32),
                                      want.view(np.uint32))


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_clipped_gradient_against_float64(sel):
    inp = vr.clipped_inputs(*sel)
    n = len(inp["ch"])
    p = inp["probs"]
    p_ch = p[np.arange(n), inp["ch"]]
    d = vr.d_clipped_f32(p_ch, inp["p_old"], inp["adv"], vr.EPS)
    d64 = vr.d_clipped_f64(p_ch, inp["p_old"], inp["adv"], vr.EPS)
    rel = np.abs(d.astype(np.float64) - d64) / np.abs(d64)
    print("max |d - d64| / |d64| = %.3f * 2^-24" % (rel.max() / vr.U32))
    assert np.all(rel <= 4 * vr.U32)
    # the probabilities' form puts d at the choice and zeros elsewhere
    g = vr.grad_f32(p, inp["ch"], inp["p_old"], inp["adv"], "probs", "clipped")
    assert np.count_nonzero(g) == n
    np.testing.assert_array_equal(g[np.arange(n), inp["ch"]], d)


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_no_row_is_excluded(sel):
    inp = vr.clipped_inputs(*sel)
    n = len(inp["ch"])
    hi, lo = (float(b) for b in vr.clip_bounds(vr.EPS))
    p_ch = inp["probs"][np.arange(n), inp["ch"]]
    assert (inp["p_old"] > 0).all() and (inp["p_old"] < 1).all()
    assert (inp["adv"] > 0).any() and (inp["adv"] < 0).any()
    # the ratios of the f32 probabilities and of the float64 softmax (the
    # kernel's own softmax lies within (B + 4) 2^-24 of the latter)
    for p in (p_ch.astype(np.float64), inp["p64"][np.arange(n), inp["ch"]]):
        r = p / inp["p_old"].astype(np.float64)
        assert np.abs(r - inp["ratio"]).max() < 1e-6
        assert np.minimum(np.abs(r - hi), np.abs(r - lo)).min() >= 0.009
        assert vr.excluded_rows(p, inp["p_old"], inp["adv"]).sum() == 0
        share = np.bincount(vr.regimes(p, inp["p_old"], inp["adv"]),
                            minlength=6) / n
        print("regime shares", share)
        assert share.min() >= 0.10


def test_skipped_rows_and_the_value_head():
    """q_old <= 0 or NaN: zero gradient and dvalue rows, counted in SKIPPED
    only; the value head is (v - target) * value_scale in f32."""
    inp = vr.clipped_inputs(vr.CASES[0])
    n = len(inp["ch"])
    q = inp["p_old"].copy()
    q[[1, 5, 7]] = [0.0, np.nan, -0.25]
    for kind, loss in (("logits", "clipped"), ("probs", "log")):
        g = vr.grad_f32(inp["probs"], inp["ch"], q, inp["adv"], kind, loss)
        assert not g[[1, 5, 7]].any() and np.isfinite(g).all()
        assert g[[0, 2, 3]].any(axis=1).all()
    v = np.linspace(-1, 1, n).astype(f32)
    tg = np.linspace(2, -3, n).astype(f32)
    dval, dv = vr.dvalue_f32(v, tg, 0.5, q)
    np.testing.assert_array_equal(dval[0], (v[0] - tg[0]) * f32(0.5))
    assert not dval[[1, 5, 7]].any()
    st, _ = vr.stats_f64(inp["probs"], inp["ch"], q, inp["adv"], vr.EPS, dv)
    assert st[vr.SKIPPED] == 3 and st[vr.ROWS] == n - 3
    full, _ = vr.stats_f64(inp["probs"], inp["ch"], inp["p_old"], inp["adv"],
                           vr.EPS, dv)
    assert full[vr.CLIPPED] == (vr.regimes(
        inp["probs"][np.arange(n), inp["ch"]], inp["p_old"], inp["adv"]) // 2
        != 1).sum()
    assert full[vr.K3_SUM] > 0 and full[vr.ENTROPY_SUM] > 0
