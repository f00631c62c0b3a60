"""The host restatements in tests/venv_kl_ref.py, which the GPU tests of the
VecEnv's KL-PPO calls compare against (CPU only):

  * kl_grad_f32 equals policy_loss_row + (p - q) * beta formed as
    tests/test_gpu_model_api.py forms its kl_regulated expectation (the
    expression xh_action_loss_grad is pinned to);
  * beta_rule_f32 equals loss_kl's rule (oracle/oracle.c): on the rows a
    KL-PPO oracle trainer logs, and, transcribed line by line, on a table of d
    with values just inside and outside both thresholds, 0, NaN and both
    clamps;
  * row_kl_f64's zero rule and its +inf.
"""
import math

import numpy as np

import venv_kl_ref as kr
import venv_loss_ref as vr

f32 = np.float32


def test_gradient_restatement_is_the_model_api_expression():
    rng = np.random.default_rng(9)
    rows, B = 50, 16
    p = rng.random((rows, B)).astype(f32) + f32(0.01)
    p /= p.sum(1, keepdims=True)
    q = rng.random((rows, B)).astype(f32) + f32(0.01)
    q /= q.sum(1, keepdims=True)
    ch = rng.integers(0, B, rows).astype(np.int32)
    adv = rng.normal(size=rows).astype(f32)
    beta = f32(0.05)
    want = np.zeros((rows, B), f32)
    for r in range(rows):
        c, a = ch[r], adv[r]
        row = p[r] * a
        row[c] = f32(p[r, c] * a) - a
        want[r] = row + (p[r] - q[r]) * beta
    got = kr.kl_grad_f32(p, q, ch, np.ones(rows, f32), adv, beta)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    # beta 0 and p == q both leave policy_loss's row
    log = vr.grad_f32(p, ch, np.ones(rows, f32), adv, "probs", "log")
    np.testing.assert_array_equal(
        kr.kl_grad_f32(p, q, ch, np.ones(rows, f32), adv, 0.0), log)
    np.testing.assert_array_equal(
        kr.kl_grad_f32(p, p, ch, np.ones(rows, f32), adv, beta), log)
    # scale and the skipped rows
    q_old = np.ones(rows, f32)
    q_old[[3, 7]] = [0.0, np.nan]
    got = kr.kl_grad_f32(p, q, ch, q_old, adv, beta, scale=0.25)
    assert not got[[3, 7]].any()
    keep = np.ones(rows, bool)
    keep[[3, 7]] = False
    np.testing.assert_array_equal(got[keep], want[keep] * f32(0.25))


def _loss_kl_rule(d_avg, d_targ, beta):
    """oracle/oracle.c loss_kl, the lines after d_avg, one by one in f32."""
    d_avg, d_targ, b = f32(d_avg), f32(d_targ), f32(beta)
    if abs(d_avg) < d_targ / f32(1.5):
        b = b / f32(2)
    elif abs(d_avg) > d_targ * f32(1.5):
        b = b * f32(2)
    if b < f32(1e-25):
        b = f32(1e-25)
    if b > f32(0.1):
        b = f32(0.1)
    return f32(b)


def test_beta_rule_on_a_table():
    d_targ = f32(0.01)
    lo, hi = d_targ / f32(1.5), d_targ * f32(1.5)
    table = [0.0, -0.0, float("nan"), 1e-30, float("inf"), 0.01, -0.01,
             lo, np.nextafter(lo, f32(0)), np.nextafter(lo, f32(1)),
             hi, np.nextafter(hi, f32(0)), np.nextafter(hi, f32(1)),
             -lo, -np.nextafter(lo, f32(0)), -hi, -np.nextafter(hi, f32(1))]
    betas = [1.0, 0.1, 0.08, 0.05, 0.03, 1e-3, 1.5e-25, 1e-25, 3e-26, 0.0]
    moved = set()
    with np.errstate(all="ignore"):
        for d in table:
            for beta in betas:
                b0, dd, b1 = kr.beta_rule_f32(np.float64(f32(d)) * 7.0, 7.0,
                                              d_targ, beta)
                want = _loss_kl_rule(dd, d_targ, beta)
                assert b0.tobytes() == f32(beta).tobytes()
                assert b1.dtype == f32 and b1.tobytes() == want.tobytes(), \
                    (d, beta, b1, want)
                assert f32(1e-25) <= b1 <= f32(0.1)
                moved.add("half" if b1 < b0 else "double" if b1 > b0
                          else "same")
    assert moved == {"half", "double", "same"}
    # the thresholds themselves are in the dead band, their neighbours not
    assert kr.beta_rule_f32(float(lo), 1.0, d_targ, 0.05)[2] == f32(0.05)
    assert kr.beta_rule_f32(float(np.nextafter(lo, f32(0))), 1.0, d_targ,
                            0.05)[2] == f32(0.025)
    assert kr.beta_rule_f32(float(hi), 1.0, d_targ, 0.04)[2] == f32(0.04)
    assert kr.beta_rule_f32(float(np.nextafter(hi, f32(1))), 1.0, d_targ,
                            0.04)[2] == f32(0.08)
    # no rows: d is NaN and only the clamp acts
    b0, d, b1 = kr.beta_rule_f32(0.0, 0.0, d_targ, 0.05)
    assert math.isnan(d) and b1 == f32(0.05)
    assert kr.beta_rule_f32(0.0, 0.0, d_targ, 1.0)[2] == f32(0.1)
    assert kr.beta_rule_f32(0.0, 0.0, d_targ, 0.0)[2] == f32(1e-25)


def test_beta_rule_reproduces_the_oracle_trainers_log():
    """loss_kl itself: the {beta used, mean KL, beta after} rows of a KL-PPO
    oracle trainer (d_targ 1e-9, beta 1 at first: epoch 0's KL of 0 halves it,
    the later epochs double it into the upper clamp)."""
    from dependence_free_rl_amd import init_policy, init_value
    from oracle import pyoracle as po
    B, D, N, T, widths = 8, 2, 8, 4, (128, 64)
    orc = po.Trainer(po.OR_KLPPO, B, D, N, T,
                     po.perbin_model(2 * D, list(widths), po.OR_SOFTMAX),
                     init_policy(D, *widths, seed=3),
                     po.full_model(B * 2 * D, [64, 32], 1),
                     init_value(B, D, seed=4), x0=99)
    rows = []
    for _ in range(2):
        orc.rollout()
        orc.learn()
        rows.append(np.array(orc.buf(po.BUF_KL), f32).reshape(-1, 3))
    rows = np.concatenate(rows)
    assert len(rows) >= 4 and rows[0, 0] == 1.0
    for used, d, after in rows:
        got = kr.beta_rule_f32(np.float64(d), 1.0, 1e-9, used)
        assert got[2].tobytes() == f32(after).tobytes(), (used, d, after, got)
    assert (rows[:, 2] != rows[:, 0]).any()


def test_row_kl_zero_rule():
    p = np.array([[0.5, 0.25, 0.25, 0.0], [0.5, 0.5, 0.0, 0.0],
                  [0.25, 0.25, 0.25, 0.25]], f32)
    q = np.array([[0.5, 0.5, 0.0, 0.0], [0.5, 0.25, 0.25, 0.0],
                  [0.25, 0.25, 0.25, 0.25]], f32)
    kl, mag = kr.row_kl_f64(p, q)
    assert kl[0] == 0.5 * math.log(2.0) and mag[0] == kl[0]
    assert kl[1] == math.inf          # p_k == 0 < q_k
    assert kl[2] == 0.0 and mag[2] == 0.0
    st, m = kr.kl_stats_f64(p[[0, 2, 2]], q[[0, 2, 2]],
                            np.array([1.0, 0.0, 0.5], f32))
    assert st[kr.ROWS] == 2 and st[kr.KL_SUM] == kl[0]
    assert st[kr.KL_SQSUM] == kl[0] * kl[0] and m == mag[0]


def test_kl_inputs_have_both_kinds_of_zero():
    for sel in [(c, None) for c in vr.CASES] + [(vr.CASES[0], 600)]:
        q = kr.kl_inputs(sel)
        n, B = q.shape
        assert q.dtype == f32 and n == (sel[1] or vr.T * sel[0][2])
        s = q.sum(axis=1, dtype=np.float64)
        assert np.all(s > 0) and np.all(s < 1 + 1e-5)
        # rows 0, 7, ...: softmax underflow; rows 0, 5, ...: a zero set outright
        assert (q[0] == 0).sum() >= 3 and (q[5] == 0).sum() >= 1
