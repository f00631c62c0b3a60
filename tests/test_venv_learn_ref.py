"""Pin the host references of venv_learn_ref.py before test_gpu_venv_learn.py
trusts them: against long_window_ref's restatements (themselves pinned to the
CPU oracle by test_long_window_ref.py) and against venv_act_ref's reference
trajectories.  CPU only."""
import numpy as np
import pytest

import long_window_ref as lw
import venv_learn_ref as vl
from venv_act_ref import mixed_rows, run

GAMMA, LAM = 0.99, 0.95
WINDOWS = [1, 7, 8, 9, 17, 64]


@pytest.mark.parametrize("T", WINDOWS)
def test_implied_rewards_give_the_trainer_restatements(T):
    """With reward = done ? 0 : 1 the restatements with explicit rewards are
    gae_f32 / td_targets_f32 bit for bit, with terminals on and beside every
    multiple of 8 from both ends of the window."""
    N = 24
    g = np.random.default_rng(100 + T)
    done = vl.edge_done(T, N, T)
    if T >= 17:  # the pattern is what the docstring says
        assert done[8, 2] and done[7, 3] and done[9, 4] and done[T - 9, 5]
        assert done[0, 8] and done[T - 1, 8]
    assert not done[:, 0].any() and done[:, 1].all()
    reward = np.where(done != 0, 0.0, 1.0).astype(np.float32)
    values = g.normal(0.0, 2.0, (T + 1, N)).astype(np.float32)
    v_term = g.normal(0.0, 2.0, (T, N)).astype(np.float32)
    adv = vl.gae_reward_f32(done, reward, values, GAMMA, LAM)
    np.testing.assert_array_equal(adv, lw.gae_f32(done, values, GAMMA, LAM))
    np.testing.assert_array_equal(
        vl.td_targets_reward_f32(done, reward, values, v_term, GAMMA),
        lw.td_targets_f32(done, values, v_term, GAMMA))
    np.testing.assert_array_equal(
        vl.td_targets_reward_f32(done, reward, values, None, GAMMA),
        lw.td_targets_f32(done, values, np.zeros((T, N), np.float32), GAMMA))
    lr = vl.lambda_return_f32(adv, values)
    assert lr.dtype == np.float32
    np.testing.assert_array_equal(lr, adv + values[:T])
    a64, S = vl.gae_reward_f64_forward(done, reward, values, GAMMA, LAM)
    b64, S2 = lw.gae_f64_forward(done, values, GAMMA, LAM)
    np.testing.assert_allclose(a64, b64, rtol=0, atol=1e-12 * S.max())
    np.testing.assert_allclose(S, S2, rtol=1e-13)


@pytest.mark.parametrize("T", WINDOWS)
def test_f32_gae_within_the_stated_bound_of_the_forward_sum(T):
    """Random rewards in [-2, 2] and values in [-50, 50]: the float32 reverse
    scan stays within 4 * 2^-24 * S_t of the float64 forward sum (DESIGN.md's
    gae_kernel row states the bound)."""
    N = 40
    g = np.random.default_rng(7 * T + 1)
    done = vl.edge_done(T, N, T + 50)
    reward = g.uniform(-2.0, 2.0, (T, N)).astype(np.float32)
    values = g.uniform(-50.0, 50.0, (T + 1, N)).astype(np.float32)
    a32 = vl.gae_reward_f32(done, reward, values, GAMMA, LAM)
    a64, S = vl.gae_reward_f64_forward(done, reward, values, GAMMA, LAM)
    err = np.abs(a32.astype(np.float64) - a64)
    print("T=%d: max err / (2^-24 S) = %.3f" % (T, (err / (lw.U32 * S)).max()))
    assert (S > 0).all() and (S >= np.abs(a64) * (1 - 1e-12)).all()
    assert np.all(err <= 4 * lw.U32 * S)


@pytest.mark.parametrize("case", [(8, 2, 19), (32, 1, 70)],
                         ids=lambda c: "B%d-D%d-N%d" % c)
def test_next_rows_are_terminal_views_or_the_following_slot(case):
    """On a reference trajectory: next_rows equals obs_f64(terminal_views) on
    the ended rows and the following slot's observation elsewhere; state_rows
    is the trajectory's own observations."""
    B, D, N = case
    S = 16
    ref = run(B, D, N, 4242, mixed_rows(B * 10 + D, S, N, B))
    done = ref["done"] != 0
    assert done.any() and not done.all()
    record = {"bins": ref["bins"][:S], "items": ref["item"][:S],
              "action": ref["action"], "done": ref["done"]}
    nxt = vl.next_rows(record, (ref["bins"][S], ref["item"][S]))
    assert nxt.shape == (S * N, B * 2 * D)
    follow = lw.obs_f64(ref["bins"][1:].reshape(S * N, B, D),
                        ref["item"][1:].reshape(S * N, D))
    open_rows = ~done.reshape(-1)
    np.testing.assert_array_equal(nxt[open_rows], follow[open_rows])
    t, e, eb, ei = lw.terminal_views(ref["bins"], ref["item"], ref["action"],
                                     ref["done"])
    assert len(t) == done.sum()
    np.testing.assert_array_equal(nxt[t * N + e], lw.obs_f64(eb, ei))
    # an ended row is not what followed it: the env was reset
    assert (nxt[t * N + e] != follow[t * N + e]).any(axis=1).all()
    st = vl.state_rows(record, ref["bins"][S], ref["item"][S])
    np.testing.assert_array_equal(
        st, ref["obs"].reshape((S + 1) * N, B * 2 * D).astype(np.float64))


def test_stats_are_exact_sums():
    a = np.array([[1.5, -2.25], [2.0 ** -20, 3.0]], np.float32)
    s = vl.stats_f64(a, [[0, 1], [1, 1]])
    assert s.tolist() == [2.25 + 2.0 ** -20, 16.3125 + 2.0 ** -40, 4, 3]
