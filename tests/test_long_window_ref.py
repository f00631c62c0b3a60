"""Pin the host references of long_window_ref.py against the CPU oracle
(oracle/oracle.c through po.Trainer) on rollout windows longer than 8 steps,
before test_gpu_long_window.py trusts them.  CPU only.

Every item goes into bin 0 (forced action 0): an 8 x (8, 8) env overflows
every 3 to 5 steps, so about a quarter of a window's transitions are terminal
and, from the engine state chosen here, every env ends at least two episodes
in each window also at T = 9 (asserted: a window must not go sparse
silently).  Two consecutive windows: the second starts inside running
episodes.

The references are fed the oracle's own done flags and values, so each
assertion isolates one function: gae_f32 / gae_f64_forward against
BUF_ADVANTAGES, td_targets_f32 against BUF_TARGETS, terminal_views + value_f64
against BUF_VALUES (and terminal_views + obs_f64 against the oracle's end rows
bit for bit)."""
import numpy as np
import pytest

import long_window_ref as lw
from conftest import RTOL, assert_close
from gpu_helpers import row_index
from oracle import pyoracle as po

B, D, WIDTHS, N = 8, 2, (128, 64), 8
X0 = 31  # every env ends two episodes in both windows, also at T = 9
GAMMA, LAM = 0.99, 0.95
WINDOWS = 2


def oracle_rows(orc, it, T, done):
    """(kind, t, env) of every learn row of the oracle's last learn(), as
    gpu_helpers.row_index gives them for a golden; an end row is a terminal
    one where the transition before it ended the episode."""
    env, step = orc.buf(po.BUF_ROW_ENV), orc.buf(po.BUF_ROW_STEP)
    is_end = orc.buf(po.BUF_ROW_IS_END)
    frozen = np.zeros(len(env), np.int32)
    for k in np.nonzero(is_end)[0]:
        frozen[k] = int(done[step[k] - it * T - 1, env[k]])
    p = "it%d_" % it
    g = {p + "row_env": env, p + "row_step": step, p + "row_is_end": is_end,
         p + "row_frozen": frozen}
    return row_index(g, it, T)


def scatter_rows(rows, vals, T, n):
    """Row values -> (v_state [T+1][n], v_term [T][n]); entries no row
    supplies stay 0 (slot T of an env that ended on step T-1: never read)."""
    v = np.zeros((T + 1, n), np.float32)
    vt = np.zeros((T, n), np.float32)
    for (kind, t, e), x in zip(rows, vals):
        if kind == 2:
            vt[t, e] = x
        else:
            v[t, e] = x
    return v, vt


def window_buffers(orc, T):
    """The oracle's last rollout in the device's layout."""
    n, b, d = orc.N, orc.B, orc.D
    bins = np.zeros((T + 1, n, b, d), np.int32)
    items = np.zeros((T + 1, n, d), np.int32)
    bins[:T] = orc.buf(po.BUF_STEP_BINS).reshape(n, T, b, d).swapaxes(0, 1)
    bins[T] = orc.buf(po.BUF_FINAL_BINS).reshape(n, b, d)
    items[:T] = orc.buf(po.BUF_STEP_ITEM).reshape(n, T, d).swapaxes(0, 1)
    items[T] = orc.buf(po.BUF_FINAL_ITEM).reshape(n, d)
    done = orc.buf(po.BUF_STEP_DONE).reshape(n, T).T.astype(np.uint8)
    action = orc.buf(po.BUF_STEP_CHOICE).reshape(n, T).T
    return bins, items, action, done


@pytest.mark.parametrize("T", [9, 17, 64])
def test_references_against_oracle(T):
    from dependence_free_rl_amd import init_policy
    pol = po.perbin_model(2 * D, list(WIDTHS), po.OR_SOFTMAX)
    val = po.full_model(B * 2 * D, [64, 32], 1)
    orc = po.Trainer(po.OR_PPO, B, D, N, T, pol, init_policy(D, *WIDTHS, seed=3),
                     val, lw.value_params(B, D), gamma=GAMMA, x0=X0)
    worst = {}

    def close(what, x, y):
        worst[what] = max(worst.get(what, 0.0), assert_close(x, y, what=what))

    for it in range(WINDOWS):
        w = "T%d it%d " % (T, it)
        vp_before = orc.params(1)
        orc.rollout(forced=np.zeros((N, T), np.int32))
        bins, items, action, done = window_buffers(orc, T)
        share, per_env = lw.assert_dense(done, w)
        print(w, "terminal share %.3f, episodes per env %d-%d"
              % (share, per_env.min(), per_env.max()))
        orc.learn()
        rows = oracle_rows(orc, it, T, done)
        sm = orc.buf(po.BUF_ROWS).reshape(len(rows), B * 2 * D)
        kinds = np.array([k for k, _, _ in rows])
        assert (kinds == 0).sum() == T * N
        assert (kinds == 2).sum() == int(done.sum())

        # terminal views: the oracle's end rows, bit for bit, then V of them
        tq, eq, eb, ei = lw.terminal_views(bins, items, action, done)
        eobs = lw.obs_f64(eb, ei)
        where = {(t, e): k for k, (kind, t, e) in enumerate(rows) if kind == 2}
        term_rows = np.array([where[(t, e)] for t, e in zip(tq, eq)])
        np.testing.assert_array_equal(eobs.astype(np.float32), sm[term_rows])
        values = orc.buf(po.BUF_VALUES)
        lw.assert_values_differ(values[term_rows], RTOL, w + "v_term")
        close("v_term", lw.value_f64(vp_before, eobs), values[term_rows])
        # ... and V of all (T+1) N states
        v0_ref, vt_ref = scatter_rows(rows, values, T, N)
        v0 = lw.value_f64(vp_before, lw.obs_f64(
            bins.reshape(-1, B, D), items.reshape(-1, D))).reshape(T + 1, N)
        open_T = done[T - 1] == 0  # slot T is a row only where still open
        close("v_state0", v0[:T], v0_ref[:T])
        close("v_state0[T]", v0[T][open_T], v0_ref[T][open_T])

        # TD targets from the oracle's own values
        tg = lw.td_targets_f32(done, v0_ref, vt_ref, GAMMA)
        tg_ref, _ = scatter_rows(rows, orc.buf(po.BUF_TARGETS), T, N)
        close("targets", tg, tg_ref[:T])

        # advantages from the oracle's post-update values on its own rows
        v_after, _ = scatter_rows(
            rows, po.model_eval(val, orc.params(1), sm)[:, 0], T, N)
        adv_ref, _ = scatter_rows(rows, orc.buf(po.BUF_ADVANTAGES), T, N)
        a32 = lw.gae_f32(done, v_after, GAMMA, LAM)
        a64, S = lw.gae_f64_forward(done, v_after, GAMMA, LAM)
        close("gae_f32", a32, adv_ref[:T])
        close("gae_f64_forward", a64, adv_ref[:T])
        # the two references agree within the bound the GPU test applies
        assert np.all(np.abs(a32 - a64) <= 4 * lw.U32 * S + 1e-30)
        assert (S >= np.abs(a64)).all()
    print("T=%d" % T, {k: "%.2e" % v for k, v in worst.items()})


def test_adv_normalize_and_ulp_helpers():
    rng = np.random.default_rng(5)
    a = rng.normal(2.0, 1.5, (9, 7)).astype(np.float32)
    z = lw.adv_normalize_f64(a, a.size).astype(np.float64)
    assert abs(z.mean()) < 1e-6 and abs(z.std() - 1.0) < 1e-6
    one = np.float32(1.0)
    up = np.nextafter(one, np.float32(2.0))
    assert lw.ulp_distance_f32([one, -one, 0.0], [up, -up, -0.0]).tolist() == [1, 1, 0]
