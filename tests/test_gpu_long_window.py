"""Rollout windows longer than 8 steps: gae_kernel's chunks of 8, the three
end-row list kernels and the in-register rollouts, each link on its own.

(a) teacher-forced windows of 9 and 17 steps against the CPU oracle run in
    lockstep: env states, items, dones and engine states bit for bit, p_old,
    V, advantages and the value gradient within conftest.RTOL;
(b) the learner's chain from the device's own buffers against the host
    references of long_window_ref.py (pinned to the oracle by
    test_long_window_ref.py): v_state0 and v_term against the float64 value
    net, targets and advantages bit for bit against the float32 restatements
    of their kernels (gae_f32 has no chunks: chunking must not change a bit),
    advantages within 4 u S_t of the reference's float64 forward sum;
(c) the episode statistics with several episodes per env per window;
(d) PPO's epoch 0 on the rollout's outputs at a 17-step window.

Every item goes into bin 0 (forced action 0) unless a case says otherwise: an
episode lasts 3 to 5 steps, so about a quarter of the transitions are terminal
and an env ends two or three episodes in 9 steps (two of 5 steps do not fit:
the lockstep cases run from an engine state for which every env ends at least
two in both windows; the batches of hundreds of envs ask it of most envs).
long_window_ref.assert_dense asserts this on the device's own done flags.
"""
import numpy as np
import pytest

import long_window_ref as lw
from conftest import RTOL, assert_close, log_record

pytestmark = pytest.mark.gpu

GAMMA, LAM = 0.99, 0.95
# engine states for which every env ends two episodes in both windows of every
# lockstep case (also at T = 9), and for which the free-running policy ends
# episodes on both sides of a chunk edge (both found with the CPU oracle)
X0 = 31
EDGE_X0 = 186
LOG = "long_window.jsonl"


def _params(B, D, widths):
    from dependence_free_rl_amd import init_policy
    # V of order 1, different from state to state (long_window_ref)
    return init_policy(D, *widths, seed=3), lw.value_params(B, D)


def _trainer(ctx, B, D, widths, N, T, algo="ppo", forced=True, x0=X0, **kw):
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=widths, rng_state=x0, gamma=GAMMA, lam=LAM, **kw)
    pp, vp = _params(B, D, widths)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if forced:
        tr.set_forced_actions(np.zeros((T, N), np.int32))
    return tr


# ------------------------------------------- (a) lockstep with the oracle ----
LOCKSTEP = [
    # algo, B, D, widths, N, T, the rollout kernel the shape runs
    ("ppo", 8, 2, (128, 64), 8, 9, "rollout_step_kernel"),
    ("ppo", 8, 2, (128, 64), 8, 17, "rollout_step_kernel"),
    ("ppo", 32, 1, (64, 64), 8, 17, "rollout_split_kernel"),
    ("ppo", 64, 2, (128, 128), 4, 17, "rollout_split_kernel"),
    ("ac", 128, 3, (128, 128), 4, 9, "rollout_split128_kernel"),
]


@pytest.mark.parametrize("algo,B,D,widths,N,T,kernel", LOCKSTEP)
def test_teacher_forced_long_window_matches_oracle(ctx, algo, B, D, widths, N,
                                                   T, kernel):
    """Two consecutive windows, every item into bin 0: several resets per env
    inside one launch of the register-stepping rollouts, the second window
    from slot T and the jumped stream states.  Bit-exact env transitions and
    engine states; p_old, V (transition rows and, through v_term, terminal
    end rows), advantages and the value gradient within RTOL of the oracle's
    learn() on the same parameters."""
    from dependence_free_rl_amd.trainer import (BUF_ADV, BUF_BINS, BUF_DONE,
                                                BUF_ITEMS, BUF_POLD, BUF_RNG,
                                                BUF_V_STATE0, BUF_V_TERM,
                                                BUF_VALUE_GRAD, POLICY, VALUE)
    from gpu_helpers import default_lr
    from oracle import pyoracle as po
    from test_long_window_ref import oracle_rows, scatter_rows, window_buffers
    tr = _trainer(ctx, B, D, widths, N, T, algo=algo)
    pp, vp = _params(B, D, widths)
    head = po.OR_SOFTMAX_XENT if algo == "ac" else po.OR_SOFTMAX
    orc = po.Trainer({"ppo": po.OR_PPO, "ac": po.OR_AC}[algo], B, D, N, T,
                     po.perbin_model(2 * D, list(widths), head), pp,
                     po.full_model(B * 2 * D, [64, 32], 1), vp,
                     lr_pi=default_lr(algo, 0), lr_v=default_lr(algo, 1),
                     gamma=GAMMA, x0=X0)
    worst = {}

    def close(what, x, y):
        worst[what] = max(worst.get(what, 0.0), assert_close(x, y, what=what))

    for it in range(2):
        w = "%s b%dd%d N%d T%d it%d " % (algo, B, D, N, T, it)
        # the oracle learns from the device trainer's own parameters
        orc.set_params(0, tr.params(POLICY))
        orc.set_params(1, tr.params(VALUE))
        tr.rollout()
        assert tr.kernel_info()["rollout_step"]["kernel"] == kernel
        orc.rollout(forced=np.zeros((N, T), np.int32))
        obins, oitems, _, odone = window_buffers(orc, T)
        done = tr.buffer(BUF_DONE)
        np.testing.assert_array_equal(tr.buffer(BUF_BINS), obins, err_msg=w)
        np.testing.assert_array_equal(tr.buffer(BUF_ITEMS)[:, :, :D], oitems,
                                      err_msg=w)
        np.testing.assert_array_equal(done, odone, err_msg=w)
        lw.assert_dense(done, w)
        # per-env engine states: reference-order positions
        rng = tr.buffer(BUF_RNG)
        for e in range(N):
            assert rng[e] == po.minstd_jump(X0, 2 * N + 4 * T * N * (it + 1)
                                            + 4 * T * e), (w, e)
            assert rng[e] == po.minstd_jump(orc.rng, 4 * T * e), (w, e)
        close("p_old", tr.buffer(BUF_POLD),
              orc.buf(po.BUF_STEP_PCHOICE).reshape(N, T).T)
        tr.learn()
        orc.learn()
        rows = oracle_rows(orc, it, T, done)
        ov, ovt = scatter_rows(rows, orc.buf(po.BUF_VALUES), T, N)
        oadv, _ = scatter_rows(rows, orc.buf(po.BUF_ADVANTAGES), T, N)
        ended = done != 0
        assert int(ended.sum()) == sum(k == 2 for k, _, _ in rows)
        lw.assert_values_differ(ovt[ended], RTOL, w + "v_term")
        close("V transition rows", tr.buffer(BUF_V_STATE0)[:T], ov[:T])
        close("V terminal end rows", tr.buffer(BUF_V_TERM)[ended], ovt[ended])
        close("advantages", tr.buffer(BUF_ADV), oadv[:T])
        close("value_grad", tr.buffer(BUF_VALUE_GRAD),
              orc.buf(po.BUF_VALUE_GRAD))
    log_record(LOG, {"test": "lockstep", "algo": algo, "B": B, "D": D, "N": N,
                     "T": T, "kernel": kernel, "max_scaled_err": worst})
    print(w, {k: "%.2e" % v for k, v in worst.items()})
    tr.close()


# ------------------------------ (b) the chain from the device's buffers ----
def end_list_form(N):
    """launch_end_list's choice (kl_kernels.hip), restated."""
    if N % 4 == 0 and N <= 8192:
        return "end_list_kernel<4>" if N <= 4096 else "end_list_kernel<8>"
    return "three passes, %d blocks" % ((N + 255) // 256)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_chain(tr, what, normalized=False):
    """One rollout() + learn() of `tr`, every link of the learner's value /
    advantage chain checked from the device's own buffers.  Returns the
    record it logs (figures first, then the assertions)."""
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_ADV, BUF_BINS,
                                                BUF_DONE, BUF_ITEMS,
                                                BUF_TARGETS, BUF_V_STATE,
                                                BUF_V_STATE0, BUF_V_TERM, VALUE)
    T, N, B, D = tr.T, tr.N, tr.B, tr.D
    vp = tr.params(VALUE)  # the parameters before the value step
    tr.rollout()
    tr.learn()
    bins, items = tr.buffer(BUF_BINS), tr.buffer(BUF_ITEMS)
    action, done = tr.buffer(BUF_ACTION), tr.buffer(BUF_DONE)
    v0, vt = tr.buffer(BUF_V_STATE0), tr.buffer(BUF_V_TERM)
    tg, vs, adv = (tr.buffer(BUF_TARGETS), tr.buffer(BUF_V_STATE),
                   tr.buffer(BUF_ADV))
    ended = done != 0
    share, per_env = lw.density(done)
    rec = {"test": "chain", "what": what, "B": B, "D": D, "N": N, "T": T,
           "end_list": end_list_form(N), "n_end": int(ended.sum()),
           "terminal_share": round(share, 4),
           "episodes_per_env": [int(per_env.min()), int(per_env.max())]}
    # V(S_0..S_T) and V(E_t) against the float64 value net: a misplaced or
    # missing end-list entry leaves a v_term entry of an ended transition
    # with another state's value (or a stale one)
    v0_ref = lw.value_f64(vp, lw.obs_f64(
        bins.reshape(-1, B, D), items.reshape(-1, 4))).reshape(T + 1, N)
    tq, eq, eb, ei = lw.terminal_views(bins, items, action, done)
    vt_ref = lw.value_f64(vp, lw.obs_f64(eb, ei))
    assert np.isfinite(v0).all() and np.isfinite(vt[tq, eq]).all()
    lw.assert_values_differ(vt_ref, RTOL, what + " v_term")
    lw.assert_values_differ(v0_ref, RTOL, what + " v_state0")
    # the float32 restatements, from the device's own inputs of each kernel
    tg_ref = lw.td_targets_f32(done, v0, vt, GAMMA)
    a32 = lw.gae_f32(done, vs, GAMMA, LAM)
    a64, S = lw.gae_f64_forward(done, vs, GAMMA, LAM)
    if normalized:
        a32n = lw.adv_normalize_f64(a32, T * N)
        ulps = lw.ulp_distance_f32(adv, a32n)
        rec["adv_normalized_max_ulp"] = int(ulps.max())
    else:
        rec["adv_bit_equal"] = bool(np.array_equal(_bits(adv), _bits(a32)))
        bound = 4 * lw.U32 * S + 1e-30
        rec["adv_f64_bound_ratio"] = float((np.abs(adv - a64) / bound).max())
    rec["targets_bit_equal"] = bool(np.array_equal(_bits(tg), _bits(tg_ref)))
    rec["v_state0_err"] = float((np.abs(v0 - v0_ref)
                                 / np.maximum(1.0, np.abs(v0_ref))).max())
    if len(tq):
        rec["v_term_err"] = float((np.abs(vt[tq, eq] - vt_ref)
                                   / np.maximum(1.0, np.abs(vt_ref))).max())
    log_record(LOG, rec)
    print(rec)
    assert_close(v0, v0_ref, what=what + " v_state0")
    assert_close(vt[tq, eq], vt_ref, what=what + " v_term")
    np.testing.assert_array_equal(_bits(tg), _bits(tg_ref),
                                  err_msg=what + " targets")
    if normalized:
        # the device's double sums run in another order: a rounding boundary
        # of the one final rounding may fall the other way
        assert ulps.max() <= 1, (what, int(ulps.max()))
    else:
        np.testing.assert_array_equal(_bits(adv), _bits(a32),
                                      err_msg=what + " advantages")
        assert rec["adv_f64_bound_ratio"] <= 1.0, (what, rec)
    return rec, done, adv


@pytest.mark.parametrize("T", [1, 7, 8, 9, 15, 16, 17, 33])
def test_chain_T_sweep(ctx, T):
    """gae_kernel's chunking: one partial chunk, an exact one, a tail of one
    step behind a full chunk, two chunks, two chunks and a tail, four and a
    tail."""
    tr = _trainer(ctx, 8, 2, (128, 64), 16, T)
    _, done, _ = check_chain(tr, "sweep T%d" % T)
    if T >= 9:
        lw.assert_dense(done, "sweep T%d" % T, every_env=False)
    tr.close()


def test_chain_terminal_on_chunk_edge(ctx):
    """Free-running policy, T = 17: the chunks are t = 16..9, 8..1 and 0.
    Some env ends an episode at t = T - 9 (the first step of the second
    chunk: A restarts there instead of taking the first chunk's carry) and
    some env at t = T - 8 (the last step of the first chunk: the carry into
    the second chunk is that step's A = delta)."""
    T, N = 17, 64
    tr = _trainer(ctx, 8, 2, (128, 64), N, T, forced=False, x0=EDGE_X0)
    _, done, _ = check_chain(tr, "chunk edge")
    assert done[T - 9].any() and done[T - 8].any(), (
        done[T - 9].sum(), done[T - 8].sum())
    tr.close()


def test_chain_T1024_and_range(ctx):
    """The top of the range of steps: 128 chunks; steps = 1025 is refused
    with XH_ERR_INVALID (status 1)."""
    from dependence_free_rl_amd import Trainer
    from dependence_free_rl_amd._lib import XhError
    tr = _trainer(ctx, 8, 2, (128, 64), 8, 1024)
    _, done, _ = check_chain(tr, "T1024")
    lw.assert_dense(done, "T1024")
    tr.close()
    with pytest.raises(XhError, match=r"status 1: steps 1025 not in \[1,1024\]"):
        Trainer(ctx, algo="ppo", bins=8, dims=2, num_envs=8, steps=1025,
                widths=(128, 64))


def test_chain_two_gae_blocks_and_normalisation(ctx):
    """N = 264 at T = 9: two gae blocks, the second with 8 of 256 lanes in
    range.  Again with adv_normalize: the block partials, their reduction
    and the one final rounding, within one float32 ulp of the float64
    normalisation of the float32 advantages; the statistics' advantage sums
    within 1e-12 of the exact float64 sums of the buffer (relative to the sum
    where every term has one sign, to the sum of magnitudes for the
    normalised advantages' sum, which cancels to about zero)."""
    import math

    from dependence_free_rl_amd import _lib as L
    T, N = 9, 264
    plain = _trainer(ctx, 8, 2, (128, 64), N, T)
    plain.set_stats(4)
    _, done, adv = check_chain(plain, "N264")
    lw.assert_dense(done, "N264", every_env=False)
    norm = _trainer(ctx, 8, 2, (128, 64), N, T, adv_normalize=True)
    norm.set_stats(4)
    _, done_n, adv_n = check_chain(norm, "N264 normalised", normalized=True)
    np.testing.assert_array_equal(done_n, done)
    for tr, a, what in ((plain, adv, "plain"), (norm, adv_n, "normalised")):
        row = tr.stats()[0]
        x = a.astype(np.float64).ravel().tolist()
        s1, s2 = math.fsum(x), math.fsum(v * v for v in x)
        mag = math.fsum(abs(v) for v in x)
        scale = mag if what == "normalised" else abs(s1)
        e1 = abs(row[L.STAT_ADV_SUM] - s1) / scale
        e2 = abs(row[L.STAT_ADV_SQSUM] - s2) / s2
        log_record(LOG, {"test": "adv sums", "what": what, "sum_rel": e1,
                         "sqsum_rel": e2, "sum_over_magnitude": abs(s1) / mag})
        print("adv sums", what, e1, e2)
        assert e1 <= 1e-12 and e2 <= 1e-12, (what, e1, e2)
        tr.close()


@pytest.mark.parametrize("B,D,widths,N,form", [
    (8, 2, (128, 64), 4104, "end_list_kernel<8>"),
    (8, 2, (128, 64), 4096, "end_list_kernel<4>"),   # every thread loaded
    (32, 1, (64, 64), 774, "three passes, 4 blocks"),  # N % 4 == 2, last partial
    (8, 2, (128, 64), 8200, "three passes, 33 blocks"),  # N % 4 == 0, > 8192
])
def test_chain_end_list_forms(ctx, B, D, widths, N, form):
    """Each implementation of the end-row list with per-env counts of 2 or 3
    at T = 9 and about a quarter of the T N transitions listed: v_term of
    every ended transition must be V of that transition's terminal view."""
    assert end_list_form(N) == form
    tr = _trainer(ctx, B, D, widths, N, 9)
    rec, done, _ = check_chain(tr, "end list N%d" % N)
    lw.assert_dense(done, "end list N%d" % N, every_env=False)
    tr.close()


# ------------------------------------------------ (c) episode statistics ----
def test_episode_statistics_long_window(ctx):
    """N = 16, T = 17, three windows, every item into bin 0: four or five
    episodes per env per window, their lengths carried across the window
    edges.  The integer statistics equal the numpy walk of the done buffers;
    the floating sums are held to test_gpu_stats.py's bound."""
    from dependence_free_rl_amd import _lib as L
    from test_gpu_stats import HostStats, check_row
    T, N = 17, 16
    tr = _trainer(ctx, 8, 2, (128, 64), N, T)
    tr.set_stats(8)
    host = HostStats(tr)
    for it in range(3):
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
    rows = tr.stats()
    assert rows.shape[0] == 3
    worst = 0.0
    for it in range(3):
        worst = max(worst, check_row(rows[it], host.rows[it],
                                     what="long window it%d" % it))
        per_env = np.bincount([e for _, e, _ in host.ends[it]], minlength=N)
        assert per_env.min() >= 2, per_env
        assert rows[it, L.STAT_EPISODES] == len(host.ends[it]) >= 0.15 * T * N
    # an episode that crossed a window edge was counted with its whole length
    assert any(n > t + 1 for w in host.ends[1:] for t, _, n in w)
    log_record(LOG, {"test": "episode statistics", "N": N, "T": T,
                     "worst_bound_ratio": worst})
    tr.close()


# ------------------------------------------- (d) epoch-0 reuse, T = 17 ----
def test_e0_reuse_long_window(ctx, monkeypatch):
    """64 bins 2-D (128, 128), PPO, N = 3, T = 17: the records of a 17-slot
    split rollout feed epoch 0.  test_gpu_e0_reuse.py's assertion between
    XH_E0_REUSE=2 and XH_E0_REUSE=0 on the same data, at this shape."""
    import test_gpu_e0_reuse as e0
    e0.test_e0_vs_oracle_and_switched_off(ctx, monkeypatch, 3, 17, 0)
