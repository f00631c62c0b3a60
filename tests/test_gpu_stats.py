"""On-device training statistics (xh_trainer_set_stats) against a host
restatement written here in numpy.

The host check keeps its own running episode length per env across
iterations, reads BUF_DONE / BUF_POLD after each rollout() and BUF_V_STATE0 /
BUF_TARGETS / BUF_ADV / BUF_POLICY_GRADS / BUF_VALUE_GRAD / BUF_KL after each
learn(), and forms every sum with math.fsum over float64 terms.

How closely a row must match:

* the integer-valued entries (ITER, TRANSITIONS, EPISODES, EPLEN_SUM,
  EPLEN_SQSUM, REWARD_SUM) are equal;
* a floating sum of n terms satisfies
  |device - host| <= (n + 8) * 2**-52 * fsum(|terms|):
  a double sum of n terms in any order is within (n - 1) 2^-53 sum|terms| of
  the exact sum and fsum is exact; one ulp per term covers a product, about
  two a double log on each side.  The bound is derived, not measured.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def _trainer(ctx, algo="ppo", B=8, D=2, N=24, T=3, widths=(128, 64), x0=4711,
             stats=32, forced=False, **kw):
    from dependence_free_rl_amd import (POLICY, VALUE, Trainer, init_policy,
                                        init_value)
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=widths, rng_state=x0, **kw)
    tr.set_params(POLICY, init_policy(D, *widths, seed=11))
    tr.set_params(VALUE, init_value(B, D, seed=12))
    if forced:
        tr.set_forced_actions(np.zeros((T, N), np.int32))
    if stats:
        tr.set_stats(stats)
    return tr


def _fsum(terms):
    """(fsum, fsum of magnitudes, count) of float64 terms."""
    t = np.asarray(terms, np.float64).ravel().tolist()
    return math.fsum(t), math.fsum(abs(x) for x in t), len(t)


class HostStats:
    """The numpy restatement: one dict per row, {index: int} for the exact
    entries and {index: (sum, magnitude, terms)} for the floating sums."""

    def __init__(self, tr):
        self.tr = tr
        self.ep_len = np.zeros(tr.N, np.int64)
        self.rows = []
        self.ends = []  # per window: list of (slot, env, length)

    def rollout(self):
        from dependence_free_rl_amd import _lib as L
        from dependence_free_rl_amd.trainer import BUF_DONE, BUF_POLD
        done, pold = self.tr.buffer(BUF_DONE), self.tr.buffer(BUF_POLD)
        T, N = done.shape
        ends = []
        for e in range(N):
            for t in range(T):
                self.ep_len[e] += 1
                if done[t, e]:
                    ends.append((t, e, int(self.ep_len[e])))
                    self.ep_len[e] = 0
        self.ends.append(ends)
        row = {
            L.STAT_ITER: len(self.rows),
            L.STAT_TRANSITIONS: T * N,
            L.STAT_EPISODES: len(ends),
            L.STAT_EPLEN_SUM: sum(n for _, _, n in ends),
            L.STAT_EPLEN_SQSUM: sum(n * n for _, _, n in ends),
            L.STAT_REWARD_SUM: T * N - int(done.astype(np.int64).sum()),
            L.STAT_NEGLOGP_SUM: _fsum([-math.log(float(p))
                                       for p in pold.ravel()]),
        }
        self.rows.append(row)
        return row

    def learn(self):
        from dependence_free_rl_amd import _lib as L
        from dependence_free_rl_amd.trainer import (BUF_ADV, BUF_KL,
                                                    BUF_POLICY_GRADS,
                                                    BUF_TARGETS, BUF_V_STATE0,
                                                    BUF_VALUE_GRAD)
        tr, row = self.tr, self.rows[-1]
        v0 = tr.buffer(BUF_V_STATE0)[:tr.T].astype(np.float64)
        tg = tr.buffer(BUF_TARGETS).astype(np.float64)
        adv = tr.buffer(BUF_ADV).astype(np.float64)
        err = tg - v0
        pg = tr.buffer(BUF_POLICY_GRADS).astype(np.float64)
        vg = tr.buffer(BUF_VALUE_GRAD).astype(np.float64)
        row.update({
            L.STAT_VERR_SUM: _fsum(err), L.STAT_VERR_SQSUM: _fsum(err * err),
            L.STAT_TARGET_SUM: _fsum(tg), L.STAT_TARGET_SQSUM: _fsum(tg * tg),
            L.STAT_ADV_SUM: _fsum(adv), L.STAT_ADV_SQSUM: _fsum(adv * adv),
            L.STAT_PGRAD_SQ_FIRST: _fsum(pg[0] * pg[0]),
            L.STAT_PGRAD_SQ_LAST: _fsum(pg[-1] * pg[-1]),
            L.STAT_VGRAD_SQ: _fsum(vg * vg),
        })
        if tr.cfg.algo == L.XH_KLPPO:
            kl = tr.buffer(BUF_KL)
            row["kl"] = (np.float64(kl[-1, 2]), np.float64(kl[-1, 1]))
        return row


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_row(dev, host, learned=True, what=""):
    """One device row against the host row; prints every floating entry's
    error and bound before asserting."""
    from dependence_free_rl_amd import _lib as L
    assert dev.shape == (L.STAT_COUNT,)
    worst = 0.0
    for k, want in sorted((k, v) for k, v in host.items() if k != "kl"):
        if isinstance(want, tuple):
            s, mag, n = want
            bound = (n + 8) * EPS * mag
            err = abs(float(dev[k]) - s)
            print("%s entry %d: device %.17g host %.17g err %.3g bound %.3g"
                  % (what, k, dev[k], s, err, bound))
            assert err <= bound, (what, k, float(dev[k]), s, err, bound)
            worst = max(worst, err / bound if bound else 0.0)
        else:
            assert float(dev[k]) == float(want), (what, k, float(dev[k]), want)
    if not learned:
        assert np.isnan(dev[L.STAT_VERR_SUM:]).all(), (what, dev)
    elif "kl" in host:
        np.testing.assert_array_equal(
            _bits(dev[[L.STAT_KL_BETA, L.STAT_KL_MEAN]]), _bits(host["kl"]))
    else:
        assert np.isnan(dev[[L.STAT_KL_BETA, L.STAT_KL_MEAN]]).all(), (what, dev)
    return worst


def _run_checked(tr, iters, what):
    host = HostStats(tr)
    for it in range(iters):
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
    assert tr.stats_count() == iters
    rows = tr.stats()
    assert rows.shape[0] == iters
    for it in range(iters):
        check_row(rows[it], host.rows[it], what="%s it%d" % (what, it))
    return host, rows


# ------------------------------------------------- 1, 2: forced actions ----
def test_episodes_span_windows(ctx):
    """Every item into bin 0 of an 8 x (8, 8) env: an episode lasts 3 to 5
    steps, so with T = 3 every episode crosses a window edge."""
    T, N = 3, 24
    tr = _trainer(ctx, T=T, N=N, forced=True)
    host, rows = _run_checked(tr, 6, "span")
    ends = [e for w in host.ends for e in w]
    assert all(3 <= n <= 5 for _, _, n in ends), ends
    # conditions on the inputs (the seed is chosen so that they hold)
    assert any(t == T - 1 for t, _, _ in ends), "no episode ended on slot T-1"
    assert any(t == 0 for t, _, _ in ends), "no episode ended on slot 0"
    assert any(len({e for _, e, _ in w}) < N for w in host.ends), \
        "every env ended an episode in every window"
    tr.close()


def test_several_episodes_per_window(ctx):
    T, N = 12, 24
    tr = _trainer(ctx, T=T, N=N, forced=True)
    host, rows = _run_checked(tr, 6, "multi")
    per_env = np.zeros(N, np.int64)
    for _, e, _ in host.ends[1]:
        per_env[e] += 1
    assert per_env.min() >= 2 and per_env.max() <= 4, per_env
    tr.close()


# ------------------------------- 3: partial wave, workgroup boundary ----
@pytest.mark.parametrize("N", [1, 300])
def test_partial_wave_and_workgroup_boundary(ctx, N):
    tr = _trainer(ctx, B=64, D=2, N=N, T=4, widths=(128, 128))
    _run_checked(tr, 3, "n%d" % N)
    tr.close()


# ----------------------------------------- 4: each algorithm's learner ----
@pytest.mark.parametrize("algo,B,N,T,widths", [
    ("ppo", 8, 16, 4, (128, 64)),
    ("ac", 8, 16, 8, (64, 32)),
    ("klppo", 64, 16, 4, (128, 128)),
])
def test_learner_part_per_algorithm(ctx, algo, B, N, T, widths):
    from dependence_free_rl_amd import _lib as L
    tr = _trainer(ctx, algo=algo, B=B, N=N, T=T, widths=widths)
    host, rows = _run_checked(tr, 2, algo)
    kl = rows[:, [L.STAT_KL_BETA, L.STAT_KL_MEAN]]
    assert np.isfinite(kl).all() if algo == "klppo" else np.isnan(kl).all()
    curve = tr.training_curve()
    n = T * N
    np.testing.assert_allclose(curve["value_loss"],
                               rows[:, L.STAT_VERR_SQSUM] / n, rtol=1e-15)
    np.testing.assert_allclose(curve["value_grad_norm"],
                               np.sqrt(rows[:, L.STAT_VGRAD_SQ]), rtol=1e-15)
    tr.close()


def test_normalised_advantages(ctx):
    from dependence_free_rl_amd import _lib as L
    T, N = 4, 16
    tr = _trainer(ctx, B=8, N=N, T=T, adv_normalize=True)
    host, rows = _run_checked(tr, 2, "advnorm")
    curve = tr.training_curve()
    for it in range(2):
        assert abs(rows[it, L.STAT_ADV_SUM] / (T * N)) < 1e-3
        assert abs(curve["adv_mean"][it]) < 1e-3
        assert abs(curve["adv_std"][it] - 1.0) < 1e-3
    tr.close()


# ------------------------------------- 5: statistics change nothing ----
def test_statistics_change_nothing_else(ctx):
    from dependence_free_rl_amd import POLICY, VALUE
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_ADV, BUF_DONE,
                                                BUF_RNG)
    out = []
    for stats in (0, 16):
        tr = _trainer(ctx, B=8, N=16, T=4, stats=stats)
        tr.iterate(3)
        out.append([tr.params(POLICY), tr.params(VALUE)] +
                   [tr.buffer(b) for b in (BUF_ACTION, BUF_DONE, BUF_ADV,
                                           BUF_RNG)])
        tr.close()
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


# ------------------------------------ 6: asynchronous history, the ring ----
def test_async_history_and_ring(ctx):
    from dependence_free_rl_amd import XhError

    def run_async():
        tr = _trainer(ctx, B=8, N=16, T=4, stats=4)
        tr.iterate(6)  # no host call in between
        assert tr.stats_count() == 6
        rows = tr.stats()
        np.testing.assert_array_equal(_bits(rows), _bits(tr.stats(2, 4)))
        with pytest.raises(XhError, match="status 1"):  # overwritten
            tr.stats(first=0, count=1)
        with pytest.raises(XhError, match="status 1"):  # not written yet
            tr.stats(first=5, count=2)
        tr.close()
        return rows

    a, b = run_async(), run_async()
    assert a.shape[0] == 4
    np.testing.assert_array_equal(_bits(a), _bits(b))
    tr = _trainer(ctx, B=8, N=16, T=4, stats=8)
    for _ in range(6):
        tr.rollout()
        tr.learn()
    stepped = tr.stats()
    assert stepped.shape[0] == 6
    np.testing.assert_array_equal(stepped[:, 0], np.arange(6.0))
    np.testing.assert_array_equal(_bits(a), _bits(stepped[2:6]))
    tr.close()


# ------------------------------------------------------ 7: row states ----
def test_forget_leaves_the_learner_part_nan(ctx):
    tr = _trainer(ctx, T=3, N=24, forced=True)
    host = HostStats(tr)
    tr.rollout()
    host.rollout()
    check_row(tr.stats()[0], host.rows[0], learned=False, what="unconsumed")
    tr.forget()
    check_row(tr.stats()[0], host.rows[0], learned=False, what="forgotten")
    # the running lengths survive the forget() shift
    for it in (1, 2):
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
    rows = tr.stats()
    check_row(rows[0], host.rows[0], learned=False, what="forgotten, later")
    for it in (1, 2):
        check_row(rows[it], host.rows[it], what="after forget it%d" % it)
    tr.close()


def test_set_env_state_restarts_the_episode(ctx):
    from dependence_free_rl_amd import _lib as L
    T, N, B, D = 3, 8, 8, 2
    tr = _trainer(ctx, T=T, N=N, forced=True)
    host = HostStats(tr)
    for _ in range(4):  # until env 0 stands in mid-episode after a window
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
        if host.ep_len[0] > 0:
            break
    assert host.ep_len[0] > 0, "env 0 ended on the last slot of every window"
    carried = int(host.ep_len[0])
    tr.set_env_state(0, np.full((1, B, D), 8, np.int8),
                     np.array([[1, 2]], np.int8))
    host.ep_len[0] = 0  # a new episode; the replaced one is never counted
    start = len(host.rows)
    first_end = None
    for _ in range(3):
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
        ends0 = [(t, n) for t, e, n in host.ends[-1] if e == 0]
        if ends0 and first_end is None:
            first_end = (len(host.rows) - 1, ends0[0])
    rows = tr.stats()
    for it in range(len(host.rows)):
        check_row(rows[it], host.rows[it], what="replace it%d" % it)
    # env 0's next end: the length counted from the replacement -- the steps
    # since then, not those plus the replaced episode's
    assert first_end is not None
    row, (slot, length) = first_end
    assert carried > 0 and 3 <= length <= 5
    # on the device row: the window's length sum minus every other end's
    # length is env 0's, counted from the replacement
    others = sum(n for t, e, n in host.ends[row]) - length
    assert rows[row, L.STAT_EPLEN_SUM] - others == (row - start) * T + slot + 1
    tr.close()


def test_set_buffer_bins_restarts_every_episode(ctx):
    """Bin states uploaded through set_buffer(BUF_BINS) start new episodes."""
    from dependence_free_rl_amd.trainer import BUF_BINS
    T, N, B, D = 3, 8, 8, 2
    tr = _trainer(ctx, T=T, N=N, forced=True)
    host = HostStats(tr)
    tr.rollout()
    host.rollout()
    tr.learn()
    host.learn()
    assert host.ep_len.max() > 0  # some env stands in mid-episode
    tr.set_buffer(BUF_BINS, np.full((T + 1, N, B, D), 8, np.int8))
    host.ep_len[:] = 0
    for _ in range(2):
        tr.rollout()
        host.rollout()
        tr.learn()
        host.learn()
    rows = tr.stats()
    for it in range(3):
        check_row(rows[it], host.rows[it], what="upload it%d" % it)
    # every env restarted from full bins: its first end is 3 to 5 steps later
    first = {}
    for w, ends in enumerate(host.ends[1:]):
        for t, e, n in ends:
            if e not in first:
                first[e] = (w * T + t + 1, n)
    assert len(first) == N, first
    assert all(a == n and 3 <= n <= 5 for a, n in first.values()), first
    tr.close()


def test_example_prints_the_curve():
    """examples/ppo_training_curve.cc: 250 iterations of 256 envs in blocks
    of 100 print one line per block with consistent figures."""
    import os
    import re
    import subprocess
    from compat_helpers import app
    exe = app("ppo_training_curve")
    assert os.path.exists(exe), "build/compat/ppo_training_curve (make compat)"
    out = subprocess.run([exe, "250", "256"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr[-1000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("iteration")]
    assert [int(ln.split()[1]) for ln in lines] == [100, 200, 250], out.stdout
    for ln, iters in zip(lines, (100, 100, 50)):
        f = dict(re.findall(r"(\w+) ([-+0-9.eE]+|nan|inf)", ln))
        v = {k: float(x) for k, x in f.items()}
        # an episode of the 64-bin env lasts at least 3 steps and every step
        # ends at most one: bounds that hold for any policy
        assert 0 < v["episodes"] <= iters * 256 * 4 / 3, ln
        assert v["mean_return"] >= 2.0, ln
        assert 0.0 < v["entropy"] < 2 * math.log(64), ln
        assert v["value_loss"] > 0 and v["explained_variance"] <= 1.0, ln
        assert v["policy_grad_norm"] > 0 and v["value_grad_norm"] > 0, ln


def test_stats_off_and_reinforce(ctx):
    from dependence_free_rl_amd import Trainer, XhError
    tr = _trainer(ctx, B=8, N=16, T=4, stats=8)
    tr.iterate(1)
    assert tr.stats().shape[0] == 1
    tr.set_stats(0)
    with pytest.raises(XhError, match="status 4"):  # XH_ERR_STATE
        tr.stats()
    tr.iterate(1)  # and the default path runs on
    tr.set_stats(8)  # restarts at row 0, every running length at zero
    assert tr.stats_count() == 0
    tr.close()
    pg = Trainer(ctx, algo="pg", bins=8, dims=2, num_envs=8, steps=1,
                 widths=(32, 0))
    with pytest.raises(XhError, match="status 1"):  # XH_ERR_INVALID
        pg.set_stats(8)
    pg.close()


# --------------------------------- 8: the all-reduce path on one device ----
def test_one_rank_communicator_rows_are_identical(ctx):
    from dependence_free_rl_amd import Context
    rc = Context(device=0, rank=0, world=1, uid=Context.unique_id())
    try:
        out = []
        for c in (ctx, rc):
            tr = _trainer(c, B=8, N=16, T=4, stats=8)
            tr.iterate(3)
            out.append(tr.stats())
            tr.close()
    finally:
        rc.close()
    assert out[0].shape[0] == 3
    np.testing.assert_array_equal(_bits(out[0]), _bits(out[1]))
