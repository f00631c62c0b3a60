"""The 64-bin 2-D [128,128] rollout on its logit table
(dependence_free_rl_amd/csrc/policy_kernels.hip: build_logit_table and the
table build of rollout_split_kernel, xh_logit_table.h): the
per-bin policy is a function of (bin state, item), 289 states x 2 items, so a
launch computes those 578 logits once with the rollout's own forward and every
env-step reads its 64 from the table.

Bit identity is the yardstick: every case runs the default path and
XH_ROLLOUT_TABLE=0 (the per-row forward) in the same process and compares for
exact equality every window's bins (all T + 1 slots), actions, p_old and done
flags, the last step's recorded logits and probabilities, the env state the
next window starts from, and after the iterations both nets' parameters and
the state digests.  The learn() is a deterministic function of the batch, so
any difference is the rollout's.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, D, WIDTHS = 64, 2, (128, 128)
X0 = 4711
KERNEL = "rollout_split_kernel"
ITEMS = np.array([[4, 2], [1, 2]], np.int8)  # the 2-D item table (item_a, item_b)
CAP = 8

_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    return init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)


def _env(monkeypatch, table, e0=None):
    for k, v in (("XH_ROLLOUT_TABLE", table), ("XH_E0_REUSE", e0)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(ctx, monkeypatch, table, algo="ppo", N=48, T=4, iters=1, e0=None, states=None,
         forced=None, upd_diag=False, learn=True, cache=True):
    """`iters` iterations (rollout, learn) of a fresh trainer; every window's
    buffers, then the parameters and digests.  states: {env: (bins, item)} set
    into slot 0 before the first rollout; learn=False: one rollout only."""
    skey = None if states is None else b"".join(
        bytes([e]) + b.tobytes() + i.tobytes() for e, (b, i) in sorted(states.items()))
    key = (table, algo, N, T, iters, e0, skey, None if forced is None else forced.tobytes(),
           upd_diag, learn)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_BINS, BUF_DONE, BUF_LOGITS,
                                                BUF_POLD, BUF_PROBS, BUF_QOLD)
    _env(monkeypatch, table, e0)
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0, record_last_step=True)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if upd_diag:
        tr.set_update_diag(4)
    if states:
        for e, (bins, item) in states.items():
            tr.set_env_state(e, bins[None], item[None])
    if forced is not None:
        tr.set_forced_actions(forced)
    out = {"windows": [], "flags": [], "kernels": []}
    for _ in range(iters):
        tr.rollout()
        k = tr.kernel_info()["rollout_step"]
        out["flags"].append(k["logit_table"])
        out["kernels"].append(k["kernel"])
        w = {"bins": tr.buffer(BUF_BINS), "action": tr.buffer(BUF_ACTION),
             "pold": tr.buffer(BUF_POLD), "done": tr.buffer(BUF_DONE),
             "logits": tr.buffer(BUF_LOGITS), "probs": tr.buffer(BUF_PROBS)}
        if algo == "klppo":
            w["qold"] = tr.buffer(BUF_QOLD)
        out["windows"].append(w)
        if learn:
            tr.learn()
    out["env_state"] = tr.env_state() if learn else None
    out["pp"], out["vp"] = tr.params(POLICY), tr.params(VALUE)
    out["digest"] = tr.state_digest()
    tr.close()
    if cache:
        _runs[key] = out
    return out


def _same(a, b):
    assert len(a["windows"]) == len(b["windows"])
    for i, (wa, wb) in enumerate(zip(a["windows"], b["windows"])):
        assert wa.keys() == wb.keys()
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k], err_msg="window %d %s" % (i, k))
            if wa[k].dtype.kind == "f":  # the bits, not only the values
                np.testing.assert_array_equal(wa[k].view(np.uint32), wb[k].view(np.uint32),
                                              err_msg="window %d %s bits" % (i, k))
    if a["env_state"] is not None:
        for x, y in zip(a["env_state"], b["env_state"]):
            np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a["pp"].view(np.uint32), b["pp"].view(np.uint32))
    np.testing.assert_array_equal(a["vp"].view(np.uint32), b["vp"].view(np.uint32))
    assert a["digest"] == b["digest"]


def _pair(ctx, monkeypatch, want_table=True, **kw):
    new = _run(ctx, monkeypatch, None, **kw)
    old = _run(ctx, monkeypatch, 0, **kw)
    assert new["flags"] == [want_table] * len(new["flags"]), new["flags"]
    assert old["flags"] == [False] * len(old["flags"]), old["flags"]
    assert new["kernels"] == old["kernels"]
    _same(new, old)
    return new, old


def _dones(run):
    return int(sum(int(w["done"].sum()) for w in run["windows"]))


@pytest.mark.parametrize("N,T,iters,need_done", [
    (48, 4, 8, True),    # the headline window
    (48, 9, 4, True),    # longer than 8 steps: the slot-T shift and resets
    (1, 4, 2, False),    # one wave has work
    (300, 4, 2, False),  # workgroups own more than one group
])
def test_ppo(ctx, monkeypatch, N, T, iters, need_done):
    new, _ = _pair(ctx, monkeypatch, algo="ppo", N=N, T=T, iters=iters)
    assert new["kernels"] == [KERNEL] * iters
    nd = _dones(new)
    print("rollout table ppo N=%d T=%d: %d resets over %d iterations" % (N, T, nd, iters))
    if need_done:
        assert nd >= 1


# ---- every table entry: slot 0 covers [-8, 8]^2 under both items
def _all_states():
    st = np.array([(a, b) for a in range(-CAP, CAP + 1) for b in range(-CAP, CAP + 1)], np.int8)
    assert len(st) == 289
    rng = np.random.RandomState(7)
    rows = np.concatenate([np.arange(289), rng.randint(0, 289, 5 * B - 289)])
    grid = st[rng.permutation(rows)].reshape(5, B, D)
    out = {}
    for item in range(2):
        for e in range(5):
            out[5 * item + e] = (grid[e], ITEMS[item])
        got = {tuple(x) for e in range(5) for x in grid[e]}
        assert len(got) == 289
    return out


ALL_STATES = _all_states()
FORCED = np.random.RandomState(11).randint(0, B, (4, 10)).astype(np.int32)


def test_every_entry_recorded(ctx, monkeypatch):
    """T = 1: the recorded logits are slot 0's, one per (state, item)."""
    new, _ = _pair(ctx, monkeypatch, N=10, T=1, states=ALL_STATES, learn=False)
    bins = new["windows"][0]["bins"][0]
    for e, (st, _) in ALL_STATES.items():
        np.testing.assert_array_equal(bins[e], st)
    assert np.isfinite(new["windows"][0]["logits"]).all()


def test_every_entry_forced(ctx, monkeypatch):
    new, _ = _pair(ctx, monkeypatch, N=10, T=4, states=ALL_STATES, forced=FORCED, learn=False)
    np.testing.assert_array_equal(new["windows"][0]["action"], FORCED)


def test_wide_slot_runs_f32(ctx, monkeypatch):
    """A bin below -capacity: the f32 kernel on both sides, no table."""
    st = {e: (b.copy(), i) for e, (b, i) in ALL_STATES.items()}
    st[3][0][17, 1] = -CAP - 1
    new, _ = _pair(ctx, monkeypatch, want_table=False, N=10, T=1, states=st, learn=False)
    assert new["kernels"] != [KERNEL]


def test_wide_bin_persists_and_keeps_forward(ctx, monkeypatch):
    """T = 4 from a slot 0 with bins below -capacity that the forced actions
    never take: slot 0 runs on the f32 kernel, and the bins stay, outside the
    table's domain, through slots 1-3 and into the next window, whose slot 0
    carries no `wide` mark.  A trainer that has seen such a slot 0 keeps the
    per-row forward from then on (RolloutArgs::wide_seen)."""
    st = {e: (b.copy(), i) for e, (b, i) in ALL_STATES.items()}
    forced = FORCED.copy()
    for e, k in ((3, 17), (8, 40)):
        st[e][0][k] = (-40, -CAP - 1)
        # these two envs never end: step t takes bin t, full at the start (two
        # windows subtract at most (4, 2) twice from it)
        st[e][0][:4] = (CAP, CAP)
        forced[:, e] = np.arange(4)
    new, _ = _pair(ctx, monkeypatch, want_table=False, N=10, T=4, iters=2, states=st,
                   forced=forced)
    assert new["kernels"] == [KERNEL] * 2
    assert not any(w["done"][:, (3, 8)].any() for w in new["windows"])
    for w in new["windows"]:
        assert (w["bins"][:, 3, 17] == (-40, -CAP - 1)).all()
        assert (w["bins"][:, 8, 40] == (-40, -CAP - 1)).all()


# ---- the other paths
def test_actor_critic(ctx, monkeypatch):
    _pair(ctx, monkeypatch, algo="ac", N=48, T=4, iters=2)


def test_klppo_with_distributions(ctx, monkeypatch):
    new, _ = _pair(ctx, monkeypatch, algo="klppo", N=48, T=4, iters=2)
    assert "qold" in new["windows"][0]


def test_e0_reuse_keeps_forward(ctx, monkeypatch):
    """XH_E0_REUSE=2 reads the relu masks of every row: the E0 launch."""
    _pair(ctx, monkeypatch, want_table=False, N=48, T=4, iters=2, e0=2)


def test_update_diag_keeps_forward(ctx, monkeypatch):
    _pair(ctx, monkeypatch, want_table=False, N=48, T=4, iters=2, upd_diag=True)


def test_deterministic(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, None, N=48, T=4, iters=8)
    b = _run(ctx, monkeypatch, None, N=48, T=4, iters=8, cache=False)
    assert a["flags"] == [True] * 8
    _same(a, b)
