"""The lean table kernels of the config-3 PPO / actor-critic epochs
(dependence_free_rl_amd/csrc/table_mm_kernels.hip, table_tile_layout.h;
DESIGN.md §3.0e, "the epoch on the table"): the table's forward and backward on
the exact f32 MFMA, one workgroup per tile of entries, G summed from the
streaming pass's per-workgroup sums inside the backward.

Shape: 64 bins, 2-D, [128,128], the seeds and parameters of
test_gpu_train_table.py (whose runner, oracle and mixed batch this file uses).
Three paths run the same inputs: the default (the lean kernels), the table's
former launches (XH_TRAIN_TABLE=spec8) and the packed launches
(XH_TRAIN_TABLE=0).

Measured on MI355X, epoch-0 p99 units against the oracle, lean / former: PPO
N1 T1 0.839 / 0.839, N7 T3 8.15 / 8.74, N48 T4 18.9 / 17.7 (the same at
train_grid_cap 1, 5, 17), actor-critic N48 T4 22.5 / 19.2; medians 0.19-0.23 /
0.13-0.19.  Every entry live, relative L2 from XH_TRAIN_KERNEL=f32: PPO
1.6e-7 / 2.9e-7, actor-critic 1.3e-7 / 1.7e-7.  Every case prints its figures
before it asserts.
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units, grad_units
from test_gpu_train_table import (B, D, FN, FT, KERNEL, MIXED, RAN, WIDTHS, X0, _oracle,
                                  _params, _rel_l2, _run, _same)

pytestmark = pytest.mark.gpu

SPEC8 = "spec8"
ITEM_A, ITEM_B = (4, 2), (1, 2)
STATES = [(a, b) for a in range(-8, 9) for b in range(-8, 9)]  # lt::state_index order


def _units(run, ref, mag, ep=0):
    npi = run["grads"].shape[1]
    u, _, _ = grad_units(run["grads"][ep], ref.reshape(-1, npi)[ep], mag.reshape(-1, npi)[ep])
    return float(np.percentile(u, 99)), float(np.median(u))


def _check(ctx, monkeypatch, algo, N, T, cap):
    """Every epoch within conftest's budgets; epoch 0's p99 units within the
    rule between kernels of the former launches'; the reports unchanged."""
    ref, mag = _oracle(algo, N, T)
    new = _run(ctx, monkeypatch, algo, N, T, cap)
    old = _run(ctx, monkeypatch, algo, N, T, cap, table=SPEC8)
    assert new["table"] == [RAN] and old["table"] == [RAN], (new["table"], old["table"])
    assert new["pack"] == old["pack"] and new["pack"][0]["packed"] == N * T
    assert new["info"] == old["info"], (new["info"], old["info"])
    assert new["info"]["policy_train"]["kernel"] == KERNEL
    grid = new["info"]["train_grid"]
    if cap:
        assert grid == min(cap, N * T)
    g = new["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape and np.isfinite(g).all() and np.isfinite(new["params"]).all()
    p_new, med_new = _units(new, ref, mag)
    p_old, med_old = _units(old, ref, mag)
    print("table_mm %s N=%d T=%d grid=%d: epoch-0 p99 units %.3g (former %.3g), median %.3g "
          "(former %.3g)" % (algo, N, T, grid, p_new, p_old, med_new, med_old))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="table_mm %s N%d T%d grid=%d epoch%d" % (algo, N, T, grid, ep),
                          **budget)
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


# ---- small shapes
@pytest.mark.parametrize("N,T", [(1, 1), (7, 3), (48, 4)])
def test_small_shapes_ppo(ctx, monkeypatch, N, T):
    _check(ctx, monkeypatch, "ppo", N, T, 0)


def test_small_shapes_actor_critic(ctx, monkeypatch):
    _check(ctx, monkeypatch, "ac", 48, 4, 0)


# ---- tail and nparts: the stream's grid below 16 and no multiple of 16
@pytest.mark.parametrize("cap", [1, 5, 17])
def test_nparts(ctx, monkeypatch, cap):
    _check(ctx, monkeypatch, "ppo", 48, 4, cap)


# ---- every entry live
def _all_entries():
    """Ten envs, one step: envs 0-4 hold item_a, 5-9 item_b; env k of an item
    holds states 64 k .. 64 k + 63 of the 289 (the last: the remaining 33,
    repeated), so the batch carries all 578 entries, every env-step a wide
    group."""
    bins, items = {}, {}
    for e in range(10):
        k = e % 5
        idx = np.arange(64 * k, 64 * k + 64)
        if k == 4:
            idx = 256 + np.arange(64) % 33
        bins[e] = np.array([STATES[i] for i in idx], np.int8)
        items[e] = np.array(ITEM_A if e < 5 else ITEM_B, np.int8)
    seen = {(e // 5,) + tuple(s) for e in bins for s in bins[e]}
    assert len(seen) == 578
    return bins, items


_live = {}


def _run_live(ctx, monkeypatch, algo, table=None, kernel=None):
    key = (algo, table, kernel)
    if key in _live:
        return _live[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    for k, v in (("XH_TRAIN_TABLE", table), ("XH_TRAIN_KERNEL", kernel)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))
    monkeypatch.delenv("XH_SP8_PACK", raising=False)
    monkeypatch.setenv("XH_E0_REUSE", "0")
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=10, steps=1, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    bins, items = _all_entries()
    for e in range(10):
        tr.set_env_state(e, bins[e][None], items[e][None])
    tr.rollout()
    tr.learn()
    npi = tr.num_params(POLICY)
    out = {"table": tr.table_stats(), "pack": tr.pack_stats(),
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy()}
    tr.close()
    _live[key] = out
    return out


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_every_entry_live(ctx, monkeypatch, algo):
    new = _run_live(ctx, monkeypatch, algo)
    old = _run_live(ctx, monkeypatch, algo, table=SPEC8)
    f32 = _run_live(ctx, monkeypatch, algo, kernel="f32")
    assert new["table"] == RAN and old["table"] == RAN, (new["table"], old["table"])
    assert not f32["table"]["ran"]
    # ten env-steps of 64 distinct states: wide groups all
    assert new["pack"]["unpacked"] == 10 and new["pack"]["packed"] == 0, new["pack"]
    assert np.isfinite(new["grads"]).all() and np.abs(new["grads"][0]).max() > 0
    e_new = _rel_l2(new["grads"][0], f32["grads"][0])
    e_old = _rel_l2(old["grads"][0], f32["grads"][0])
    print("table_mm every entry %s: epoch-0 rel L2 lean-f32 %.3g, former-f32 %.3g"
          % (algo, e_new, e_old))
    assert e_new <= 2.0 * e_old, (e_new, e_old)


# ---- the bound is still computed where something reads it
def test_e0_reuse_keeps_the_bound(ctx, monkeypatch):
    """XH_E0_REUSE=2: epoch 0 on the e0 kernel, which scales by the bound on
    |g|; bit for bit the packed learn()'s epoch 0."""
    new = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=2)
    off = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=2, table=0)
    assert new["table"] == [RAN] and not off["table"][0]["ran"]
    np.testing.assert_array_equal(new["grads"][0], off["grads"][0])
    ref, mag = _oracle("ppo", 48, 4)
    npi = new["grads"].shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    for ep in range(1, new["grads"].shape[0]):
        assert_grad_units(new["grads"][ep], r[ep], m[ep], what="table_mm e0=2 epoch%d" % ep,
                          p99_units=GRAD_UNITS_P99_DRIFT)


def test_former_launches_and_packed_still_run(ctx, monkeypatch):
    """The switch: spec8 runs on the table (twice the same bits), 0 does not."""
    old = _run(ctx, monkeypatch, "ppo", 48, 4, 0, table=SPEC8)
    again = _run(ctx, monkeypatch, "ppo", 48, 4, 0, table=SPEC8, cache=False)
    off = _run(ctx, monkeypatch, "ppo", 48, 4, 0, table=0)
    assert old["table"] == [RAN] and not off["table"][0]["ran"]
    _same(old, again)


# ---- determinism
def test_deterministic(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, "ppo", 48, 4, 0)
    b = _run(ctx, monkeypatch, "ppo", 48, 4, 0, cache=False)
    assert a["table"] == [RAN] and b["table"] == [RAN]
    _same(a, b)


def test_deterministic_mixed(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, "ppo", FN, FT, 0, states=MIXED)
    b = _run(ctx, monkeypatch, "ppo", FN, FT, 0, states=MIXED, cache=False)
    assert a["table"] == [RAN] and a["pack"][0]["unpacked"] > 0
    _same(a, b)


# ---- gradient clipping on the lean path
def test_grad_clip(ctx, monkeypatch):
    """One learn() with the policy clipped at half of epoch 0's norm: the lean
    kernels run, the reported (unscaled) epoch-0 gradient holds the budgets, the
    log shows the clip, and every epoch is finite."""
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    N, T = 48, 4
    ref, mag = _oracle("ppo", N, T)
    base = _run(ctx, monkeypatch, "ppo", N, T, 0)
    norm0 = float(np.sqrt(np.sum(base["grads"][0].astype(np.float64) ** 2)))
    for k in ("XH_TRAIN_TABLE", "XH_SP8_PACK", "XH_TRAIN_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("XH_E0_REUSE", "0")
    pp, vp = _params()
    tr = Trainer(ctx, algo="ppo", bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    tr.set_grad_clip(POLICY, 0.5 * norm0)
    tr.rollout()
    tr.learn()
    npi = tr.num_params(POLICY)
    g = tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy()
    log, tab, params = tr.grad_clip_log(POLICY), tr.table_stats(), tr.params(POLICY).copy()
    tr.close()
    assert tab == RAN, tab
    assert np.isfinite(g).all() and np.isfinite(params).all()
    # the same inputs, the same kernels: epoch 0 is the unclipped run's
    np.testing.assert_array_equal(g[0], base["grads"][0])
    assert_grad_units(g[0], ref.reshape(-1, npi)[0], mag.reshape(-1, npi)[0],
                      what="table_mm clip epoch0")
    assert log.shape == (g.shape[0], 2)
    assert abs(log[0, 0] - norm0) <= 1e-5 * norm0, (log[0], norm0)
    assert abs(log[0, 1] - 0.5) <= 1e-5, log[0]
    assert (log[:, 1] > 0).all() and (log[:, 1] <= 1.0).all()
