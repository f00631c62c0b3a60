"""The config-3 PPO / actor-critic epochs ON THE TABLE
(dependence_free_rl_amd/csrc/spec8_table_kernels.hip, spec8_table_layout.h and
policy_spec8_kernels.hip built with XH_SP8_TAB_TU=1; DESIGN.md §3.0e, "the
epoch on the table"): a forward over the 578 (bin state, item) points, one
streaming pass over the packed batch that sums the loss gradient per point, a
backward over the 578 points weighted by the sums.

Shape: 64 bins, 2-D, [128,128], the seeds and parameters of
test_gpu_spec8_pack.py.  Every epoch's gradient is held to conftest's budgets
against the oracle, epoch 0 to the rule between kernels against the same
inputs with XH_TRAIN_TABLE=0 (the packed launches); the mixed batch (env-steps
of more than 16 distinct states: wide groups in the streaming pass) against
XH_TRAIN_KERNEL=f32 with the unpacked path's own distance as the limit; two
runs are equal bit for bit; and where the gate keeps the table away
(XH_TRAIN_TABLE=0, KL-PPO, a trainer that has held a bin below -8) the result
is the packed path's, bit for bit.
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units, grad_units

pytestmark = pytest.mark.gpu

B, D, H, WIDTHS = 64, 2, 128, (128, 128)
F0 = 2 * D
X0 = 4711
KERNEL = "policy_train_spec8_kernel"
RAN = {"ran": True, "out_of_domain": 0, "groups": 10}
NOT_RAN = {"ran": False, "out_of_domain": 0, "groups": 0}

_oracles = {}
_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    return init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)


def _oracle(algo, N, T):
    """One oracle iteration per (algo, N, T), shared by the cases (read only)."""
    key = (algo, N, T)
    if key not in _oracles:
        from oracle import pyoracle as po
        pp, vp = _params()
        head = po.OR_SOFTMAX_XENT if algo == "ac" else po.OR_SOFTMAX
        kw = dict(lr_pi=1e-5 if algo == "ac" else 1e-4, lr_v=1e-4 if algo == "ac" else 1e-5)
        orc = po.Trainer({"ppo": po.OR_PPO, "ac": po.OR_AC}[algo],
                         B, D, N, T, po.perbin_model(F0, list(WIDTHS), head), pp,
                         po.full_model(B * F0, [64, 32], 1), vp, x0=X0, **kw)
        orc.rollout()
        orc.learn()
        _oracles[key] = (np.asarray(orc.buf(po.BUF_POLICY_GRADS)).copy(),
                         np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).copy())
    return _oracles[key]


def _env(monkeypatch, table=None, pack=None, e0=0, kernel=None):
    for k, v in (("XH_TRAIN_TABLE", table), ("XH_SP8_PACK", pack), ("XH_E0_REUSE", e0),
                 ("XH_TRAIN_KERNEL", kernel)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(ctx, monkeypatch, algo, N, T, cap, table=None, pack=None, e0=0, kernel=None,
         states=None, iters=1, cache=True):
    """`iters` rollout + learn rounds; the outputs are the last learn()'s, the
    table and pack statistics every learn()'s."""
    key = (algo, N, T, cap, table, pack, e0, kernel, states is not None and id(states), iters)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    _env(monkeypatch, table, pack, e0, kernel)
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0, train_grid_cap=cap)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if states:
        _, items = tr.env_state()
        for e, st in states.items():
            tr.set_env_state(e, st[None], items[e:e + 1])
    tab, pk = [], []
    for _ in range(iters):
        tr.rollout()
        tr.learn()
        tab.append(tr.table_stats())
        pk.append(tr.pack_stats())
    npi = tr.num_params(POLICY)
    out = {"info": tr.kernel_info(), "table": tab, "pack": pk,
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
           "params": tr.params(POLICY).copy()}
    tr.close()
    if cache:
        _runs[key] = out
    return out


def _same(a, b):
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])


def _check(ctx, monkeypatch, algo, N, T, cap):
    ref, mag = _oracle(algo, N, T)
    new = _run(ctx, monkeypatch, algo, N, T, cap)
    old = _run(ctx, monkeypatch, algo, N, T, cap, table=0)
    assert new["table"] == [RAN], new["table"]
    assert old["table"] == [NOT_RAN], old["table"]
    # both ran over the same packed batch and report the same kernel and grid
    assert new["pack"] == old["pack"] and new["pack"][0]["packed"] == N * T
    assert new["info"] == old["info"], (new["info"], old["info"])
    assert new["info"]["policy_train"]["kernel"] == KERNEL
    grid = new["info"]["train_grid"]
    if cap:
        assert grid == min(cap, N * T)
    g, g_o = new["grads"], old["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape and g.shape[0] >= (2 if algo == "ppo" else 1)
    assert np.isfinite(g).all() and np.isfinite(new["params"]).all()
    u_new, _, _ = grad_units(g[0], r[0], m[0])
    u_old, _, _ = grad_units(g_o[0], r[0], m[0])
    p_new, p_old = float(np.percentile(u_new, 99)), float(np.percentile(u_old, 99))
    print("table %s N=%d T=%d grid=%d: epoch-0 p99 units %.3g (packed %.3g), median %.3g "
          "(packed %.3g)" % (algo, N, T, grid, p_new, p_old, float(np.median(u_new)),
                             float(np.median(u_old))))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="table %s N%d T%d grid=%d epoch%d" % (algo, N, T, grid, ep),
                          **budget)
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


CASES = [(1, 1, 1), (7, 3, 0), (48, 4, 0), (48, 4, 1), (48, 4, 5), (48, 4, 64)]


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ppo", N, T, cap)


@pytest.mark.parametrize("cap", [0, 1, 5, 64])
def test_actor_critic(ctx, monkeypatch, cap):
    _check(ctx, monkeypatch, "ac", 48, 4, cap)


def test_ppo_epoch0_on_e0_kernel(ctx, monkeypatch):
    """XH_E0_REUSE=2: epoch 0 stays on the e0 kernel (bit for bit the packed
    learn()'s), the later epochs run on the table."""
    new = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=2)
    old = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=2, table=0)
    assert new["table"] == [RAN] and old["table"] == [NOT_RAN]
    np.testing.assert_array_equal(new["grads"][0], old["grads"][0])
    ref, mag = _oracle("ppo", 48, 4)
    npi = new["grads"].shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    for ep in range(1, new["grads"].shape[0]):
        assert_grad_units(new["grads"][ep], r[ep], m[ep], what="table e0=2 epoch%d" % ep,
                          p99_units=GRAD_UNITS_P99_DRIFT)


# ---- the mixed batch of test_gpu_spec8_pack.py's test_fallback_mixed_batch:
# env-steps of more than 16 distinct bin states are wide groups of the
# streaming pass (one env-step over 64 rows, states may repeat)
FN, FT = 24, 2
LEGAL = [(a, b) for a in range(-8, 9) for b in range(-8, 9)]


def _states():
    """Envs 0-5: 64 distinct legal bin states, 6-11: exactly 16, 12-17:
    exactly 17 (negative values among all of them); 18-23 stay fresh."""
    rng = np.random.RandomState(2024)
    out = {}
    for e in range(18):
        d = (64, 16, 17)[e // 6]
        pick = rng.permutation(len(LEGAL))[:d]
        st = np.array([LEGAL[i] for i in pick], np.int8)
        if not (st < 0).any():
            st[0] = (-3, 5)
            assert len({tuple(x) for x in st}) == d
        rows = np.concatenate([np.arange(d), rng.randint(0, d, B - d)])
        out[e] = st[rng.permutation(rows)]
    return out


MIXED = _states()


def _rel_l2(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_mixed_batch(ctx, monkeypatch, algo):
    new = _run(ctx, monkeypatch, algo, FN, FT, 0, states=MIXED)
    old = _run(ctx, monkeypatch, algo, FN, FT, 0, states=MIXED, pack=0)
    f32 = _run(ctx, monkeypatch, algo, FN, FT, 0, states=MIXED, kernel="f32")
    assert new["table"] == [RAN], new["table"]
    assert old["table"] == [NOT_RAN] and f32["table"] == [NOT_RAN]
    st = new["pack"][0]
    assert st["unpacked"] >= 12 and st["packed"] >= 12, st  # wide groups present
    assert np.isfinite(new["grads"]).all()
    for ep in range(new["grads"].shape[0]):
        e_new = _rel_l2(new["grads"][ep], f32["grads"][ep])
        e_old = _rel_l2(old["grads"][ep], f32["grads"][ep])
        print("table mixed %s epoch %d: rel L2 table-f32 %.3g, unpacked-f32 %.3g (%d packed, "
              "%d wide env-steps)" % (algo, ep, e_new, e_old, st["packed"], st["unpacked"]))
        assert e_new <= 2.0 * e_old, (ep, e_new, e_old)


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


# ---- the gate
def test_gate_switch_off(ctx, monkeypatch):
    """XH_TRAIN_TABLE=0: the packed launches, whatever else is set."""
    off = _run(ctx, monkeypatch, "ppo", 48, 4, 0, table=0)
    again = _run(ctx, monkeypatch, "ppo", 48, 4, 0, table=0, cache=False)
    assert off["table"] == [NOT_RAN] and off["pack"][0]["packed"] == 48 * 4
    _same(off, again)


def test_gate_klppo(ctx, monkeypatch):
    on = _run(ctx, monkeypatch, "klppo", 48, 4, 0)
    off = _run(ctx, monkeypatch, "klppo", 48, 4, 0, table=0)
    assert on["table"] == [NOT_RAN] and off["table"] == [NOT_RAN]
    _same(on, off)


def test_gate_bin_below_table(ctx, monkeypatch):
    """A trainer whose slot 0 held a bin below -8: no table entry, in that
    window (no packed learn() at all) or in any later one (the bin stays until
    an action takes it; the packed launches run)."""
    st = np.full((B, D), 8, np.int8)
    st[17] = (-40, -9)
    states = {3: st}
    on = _run(ctx, monkeypatch, "ppo", 12, 2, 0, states=states, iters=2)
    off = _run(ctx, monkeypatch, "ppo", 12, 2, 0, states=states, iters=2, table=0)
    assert on["table"] == [NOT_RAN] * 2 and off["table"] == [NOT_RAN] * 2
    assert on["pack"] == off["pack"]
    assert on["pack"][0]["packed"] == 0        # a wide slot: unpacked
    _same(on, off)
