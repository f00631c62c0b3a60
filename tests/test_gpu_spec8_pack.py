"""The config-3 PPO / actor-critic epochs over the packed batch
(dependence_free_rl_amd/csrc/spec8_pack_kernels.hip, spec8_pack_layout.h and
policy_spec8_kernels.hip built with XH_SP8_PACK_TU=1; DESIGN.md §3.0e,
"duplicate rows"): an env-step's distinct bin states with their counts fill a
16-row segment, four env-steps of one item a 64-row group, and the softmax and
its backward run on the count-weighted sums.

Shape: 64 bins, 2-D, [128,128], the seeds and parameters of
test_gpu_spec8_l1pack.py.  Oracle parity: N = 1, T = 1 (one segment, three
empty), N = 1, T = 3, N = 7, T = 3 (both items, partly filled last groups),
N = 48, T = 4 at train_grid_cap 0, 1, 5 and 64 (49 packed groups: at 64 and
at 192 workgroups some have none and write zero slabs).  Every epoch's
gradient is held to conftest's budgets against the oracle and epoch 0 to
test_gpu_spec8.py's rule between kernels against the same inputs with
XH_SP8_PACK=0.  PPO runs with XH_E0_REUSE=0 and with the default (a packed
learn() runs epoch 0 packed too; its XH_SP8_PACK=0 partner runs the e0 kernel).

Fallback: the oracle has no state setter, so the env-steps with more than 16
distinct bin states (one 64-row group each, in the same launches) are checked
against XH_TRAIN_KERNEL=f32 on a batch whose limit is measured on the batch
itself: the unpacked path's own distance from the f32 kernels.
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units, grad_units

pytestmark = pytest.mark.gpu

B, D, H, WIDTHS = 64, 2, 128, (128, 128)
F0 = 2 * D
X0 = 4711
KERNEL = "policy_train_spec8_kernel"

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


def _distinct(bins):
    """Distinct bin states per env-step of bins [..., B, D]."""
    flat = bins.reshape(-1, B, D).astype(np.int32)
    keys = flat[:, :, 0] * 64 + flat[:, :, 1]
    return np.array([len(np.unique(k)) for k in keys])


def _env(monkeypatch, pack, e0, kernel=None):
    for k, v in (("XH_SP8_PACK", pack), ("XH_E0_REUSE", e0), ("XH_TRAIN_KERNEL", kernel)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _run(ctx, monkeypatch, algo, N, T, cap, e0=0, pack=None, cache=True):
    key = (algo, N, T, cap, e0, pack)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_BINS, BUF_POLICY_GRADS
    _env(monkeypatch, pack, e0)
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0, train_grid_cap=cap)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    tr.rollout()
    tr.learn()
    npi = tr.num_params(POLICY)
    out = {"info": tr.kernel_info(), "stats": tr.pack_stats(),
           "distinct": _distinct(tr.buffer(BUF_BINS)[:T]),
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
           "params": tr.params(POLICY).copy()}
    tr.close()
    if cache:
        _runs[key] = out
    return out


def _check(ctx, monkeypatch, algo, N, T, cap, e0):
    ref, mag = _oracle(algo, N, T)
    new = _run(ctx, monkeypatch, algo, N, T, cap, e0=e0)
    old = _run(ctx, monkeypatch, algo, N, T, cap, e0=e0, pack=0)
    # the same kernel and arithmetic reported, the switch off runs nothing packed
    assert new["info"]["policy_train"] == old["info"]["policy_train"], (new["info"], old["info"])
    assert new["info"]["policy_train"]["kernel"] == KERNEL
    assert old["stats"] == {"packed": 0, "unpacked": 0, "groups": 0}
    # every env-step ran packed (the environment reaches ten bin states)
    st = new["stats"]
    assert int(new["distinct"].max()) <= 10
    assert st["packed"] == N * T and st["unpacked"] == 0, st
    assert N * T / 4 <= st["groups"] <= N * T // 4 + 2, st
    grid = new["info"]["train_grid"]
    if cap:  # the grid stays derived from env-steps
        assert grid == min(cap, N * T)
    g, g_o = new["grads"], old["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape
    assert np.isfinite(g).all() and np.isfinite(new["params"]).all()
    u_new, _, _ = grad_units(g[0], r[0], m[0])
    u_old, _, _ = grad_units(g_o[0], r[0], m[0])
    p_new, p_old = float(np.percentile(u_new, 99)), float(np.percentile(u_old, 99))
    print("pack %s e0=%s N=%d T=%d grid=%d groups=%d: epoch-0 p99 units %.3g (unpacked %.3g), "
          "median %.3g (unpacked %.3g)" % (algo, e0, N, T, grid, st["groups"], p_new, p_old,
                                           float(np.median(u_new)), float(np.median(u_old))))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="pack %s e0=%s N%d T%d grid=%d epoch%d" % (
                              algo, e0, N, T, grid, ep), **budget)
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


CASES = [(1, 1, 1), (1, 3, 1), (7, 3, 0), (48, 4, 0), (48, 4, 1), (48, 4, 5), (48, 4, 64)]


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo_every_epoch_packed(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ppo", N, T, cap, e0=0)


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo_default(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ppo", N, T, cap, e0=None)


@pytest.mark.parametrize("N,T,cap", CASES)
def test_actor_critic(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ac", N, T, cap, e0=0)


# ---- the fallback: env-steps of more than 16 distinct bin states
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


def _fallback_run(ctx, monkeypatch, algo, pack=None, kernel=None):
    key = ("fb", algo, pack, kernel)
    if key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_BINS, BUF_POLICY_GRADS
    _env(monkeypatch, pack, 0, kernel)
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=FN, steps=FT, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    _, items = tr.env_state()
    for e, st in _states().items():
        tr.set_env_state(e, st[None], items[e:e + 1])
    tr.rollout()
    tr.learn()
    npi = tr.num_params(POLICY)
    out = {"info": tr.kernel_info(), "stats": tr.pack_stats(),
           "distinct": _distinct(tr.buffer(BUF_BINS)[:FT]).reshape(FT, FN),
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
           "params": tr.params(POLICY).copy()}
    tr.close()
    _runs[key] = out
    return out


def _rel_l2(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return float(np.linalg.norm(x - y) / np.linalg.norm(y))


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_fallback_mixed_batch(ctx, monkeypatch, algo):
    new = _fallback_run(ctx, monkeypatch, algo)
    old = _fallback_run(ctx, monkeypatch, algo, pack=0)
    f32 = _fallback_run(ctx, monkeypatch, algo, kernel="f32")
    d = new["distinct"]
    # slot 0 holds the states as set
    assert (d[0, :6] == 64).all() and (d[0, 6:12] == 16).all() and (d[0, 12:18] == 17).all()
    assert (d[0, 18:] == 1).all()
    np.testing.assert_array_equal(d, old["distinct"])
    np.testing.assert_array_equal(d, f32["distinct"])
    want_un = int((d > 16).sum())
    want = {"packed": FN * FT - want_un, "unpacked": want_un}
    st = new["stats"]
    assert {k: st[k] for k in want} == want, (st, want)
    assert want_un >= 12 and want["packed"] >= 12
    assert want["packed"] / 4 + want_un <= st["groups"] <= want["packed"] // 4 + 2 + want_un
    assert new["info"]["policy_train"] == old["info"]["policy_train"]
    assert new["info"]["policy_train"]["kernel"] == KERNEL
    assert np.isfinite(new["grads"]).all()
    for ep in range(new["grads"].shape[0]):
        e_new = _rel_l2(new["grads"][ep], f32["grads"][ep])
        e_old = _rel_l2(old["grads"][ep], f32["grads"][ep])
        e_no = _rel_l2(new["grads"][ep], old["grads"][ep])
        print("pack fallback %s epoch %d: rel L2 packed-f32 %.3g, unpacked-f32 %.3g, "
              "packed-unpacked %.3g (%d packed, %d unpacked env-steps, %d groups)" % (
                  algo, ep, e_new, e_old, e_no, st["packed"], st["unpacked"], st["groups"]))
        assert e_new <= 2.0 * e_old, (ep, e_new, e_old)


def test_deterministic_all_packed(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=None)
    b = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=None, cache=False)
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])


def test_deterministic_mixed(ctx, monkeypatch):
    a = _fallback_run(ctx, monkeypatch, "ppo")
    _runs.pop(("fb", "ppo", None, None))
    b = _fallback_run(ctx, monkeypatch, "ppo")
    assert a["stats"] == b["stats"] and a["stats"]["unpacked"] > 0
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])
