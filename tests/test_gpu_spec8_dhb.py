"""The config-3 train kernels' vector-wave schedule with dH1 moved into
phase B (XH_SP8_DHB, dependence_free_rl_amd/csrc/policy_spec8_kernels.hip,
DESIGN.md §3.0e): phase A runs g (x) H1 alone (and, at 8, dH1's r-tile 0),
phase B one stream of dH1, layer1(j + 2) and dW1(j) cut into pieces that sit in
dH1's MFMA slots.  The product library alone, whatever setting it was built
with, against the oracle on conftest's budgets: epoch 0 on the tight one,
later epochs on the drift one, parameters within 1e-4 (adam's noise-level
entries by conftest's rule).  XH_E0_REUSE=0, so every PPO epoch runs the plain
kernel.

Shapes (64 bins, 2-D, [128,128]; J = a workgroup's groups), the smallest at
which the schedule can go wrong:
  N, T, train_grid_cap
  1, 1, 1   J = 1: the prologue's layer1(0) / layer1(1) straight into the
            epilogue; in B(0) dH1(0) runs beside a layer1(2) of a clamped group
  1, 2, 1   J = 2, 3: both parities of the loop unrolled over two periods, an
  1, 3, 1   odd J skipping the second
  7, 3, 4   J = 6, 5, 5, 5: uneven workgroups, both mask slots reused
  48, 4, 0  192 groups on the default grid, one per workgroup

Seeds: PPO and actor-critic run on test_gpu_spec8_l1pack.py's rng state,
KL-PPO on test_gpu_klppo.py's.  KL-PPO's epoch-0 p99 at the 4- and 28-row
batches of (1, 3, 1) and (7, 3, 4) depends on the seed far more than PPO's
does (its end rows carry A = 0, so their g is beta times the rounding
difference between p and the recorded q, against a magnitude of few terms):
over eight seeds the kernel as it was before this schedule (bit-identical
gradients) gave 1.15 to 142 units at (1, 3, 1) and 3.7 to 129 at (7, 3, 4),
above the tight budget of 100 for 3 and 1 of the eight, where PPO stayed below
13 on all of them (profiles/dhb_kl_seed_sweep.txt).  At
test_gpu_klppo.py's seed the two cases measure 11.3 and 79.4.
"""
import numpy as np
import pytest

from conftest import (GRAD_UNITS_P99_DRIFT, assert_grad_units, assert_params_close,
                      grad_units, noise_mask)
from gpu_helpers import step_major

pytestmark = pytest.mark.gpu

B, D, H, WIDTHS = 64, 2, 128, (128, 128)
F0 = 2 * D
X0 = {"ppo": 4711, "ac": 4711, "klppo": 777001}
KERNEL = {"ppo": "policy_train_spec8_kernel", "ac": "policy_train_spec8_kernel",
          "klppo": "policy_train_spec8_kl_kernel"}
LR_PI = {"ppo": 1e-4, "ac": 1e-5}
KL_WD = 1e-5

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
        kw = dict(wd_pi=KL_WD) if algo == "klppo" else dict(
            lr_pi=LR_PI[algo], lr_v=1e-4 if algo == "ac" else 1e-5)
        orc = po.Trainer({"ppo": po.OR_PPO, "ac": po.OR_AC, "klppo": po.OR_KLPPO}[algo],
                         B, D, N, T, po.perbin_model(F0, list(WIDTHS), head), pp,
                         po.full_model(B * F0, [64, 32], 1), vp, x0=X0[algo], **kw)
        orc.rollout()
        actions = step_major(orc.buf(po.BUF_STEP_CHOICE), N, T).copy()
        orc.learn()
        _oracles[key] = {
            "grads": np.asarray(orc.buf(po.BUF_POLICY_GRADS)).copy(),
            "mag": np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).copy(),
            "actions": actions, "params": np.asarray(orc.params(0)).copy(),
            "kl": (np.asarray(orc.buf(po.BUF_KL)).reshape(-1, 3).copy()
                   if algo == "klppo" else None)}
    return _oracles[key]


def _run(ctx, monkeypatch, algo, N, T, cap, kernel=None, cache=True):
    """rollout() on the oracle's actions, learn(), every epoch on the plain
    kernel (XH_E0_REUSE=0); XH_TRAIN_KERNEL = kernel."""
    key = (algo, N, T, cap, kernel)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_ACTION, BUF_KL, BUF_POLICY_GRADS
    monkeypatch.setenv("XH_E0_REUSE", "0")
    if kernel is None:
        monkeypatch.delenv("XH_TRAIN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("XH_TRAIN_KERNEL", kernel)
    pp, vp = _params()
    kw = dict(wd_policy=KL_WD) if algo == "klppo" else {}
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0[algo], train_grid_cap=cap, **kw)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if algo == "klppo":  # (test_gpu_klppo.py: the device replays the oracle's actions)
        tr.set_forced_actions(_oracle(algo, N, T)["actions"])
    tr.rollout()
    actions = tr.buffer(BUF_ACTION).copy()
    tr.learn()
    npi = tr.num_params(POLICY)
    out = {"info": tr.kernel_info(), "actions": actions,
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
           "params": tr.params(POLICY).copy(),
           "kl": tr.buffer(BUF_KL).copy() if algo == "klppo" else None}
    tr.close()
    if cache:
        _runs[key] = out
    return out


def _check(ctx, monkeypatch, algo, N, T, cap, epochs=None):
    orc = _oracle(algo, N, T)
    new = _run(ctx, monkeypatch, algo, N, T, cap)
    assert new["info"]["policy_train"]["kernel"] == KERNEL[algo], new["info"]
    grid = new["info"]["train_grid"]
    # the device sampled (or replayed) the oracle's actions: the same batch
    np.testing.assert_array_equal(new["actions"].reshape(T, N), orc["actions"].reshape(T, N))
    g = new["grads"]
    npi = g.shape[1]
    r, m = orc["grads"].reshape(-1, npi), orc["mag"].reshape(-1, npi)
    assert g.shape == r.shape
    if epochs is not None:
        assert g.shape[0] == epochs
    assert np.isfinite(g).all() and np.isfinite(new["params"]).all()
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        med, p99, mx = assert_grad_units(
            g[ep], r[ep], m[ep],
            what="dhb %s N%d T%d grid=%d epoch%d" % (algo, N, T, grid, ep), **budget)
        print("dhb %s N=%d T=%d cap=%d grid=%d epoch %d: median %.3g p99 %.3g max %.3g units"
              % (algo, N, T, cap, grid, ep, med, p99, mx))
    if algo == "klppo":
        np.testing.assert_array_equal(new["kl"][:, 0], orc["kl"][:, 0])  # beta used
        np.testing.assert_array_equal(new["kl"][:, 2], orc["kl"][:, 2])  # beta after
        assert_params_close(new["params"], orc["params"], what="dhb klppo policy")
    else:
        assert_params_close(new["params"], orc["params"], noise_mask(r),
                            2 * LR_PI[algo] * g.shape[0],
                            what="dhb %s N%d T%d cap%d policy" % (algo, N, T, cap))
    return new, r, m


CASES = [(1, 1, 1), (1, 2, 1), (1, 3, 1), (7, 3, 4), (48, 4, 0)]


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo_four_epochs(ctx, monkeypatch, N, T, cap):
    new, r, m = _check(ctx, monkeypatch, "ppo", N, T, cap, epochs=4)
    grid = new["info"]["train_grid"]
    assert grid == {(1, 1, 1): 1, (1, 2, 1): 1, (1, 3, 1): 1, (7, 3, 4): 4,
                    (48, 4, 0): 192}[(N, T, cap)], grid
    if (N, T, cap) == (48, 4, 0):
        # test_gpu_spec8.py's rule between kernels, on the same inputs:
        # epoch 0 against XH_TRAIN_KERNEL=split8wh, whose schedule did not change
        old = _run(ctx, monkeypatch, "ppo", N, T, cap, kernel="split8wh")
        assert old["info"]["policy_train"]["kernel"] == "policy_train_split8wh_kernel"
        u_new, _, _ = grad_units(new["grads"][0], r[0], m[0])
        u_old, _, _ = grad_units(old["grads"][0], r[0], m[0])
        p_new, p_old = float(np.percentile(u_new, 99)), float(np.percentile(u_old, 99))
        print("dhb ppo N=48 T=4: epoch-0 p99 units %.3g (split8wh %.3g)" % (p_new, p_old))
        assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


@pytest.mark.parametrize("N,T,cap", [(7, 3, 4), (1, 3, 1)])
def test_actor_critic(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ac", N, T, cap)


@pytest.mark.parametrize("N,T,cap", [(7, 3, 4), (1, 3, 1)])
def test_klppo(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "klppo", N, T, cap)


def test_deterministic(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, "ppo", 7, 3, 4)
    b = _run(ctx, monkeypatch, "ppo", 7, 3, 4, cache=False)
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])
