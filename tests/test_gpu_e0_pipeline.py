"""The one-phase pipeline of PPO's epoch-0 kernel
(policy_train_spec8_e0_kernel, dependence_free_rl_amd/csrc/
policy_spec8_kernels.hip built with XH_SP8_E0_TU=1): one
barrier per 64-row group, the relu masks in a ring of four slots, g (x) H1 and
the staged g in two, the loop unrolled over four groups with a peeled first
phase and dW2 of the last group after the loop.

Shape and budgets as tests/test_gpu_e0_reuse.py (64 bins, 2-D, [128,128], PPO,
XH_E0_REUSE=2, the oracle's epoch-0 gradient in conftest's units, and p99 of
the path against the path switched off).  Cases, the smallest at which the
deeper rings can go wrong and which that file does not have:

- one workgroup running J = 4, 5, 6, 7 groups (N = 1, T = 4..7): every
  residue of the unroll period of four plus one, fewer groups than ring
  slots in the fill and drain, the clamped look-ahead of the last groups;
- N = 7, T = 3 at train_grid_cap = 4: 21 groups on 4 workgroups, J = 6, 5, 5,
  5, a grid that is no multiple of 8;
- determinism of the J = 7 case and of N = 48, T = 4 at the default grid.

All-zero advantages are not a case here: the only way to them is a host write
of the done flags (tests/test_gpu_spec8_dw2pair.py), and a host write into the
batch rightly switches the epoch-0 path off.
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units, grad_units

pytestmark = pytest.mark.gpu

B, D, WIDTHS = 64, 2, (128, 128)
X0 = 4711
PLAIN = "policy_train_spec8_kernel"

_oracles = {}
_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    return init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)


def _oracle(N, T):
    """One oracle iteration per (N, T), shared by the cases (read only)."""
    if (N, T) not in _oracles:
        from oracle import pyoracle as po
        pp, vp = _params()
        orc = po.Trainer(po.OR_PPO, B, D, N, T,
                         po.perbin_model(2 * D, list(WIDTHS), po.OR_SOFTMAX), pp,
                         po.full_model(B * 2 * D, [64, 32], 1), vp,
                         lr_pi=1e-4, lr_v=1e-5, x0=X0)
        orc.rollout()
        orc.learn()
        ref = np.asarray(orc.buf(po.BUF_POLICY_GRADS)).copy()
        mag = np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).copy()
        _oracles[(N, T)] = (ref, mag)
    return _oracles[(N, T)]


def _run(ctx, monkeypatch, N, T, cap, mode, cache=True):
    """rollout(), learn() under XH_E0_REUSE=mode."""
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    key = (N, T, cap, mode)
    if cache and key in _runs:
        return _runs[key]
    monkeypatch.setenv("XH_E0_REUSE", str(mode))
    pp, vp = _params()
    tr = Trainer(ctx, algo="ppo", bins=B, dims=D, num_envs=N, steps=T,
                 widths=WIDTHS, rng_state=X0, train_grid_cap=cap)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    tr.rollout()
    tr.learn()
    npi = tr.num_params(POLICY)
    out = {"info": tr.kernel_info(),
           "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
           "params": tr.params(POLICY).copy()}
    tr.close()
    if cache:
        _runs[key] = out
    return out


# (N, T, train_grid_cap, the largest J of a workgroup)
CASES = [(1, 4, 1, 4), (1, 5, 1, 5), (1, 6, 1, 6), (1, 7, 1, 7), (7, 3, 4, 6)]


@pytest.mark.parametrize("N,T,cap,jmax", CASES)
def test_pipeline_vs_oracle_and_switched_off(ctx, monkeypatch, N, T, cap, jmax):
    ref, mag = _oracle(N, T)
    on = _run(ctx, monkeypatch, N, T, cap, 2)  # the learn() succeeded on the path
    off = _run(ctx, monkeypatch, N, T, cap, 0)
    assert on["info"]["policy_train"]["kernel"] == PLAIN, on["info"]
    grid = on["info"]["train_grid"]
    assert grid == min(cap, N * T), (cap, grid)
    assert -(-(N * T) // grid) == jmax
    g, g_off = on["grads"], off["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape and g.shape[0] >= 2
    assert np.isfinite(g).all() and np.isfinite(on["params"]).all()
    u_on, _, _ = grad_units(g[0], r[0], m[0])
    u_off, _, _ = grad_units(g_off[0], r[0], m[0])
    p_on, p_off = float(np.percentile(u_on, 99)), float(np.percentile(u_off, 99))
    rel = float(np.linalg.norm(g[0] - g_off[0]) / np.linalg.norm(g_off[0]))
    print("e0 pipeline N=%d T=%d grid=%d J=%d: epoch-0 p99 units %.3g (off %.3g), median "
          "%.3g (off %.3g), rel L2 on vs off %.3g" % (
              N, T, grid, jmax, p_on, p_off, float(np.median(u_on)),
              float(np.median(u_off)), rel))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="e0 pipeline N%d T%d grid=%d J=%d epoch%d" % (
                              N, T, grid, jmax, ep),
                          **budget)
    # no accuracy regression against the path switched off on the same inputs
    assert p_on <= 2.0 * p_off + 2.0, (p_on, p_off)


@pytest.mark.parametrize("N,T,cap", [(1, 7, 1), (48, 4, 0)])
def test_pipeline_deterministic(ctx, monkeypatch, N, T, cap):
    a = _run(ctx, monkeypatch, N, T, cap, 2)
    b = _run(ctx, monkeypatch, N, T, cap, 2, cache=False)
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])
