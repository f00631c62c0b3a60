"""PPO's epoch 0 on the rollout's forward outputs
(policy_train_spec8_e0_kernel, dependence_free_rl_amd/csrc/
policy_spec8_kernels.hip built with XH_SP8_E0_TU=1): the
rollout's relu-mask records and distributions in place of the epoch's own
layer 2, partial logits and softmax.

XH_E0_REUSE (read per learn()): 2 fails the learn() when epoch 0 cannot run on
the rollout's outputs, 0 switches the path off, unset uses it when valid.

Shapes: 64 bins, 2-D, [128,128], PPO.  N = 48, T = 4 (192 groups) at the train
grids of test_gpu_spec8.py (one group per workgroup, J = 3, a grid that is no
multiple of 8 with unequal J, one workgroup running all 192), and 1, 2 and 3
groups in one workgroup (J = 1, 2, 3: the pipeline's fill, an odd J, the
prefetch of the last group, whose look-ahead loads are clamped).
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


def _trainer(ctx, N, T, cap=0, algo="ppo", epochs=None):
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=WIDTHS, rng_state=X0, train_grid_cap=cap, epochs=epochs)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    return tr


def _setenv(monkeypatch, mode):
    if mode is None:
        monkeypatch.delenv("XH_E0_REUSE", raising=False)
    else:
        monkeypatch.setenv("XH_E0_REUSE", str(mode))


def _learned(tr):
    from dependence_free_rl_amd import POLICY
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    npi = tr.num_params(POLICY)
    return {"info": tr.kernel_info(),
            "grads": tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy(),
            "params": tr.params(POLICY).copy()}


def _run(ctx, monkeypatch, N, T, cap, mode, between=None, cache=True):
    """rollout(), `between`(tr), learn() under XH_E0_REUSE=mode."""
    key = (N, T, cap, mode)
    if cache and between is None and key in _runs:
        return _runs[key]
    _setenv(monkeypatch, mode)
    tr = _trainer(ctx, N, T, cap)
    tr.rollout()
    if between:
        between(tr)
    tr.learn()
    out = _learned(tr)
    tr.close()
    if cache and between is None:
        _runs[key] = out
    return out


CASES = [(48, 4, 0), (48, 4, 64), (48, 4, 5), (48, 4, 1),
         (1, 1, 1), (1, 2, 1), (1, 3, 1)]


@pytest.mark.parametrize("N,T,cap", CASES)
def test_e0_vs_oracle_and_switched_off(ctx, monkeypatch, N, T, cap):
    ref, mag = _oracle(N, T)
    on = _run(ctx, monkeypatch, N, T, cap, 2)  # the learn() succeeded on the path
    off = _run(ctx, monkeypatch, N, T, cap, 0)
    # the later epochs' launches report the kernel
    assert on["info"]["policy_train"]["kernel"] == PLAIN, on["info"]
    grid = on["info"]["train_grid"]
    assert cap == 0 or grid == min(cap, N * T), (cap, grid)
    J = -(-(N * T) // grid)
    g, g_off = on["grads"], off["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape and g.shape[0] >= 2
    assert np.isfinite(g).all() and np.isfinite(on["params"]).all()
    # the figures first (epoch 0 of both runs against the oracle, and the two
    # against each other: a wrong bit layout lands orders of magnitude outside)
    u_on, _, _ = grad_units(g[0], r[0], m[0])
    u_off, _, _ = grad_units(g_off[0], r[0], m[0])
    p_on, p_off = float(np.percentile(u_on, 99)), float(np.percentile(u_off, 99))
    rel = float(np.linalg.norm(g[0] - g_off[0]) / np.linalg.norm(g_off[0]))
    print("e0 reuse N=%d T=%d grid=%d J=%d: epoch-0 p99 units %.3g (off %.3g), median "
          "%.3g (off %.3g), rel L2 on vs off %.3g" % (
              N, T, grid, J, p_on, p_off, float(np.median(u_on)),
              float(np.median(u_off)), rel))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="e0 reuse N%d T%d grid=%d J=%d epoch%d" % (N, T, grid, J, ep),
                          **budget)
    # no accuracy regression against the path switched off on the same inputs
    # (test_gpu_spec8.py's rule between kernels)
    assert p_on <= 2.0 * p_off + 2.0, (p_on, p_off)


def test_e0_deterministic(ctx, monkeypatch):
    a = _run(ctx, monkeypatch, 48, 4, 0, 2)
    b = _run(ctx, monkeypatch, 48, 4, 0, 2, cache=False)
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])


def _set_policy(tr):
    from dependence_free_rl_amd import POLICY
    tr.set_params(POLICY, _params()[0])


def _set_bins(tr):
    from dependence_free_rl_amd.trainer import BUF_BINS
    tr.set_buffer(BUF_BINS, tr.buffer(BUF_BINS))  # legal states: its own


@pytest.mark.parametrize("between", [_set_policy, _set_bins],
                         ids=["set_params", "set_buffer_bins"])
def test_a_write_invalidates(ctx, monkeypatch, between):
    """A write of the policy parameters, or a host write into the batch,
    between rollout() and learn(): XH_E0_REUSE=2 raises; with the variable
    unset the learn() runs the plain kernel -- the same bits as XH_E0_REUSE=0."""
    from dependence_free_rl_amd._lib import XhError
    N, T = 48, 4
    _setenv(monkeypatch, 2)
    tr = _trainer(ctx, N, T)
    tr.rollout()
    between(tr)
    with pytest.raises(XhError, match="XH_E0_REUSE"):
        tr.learn()
    tr.close()
    unset = _run(ctx, monkeypatch, N, T, 0, None, between=between)
    off = _run(ctx, monkeypatch, N, T, 0, 0, between=between)
    np.testing.assert_array_equal(unset["grads"], off["grads"])
    np.testing.assert_array_equal(unset["params"], off["params"])


def test_second_learn_invalid(ctx, monkeypatch):
    from dependence_free_rl_amd._lib import XhError
    _setenv(monkeypatch, 2)
    tr = _trainer(ctx, 48, 4)
    tr.rollout()
    tr.learn()
    with pytest.raises(XhError, match="XH_E0_REUSE"):
        tr.learn()  # the first learn() stepped the policy
    tr.close()


def test_wide_slot0_invalid(ctx, monkeypatch):
    """Slot 0 below -capacity runs on the f32 rollout (test_gpu_boundary.py):
    no mask records for it."""
    from dependence_free_rl_amd._lib import XhError
    _setenv(monkeypatch, 2)
    tr = _trainer(ctx, 48, 4)
    bins, items = tr.env_state()
    bins[5, 3, 0] = -40
    tr.set_env_state(0, bins, items)
    tr.rollout()
    with pytest.raises(XhError, match="XH_E0_REUSE"):
        tr.learn()
    tr.close()


@pytest.mark.parametrize("algo,epochs", [("ppo", 1), ("ac", None)])
def test_out_of_scope(ctx, monkeypatch, algo, epochs):
    """One-epoch PPO and actor-critic keep the plain kernel (kernel_info names
    the last epoch's launch), and have nothing to reuse."""
    from dependence_free_rl_amd._lib import XhError
    _setenv(monkeypatch, None)
    tr = _trainer(ctx, 48, 4, algo=algo, epochs=epochs)
    tr.rollout()
    tr.learn()
    assert tr.kernel_info()["policy_train"]["kernel"] == PLAIN
    tr.rollout()
    _setenv(monkeypatch, 2)
    with pytest.raises(XhError, match="XH_E0_REUSE"):
        tr.learn()
    tr.close()
