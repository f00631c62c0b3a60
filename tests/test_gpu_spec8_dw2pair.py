"""dW2 of policy_train_spec8_kernel on per-feature scaled f16 pairs
(dependence_free_rl_amd/csrc/policy_spec8_kernels.hip).

The operand g (x) H1 is scaled per H1 feature i by the power of two
2^14 / (G' B_i'): G' from the launch-wide bound G on the loss gradient g
(PPO max_t |A_t| max(1 + eps, 1 / p_old_t), actor-critic max_t |A_t|), B_i'
from the feature's own bound.  An f16 pair keeps 22 significant bits only
within 2^17 of that bound, so the cases put g far below G (a peaked policy
with a low-probability action sampled), the features far below each other
(test_gpu_range.py's h1_units) and both together, and hold the epoch-0 policy
gradient to conftest's tight budget against the oracle's double sums.
All-zero advantages (G = 0) must give exactly zero policy gradients.

Shape B=64, D=2, [128,128], N=32, T=4 (128 groups of 64 rows).
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units

pytestmark = pytest.mark.gpu

B, D, N, T, H = 64, 2, 32, 4, 128
F0 = 2 * D
OB1 = H * F0
OW2 = OB1 + H
OB2 = OW2 + H * H
OW3 = OB2 + H
X0 = 8642
CLIP_EPS = 0.2      # Trainer's default
W3_PEAK = 32.0      # w3 scaled: a peaked policy (p_old down to 7e-4 at X0)
SMALL = 2.0 ** -20  # test_gpu_range.py's h1_units


def _params(peaked, h1_small):
    """Reference flat layout (nn.h:499-508): W1 [H][2D], b1, W2 [H][H], b2,
    w3 [H], b3."""
    from dependence_free_rl_amd import init_policy
    p = init_policy(D, H, H, seed=61).copy()
    if peaked:
        p[OW3:OW3 + H] *= W3_PEAK
    if h1_small:  # half the layer-1 units (H1 features) tiny
        p[:OB1].reshape(H, F0)[: H // 2] *= SMALL
        p[OB1:OB1 + H // 2] *= SMALL
    return p.astype(np.float32)


def _oracle(algo, pp, vp):
    from oracle import pyoracle as po
    head = po.OR_SOFTMAX_XENT if algo == "ac" else po.OR_SOFTMAX
    return po.Trainer({"ppo": po.OR_PPO, "ac": po.OR_AC}[algo], B, D, N, T,
                      po.perbin_model(F0, [H, H], head), pp,
                      po.full_model(B * F0, [64, 32], 1), vp,
                      lr_pi=1e-5 if algo == "ac" else 1e-4,
                      lr_v=1e-4 if algo == "ac" else 1e-5, x0=X0)


def _g_range(orc, algo, pp):
    """From the oracle's buffers: the launch bound G over the median non-zero
    |g| of epoch 0 (ratio 1, nothing clipped: g = (p - onehot) A for both
    heads), and G over the median of the rows' largest |g|."""
    from oracle import pyoracle as po
    m = orc.buf(po.BUF_ROW_IS_END) == 0
    rows = orc.buf(po.BUF_ROWS).reshape(-1, B * F0)[m]
    A = orc.buf(po.BUF_ADVANTAGES).astype(np.float64)[m]
    pold = orc.buf(po.BUF_ROW_POLD).astype(np.float64)[m]
    ch = orc.buf(po.BUF_ROW_CHOICE)[m]
    assert len(A) == N * T
    p = po.model_eval(po.perbin_model(F0, [H, H], po.OR_SOFTMAX), pp,
                      rows).astype(np.float64)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(ch)), ch] = 1.0
    g = np.abs((p - onehot) * A[:, None])
    G = (np.max(np.abs(A) * np.maximum(1.0 + CLIP_EPS, 1.0 / pold))
         if algo == "ppo" else np.abs(A).max())
    assert g.max() <= G * (1 + 1e-6), (g.max(), G)  # the bound holds
    return G / np.median(g[g > 0]), G / np.median(g.max(axis=1))


def _device_and_oracle(ctx, algo, pp):
    from oracle import pyoracle as po
    from dependence_free_rl_amd import POLICY, VALUE, Trainer, init_value
    from dependence_free_rl_amd.trainer import BUF_ACTION, BUF_POLICY_GRADS
    vp = init_value(B, D, seed=62)
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=(H, H), rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    orc = _oracle(algo, pp, vp)
    tr.rollout()
    orc.rollout()
    np.testing.assert_array_equal(tr.buffer(BUF_ACTION),
                                  orc.buf(po.BUF_STEP_CHOICE).reshape(N, T).T)
    tr.learn()
    orc.learn()
    info = tr.kernel_info()
    assert info["policy_train"]["kernel"] == "policy_train_spec8_kernel", info
    npi = tr.num_params(POLICY)
    dev = tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy()
    tr.close()
    ref = np.asarray(orc.buf(po.BUF_POLICY_GRADS)).reshape(-1, npi)
    mag = np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).reshape(-1, npi)
    return dev, ref, mag, orc


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_default_parameters(ctx, algo):
    """Default parameters: epoch 0 on the tight budget; PPO's later epochs on
    the budget test_gpu_parity.py gives them (each side's own updates)."""
    pp = _params(False, False)
    dev, ref, mag, _ = _device_and_oracle(ctx, algo, pp)
    assert np.isfinite(dev).all()
    for ep in range(dev.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(dev[ep], ref[ep], mag[ep],
                          what="dw2pair default %s epoch%d" % (algo, ep), **budget)


@pytest.mark.parametrize("h1_small", [False, True], ids=["g_wide", "g_wide_h1_units"])
def test_wide_g_range(ctx, h1_small):
    """A peaked policy with a low-probability action sampled: the launch
    bound G lies at least 2^12 above the median non-zero |g| (asserted from
    the oracle's buffers); with h1_units, half the features lie 2^20 below the
    others as well."""
    pp = _params(True, h1_small)
    dev, ref, mag, orc = _device_and_oracle(ctx, "ppo", pp)
    over_median, over_rowmax = _g_range(orc, "ppo", pp)
    print("dw2pair wide g (h1_small=%s): G / median non-zero |g| = 2^%.1f, "
          "G / median row max |g| = 2^%.1f" % (h1_small, np.log2(over_median),
                                               np.log2(over_rowmax)))
    assert over_median >= 2.0 ** 12, over_median
    assert np.isfinite(dev).all()
    assert_grad_units(dev[0], ref[0], mag[0],
                      what="dw2pair wide g%s ppo epoch0" % (" h1_units" if h1_small else ""))


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_zero_advantages(ctx, algo):
    """Every transition terminal and V = 0 (zero value parameters): all
    advantages are exactly zero, so G = 0, and the policy gradients of every
    epoch must be exactly zero and finite."""
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_ADV, BUF_DONE, BUF_POLICY_GRADS
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=(H, H), rng_state=X0)
    pp = _params(False, False)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, np.zeros(tr.num_params(VALUE), np.float32))
    tr.rollout()
    tr.set_buffer(BUF_DONE, np.ones((T, N), np.uint8))
    tr.learn()
    assert tr.kernel_info()["policy_train"]["kernel"] == "policy_train_spec8_kernel"
    adv = tr.buffer(BUF_ADV)
    assert np.all(adv == 0.0), float(np.abs(adv).max())
    g = tr.buffer(BUF_POLICY_GRADS)
    assert np.isfinite(g).all()
    assert np.all(g == 0.0), float(np.abs(g).max())
    tr.close()
