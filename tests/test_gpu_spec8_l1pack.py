"""The config-3 train kernels after the changes to their vector waves
(dependence_free_rl_amd/csrc/policy_spec8_kernels.hip):
layer 1 of the H1 image as one bf16 MFMA per r-tile (the three exact bf16
parts packed along K, spec8_l1_layout.h) and the plain / KL-PPO builds' LDS
order (the f32 vectors first, the mask slots packed).  The checks hold as
well for a build with g (x) H1's f16 pair taken straight from the two factors
(XH_SP8_GHF=1, xh_split.h's split2h_x2g: measured slower and off).

Shape: 64 bins, 2-D, [128,128], the cases of test_gpu_e0_reuse.py: N = 48,
T = 4 (192 groups) at the test grids (one group per workgroup, J = 3, a grid
that is no multiple of 8 with unequal J, one workgroup running all 192), and
1, 2 and 3 groups in one workgroup (J = 1, 2, 3: the prologue's layer1(0) /
layer1(1), an odd J, the clamped look-ahead).  PPO with XH_E0_REUSE=0 (all
four epochs on the plain kernel, whose layer 1 changed) and with the default
(epoch 0 on the epoch-0 kernel, the later epochs on the plain one), actor-critic
and KL-PPO.  Every epoch's policy gradient is held to conftest's budgets
against the oracle, and epoch 0 to test_gpu_spec8.py's rule between kernels
against XH_TRAIN_KERNEL=split8wh, different source whose layer 1 and split did
not change.
"""
import numpy as np
import pytest

from conftest import GRAD_UNITS_P99_DRIFT, assert_grad_units, grad_units
from gpu_helpers import step_major

pytestmark = pytest.mark.gpu

B, D, H, WIDTHS = 64, 2, 128, (128, 128)
F0 = 2 * D
X0 = 4711
KERNEL = {"ppo": "policy_train_spec8_kernel", "ac": "policy_train_spec8_kernel",
          "klppo": "policy_train_spec8_kl_kernel"}
OTHER = {"ppo": "policy_train_split8wh_kernel", "ac": "policy_train_split8wh_kernel",
         "klppo": "policy_train_split8wh_kl_kernel"}
KL_WD = 1e-5

_oracles = {}
_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    return init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)


def _oracle(algo, N, T):
    """One oracle iteration per (algo, N, T), shared by the cases (read only):
    every epoch's gradients, their magnitudes and the sampled actions."""
    key = (algo, N, T)
    if key not in _oracles:
        from oracle import pyoracle as po
        pp, vp = _params()
        head = po.OR_SOFTMAX_XENT if algo == "ac" else po.OR_SOFTMAX
        kw = dict(wd_pi=KL_WD) if algo == "klppo" else dict(
            lr_pi=1e-5 if algo == "ac" else 1e-4, lr_v=1e-4 if algo == "ac" else 1e-5)
        orc = po.Trainer({"ppo": po.OR_PPO, "ac": po.OR_AC, "klppo": po.OR_KLPPO}[algo],
                         B, D, N, T, po.perbin_model(F0, list(WIDTHS), head), pp,
                         po.full_model(B * F0, [64, 32], 1), vp, x0=X0, **kw)
        orc.rollout()
        actions = step_major(orc.buf(po.BUF_STEP_CHOICE), N, T).copy()
        orc.learn()
        _oracles[key] = (np.asarray(orc.buf(po.BUF_POLICY_GRADS)).copy(),
                         np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).copy(), actions)
    return _oracles[key]


def _run(ctx, monkeypatch, algo, N, T, cap, e0=0, kernel=None, cache=True):
    """rollout() on the oracle's actions, learn(); XH_E0_REUSE = e0 (None: the
    default), XH_TRAIN_KERNEL = kernel."""
    key = (algo, N, T, cap, e0, kernel)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS
    if e0 is None:
        monkeypatch.delenv("XH_E0_REUSE", raising=False)
    else:
        monkeypatch.setenv("XH_E0_REUSE", str(e0))
    if kernel is None:
        monkeypatch.delenv("XH_TRAIN_KERNEL", raising=False)
    else:
        monkeypatch.setenv("XH_TRAIN_KERNEL", kernel)
    pp, vp = _params()
    kw = dict(wd_policy=KL_WD) if algo == "klppo" else {}
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0, train_grid_cap=cap, **kw)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if algo == "klppo":  # (test_gpu_klppo.py: the device replays the oracle's actions)
        tr.set_forced_actions(_oracle(algo, N, T)[2])
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


def _check(ctx, monkeypatch, algo, N, T, cap, e0):
    ref, mag, _ = _oracle(algo, N, T)
    new = _run(ctx, monkeypatch, algo, N, T, cap, e0=e0)
    old = _run(ctx, monkeypatch, algo, N, T, cap, e0=0, kernel="split8wh")
    assert new["info"]["policy_train"]["kernel"] == KERNEL[algo], new["info"]
    assert old["info"]["policy_train"]["kernel"] == OTHER[algo], old["info"]
    grid = new["info"]["train_grid"]
    g, g_o = new["grads"], old["grads"]
    npi = g.shape[1]
    r, m = ref.reshape(-1, npi), mag.reshape(-1, npi)
    assert g.shape == r.shape
    assert np.isfinite(g).all() and np.isfinite(new["params"]).all()
    u_new, _, _ = grad_units(g[0], r[0], m[0])
    u_old, _, _ = grad_units(g_o[0], r[0], m[0])
    p_new, p_old = float(np.percentile(u_new, 99)), float(np.percentile(u_old, 99))
    print("l1pack %s e0=%s N=%d T=%d grid=%d: epoch-0 p99 units %.3g (split8wh %.3g), "
          "median %.3g (split8wh %.3g)" % (algo, e0, N, T, grid, p_new, p_old,
                                           float(np.median(u_new)), float(np.median(u_old))))
    for ep in range(g.shape[0]):
        budget = {} if ep == 0 else {"p99_units": GRAD_UNITS_P99_DRIFT}
        assert_grad_units(g[ep], r[ep], m[ep],
                          what="l1pack %s e0=%s N%d T%d grid=%d epoch%d" % (
                              algo, e0, N, T, grid, ep), **budget)
    # test_gpu_spec8.py's rule between kernels, on the same inputs
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


CASES = [(48, 4, 0), (48, 4, 64), (48, 4, 5), (48, 4, 1),
         (1, 1, 1), (1, 2, 1), (1, 3, 1)]


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo_plain_kernel_every_epoch(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ppo", N, T, cap, e0=0)


@pytest.mark.parametrize("N,T,cap", CASES)
def test_ppo_default_epoch0_kernel(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ppo", N, T, cap, e0=None)


@pytest.mark.parametrize("N,T,cap", [(48, 4, 0), (1, 1, 1)])
def test_actor_critic(ctx, monkeypatch, N, T, cap):
    _check(ctx, monkeypatch, "ac", N, T, cap, e0=0)


def test_klppo(ctx, monkeypatch):
    _check(ctx, monkeypatch, "klppo", 48, 4, 0, e0=0)


@pytest.mark.parametrize("e0", [0, None], ids=["plain", "default"])
def test_deterministic(ctx, monkeypatch, e0):
    a = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=e0)
    b = _run(ctx, monkeypatch, "ppo", 48, 4, 0, e0=e0, cache=False)
    np.testing.assert_array_equal(a["grads"], b["grads"])
    np.testing.assert_array_equal(a["params"], b["params"])


# ---- the peaked policy of test_gpu_spec8_dw2pair.py (restated): g far below
# the launch's bound G, with h1_units half the H1 features 2^20 below the rest
PN, PT, PX0 = 32, 4, 8642
OB1 = H * F0
OW3 = OB1 + H + H * H + H
CLIP_EPS = 0.2
# epoch-0 p99 units of the plain kernel before these changes (the
# dW2 pair's figures: epoch 0 ran the plain kernel then)
PARENT_P99 = {False: 58.5, True: 80.4}


def _peaked_params(h1_small):
    from dependence_free_rl_amd import init_policy
    p = init_policy(D, H, H, seed=61).copy()
    p[OW3:OW3 + H] *= 32.0
    if h1_small:
        p[:OB1].reshape(H, F0)[: H // 2] *= 2.0 ** -20
        p[OB1:OB1 + H // 2] *= 2.0 ** -20
    return p.astype(np.float32)


@pytest.mark.parametrize("e0", [0, None], ids=["plain", "default"])
@pytest.mark.parametrize("h1_small", [False, True], ids=["g_wide", "g_wide_h1_units"])
def test_peaked_policy(ctx, monkeypatch, h1_small, e0):
    """XH_E0_REUSE=0 ("plain"): the asserted epoch 0 runs the plain kernel,
    whose layer 1 is the packed one.  The default: it runs the epoch-0 kernel
    (no layer 1), the later epochs the plain one."""
    from oracle import pyoracle as po
    from dependence_free_rl_amd import POLICY, VALUE, Trainer, init_value
    from dependence_free_rl_amd.trainer import BUF_ACTION, BUF_POLICY_GRADS
    if e0 is None:
        monkeypatch.delenv("XH_E0_REUSE", raising=False)
    else:
        monkeypatch.setenv("XH_E0_REUSE", str(e0))
    monkeypatch.delenv("XH_TRAIN_KERNEL", raising=False)
    pp, vp = _peaked_params(h1_small), init_value(B, D, seed=62)
    model = po.perbin_model(F0, [H, H], po.OR_SOFTMAX)
    orc = po.Trainer(po.OR_PPO, B, D, PN, PT, model, pp,
                     po.full_model(B * F0, [64, 32], 1), vp, lr_pi=1e-4, lr_v=1e-5, x0=PX0)
    tr = Trainer(ctx, algo="ppo", bins=B, dims=D, num_envs=PN, steps=PT, widths=(H, H),
                 rng_state=PX0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    tr.rollout()
    orc.rollout()
    np.testing.assert_array_equal(tr.buffer(BUF_ACTION),
                                  orc.buf(po.BUF_STEP_CHOICE).reshape(PN, PT).T)
    tr.learn()
    orc.learn()
    assert tr.kernel_info()["policy_train"]["kernel"] == KERNEL["ppo"]
    npi = tr.num_params(POLICY)
    dev = tr.buffer(BUF_POLICY_GRADS).reshape(-1, npi).copy()
    tr.close()
    ref = np.asarray(orc.buf(po.BUF_POLICY_GRADS)).reshape(-1, npi)
    mag = np.asarray(orc.buf(po.BUF_POLICY_GRADS_MAG)).reshape(-1, npi)
    # the launch bound G over the median non-zero |g| of epoch 0, from the
    # oracle's buffers: at least 2^12
    msk = orc.buf(po.BUF_ROW_IS_END) == 0
    rows = orc.buf(po.BUF_ROWS).reshape(-1, B * F0)[msk]
    A = orc.buf(po.BUF_ADVANTAGES).astype(np.float64)[msk]
    pold = orc.buf(po.BUF_ROW_POLD).astype(np.float64)[msk]
    ch = orc.buf(po.BUF_ROW_CHOICE)[msk]
    p = po.model_eval(model, pp, rows).astype(np.float64)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(ch)), ch] = 1.0
    g = np.abs((p - onehot) * A[:, None])
    G = np.max(np.abs(A) * np.maximum(1.0 + CLIP_EPS, 1.0 / pold))
    assert G / np.median(g[g > 0]) >= 2.0 ** 12
    u, _, _ = grad_units(dev[0], ref[0], mag[0])
    print("l1pack peaked policy (h1_small=%s, XH_E0_REUSE=%s): epoch-0 p99 units %.3g%s, "
          "median %.3g" % (h1_small, e0, float(np.percentile(u, 99)),
                           " (plain kernel before: %.3g)" % PARENT_P99[h1_small]
                           if e0 == 0 else "", float(np.median(u))))
    assert np.isfinite(dev).all()
    assert_grad_units(dev[0], ref[0], mag[0],
                      what="l1pack peaked%s ppo e0=%s epoch0" % (
                          " h1_units" if h1_small else "", e0))


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_zero_advantages(ctx, monkeypatch, algo):
    """Every transition terminal and V = 0: all advantages are exactly zero,
    and every epoch's policy gradient must be exactly zero."""
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import BUF_ADV, BUF_DONE, BUF_POLICY_GRADS
    monkeypatch.delenv("XH_E0_REUSE", raising=False)
    monkeypatch.delenv("XH_TRAIN_KERNEL", raising=False)
    N, T = 32, 4
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, _params()[0])
    tr.set_params(VALUE, np.zeros(tr.num_params(VALUE), np.float32))
    tr.rollout()
    tr.set_buffer(BUF_DONE, np.ones((T, N), np.uint8))
    tr.learn()
    assert tr.kernel_info()["policy_train"]["kernel"] == KERNEL[algo]
    assert np.all(tr.buffer(BUF_ADV) == 0.0)
    g = tr.buffer(BUF_POLICY_GRADS)
    assert np.isfinite(g).all()
    assert np.all(g == 0.0), float(np.abs(g).max())
    tr.close()
