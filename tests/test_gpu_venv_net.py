"""The device-resident nets of a venv learner (PolicyNet / ValueNet, xh_net_*)
on the GPU, against tests/venv_net_ref.py's float64 restatement: the fused
policy kernels' forward and gradient over every supported width pair and dims,
position invariance, grid caps and accumulation, the value net against the
layer launches it composes, the step against xh_clip_grad_norm +
xh_optimizer_apply, and the whole venv chain with the nets in it.  The inputs
and seeds are the ones tests/test_venv_net_ref.py holds plain float32
arithmetic to the same budgets on.  No torch."""
import numpy as np
import pytest

import venv_net_ref as ref
from conftest import assert_grad_units, grad_units

pytestmark = pytest.mark.gpu


def _policy_layers(D, widths):
    return [("conv1d_1", 2 * D, widths[0]), ("relu", 0, 0),
            ("conv1d_1", widths[0], widths[1]), ("relu", 0, 0),
            ("conv1d_1", widths[1], 1)]


def _value_layers(B, D, widths):
    return [("full", B * 2 * D, widths[0]), ("relu", 0, 0),
            ("full", widths[0], widths[1]), ("relu", 0, 0),
            ("full", widths[1], 1)]


@pytest.fixture(scope="module")
def nets(ctx):
    """One PolicyNet per (B, D, widths), made on first use, closed at the end."""
    from dependence_free_rl_amd import PolicyNet
    made = {}

    def get(B, D, widths):
        key = (B, D, widths)
        if key not in made:
            made[key] = PolicyNet(ctx, B, D, widths)
        made[key].set_grid_cap(0)
        return made[key]
    yield get
    for n in made.values():
        n.close()


@pytest.fixture(scope="module")
def venv_obs(ctx):
    """Observations of a real VecEnv on ITEMS[D] after a few first-fit steps:
    [N][B][2D] per (B, D)."""
    from dependence_free_rl_amd import VecEnv
    from dependence_free_rl_amd._lib import VENV_OBS
    got = {}

    def get(B, D, N):
        key = (B, D, N)
        if key not in got:
            items, cap = ref.ITEMS[D]
            v = VecEnv(ctx, N, bins=B, dims=D, rng_state=77 + B + D,
                       items=items, capacity=cap)
            for _ in range(6):
                v.act_heuristic("firstfit", write_obs=True)
            got[key] = v.get(VENV_OBS)
            v.close()
            assert got[key].any()
        return got[key]
    return get


# ---- 1. forward -----------------------------------------------------------
@pytest.mark.parametrize("rows,B,D,widths,seed", ref.policy_cases())
def test_forward_is_within_the_derived_bound(ctx, nets, venv_obs, rows, B, D,
                                             widths, seed):
    p, obs, _ = ref.case_inputs("policy", rows, B, D, widths, seed)
    real = venv_obs(B, D, rows)
    net = nets(B, D, widths)
    net.params = p
    assert net.num_params == p.size
    for name, x in (("made", obs), ("venv", real)):
        want, mag = ref.forward("policy", p, x, B, D, widths)
        bound = ref.forward_bound(D, widths, mag)
        # plain float32 arithmetic meets the bound on these inputs
        f32, _ = ref.forward("policy", p, x, B, D, widths, np.float32)
        assert np.all(np.abs(f32 - want) <= bound), name
        got = net.forward(x)
        assert got.shape == (rows, B) and got.dtype == np.float32
        err = np.abs(got - want) / bound
        print("net fwd %s %s: max err / bound %.3g" % (name, (rows, B, D, widths),
                                                        err.max()))
        assert np.all(err <= 1.0), (name, float(err.max()))


# ---- 2. position invariance ------------------------------------------------
@pytest.mark.parametrize("rows,B", [(40, 64), (9, 8)])
@pytest.mark.parametrize("widths", ref.WIDTHS)
def test_a_rows_logits_do_not_depend_on_its_position(ctx, nets, rows, B, widths):
    D = 2
    p, obs, _ = ref.case_inputs("policy", rows, B, D, widths, 31 + rows)
    net = nets(B, D, widths)
    net.params = p
    base = net.forward(obs)
    rng = np.random.default_rng(3)
    # whole observation rows, and the flat per-bin rows inside the block
    perm = rng.permutation(rows)
    np.testing.assert_array_equal(net.forward(obs[perm]), base[perm])
    flat = rng.permutation(rows * B)
    shuffled = obs.reshape(rows * B, 2 * D)[flat].reshape(rows, B, 2 * D)
    np.testing.assert_array_equal(net.forward(shuffled).ravel(),
                                  base.ravel()[flat])
    net.set_grid_cap(1)
    np.testing.assert_array_equal(net.forward(obs), base)


# ---- 3. gradient -------------------------------------------------------------
@pytest.mark.parametrize("rows,B,D,widths,seed", ref.policy_cases())
def test_gradient_against_the_reference_and_the_layer_launches(
        ctx, nets, rows, B, D, widths, seed):
    from dependence_free_rl_amd.trainer import model_forward, model_gradient
    p, obs, dout = ref.case_inputs("policy", rows, B, D, widths, seed)
    want, mag = ref.gradient("policy", p, obs, dout, B, D, widths)
    net = nets(B, D, widths)
    net.params = p
    net.grad = np.full(p.size, 7.0, np.float32)  # overwritten, not added to
    net.backward(obs, dout)
    got = net.grad
    # the comparator between kernels: the layer-by-layer launches on the same rows
    layers = _policy_layers(D, widths)
    x = obs.reshape(rows, B * 2 * D)
    acts = model_forward(ctx, layers, p, x)
    comp = model_gradient(ctx, layers, p, acts, dout)
    u_new, _, _ = grad_units(got, want, mag)
    u_old, _, _ = grad_units(comp, want, mag)
    p_new, p_old = np.percentile(u_new, 99), np.percentile(u_old, 99)
    print("net bwd %s: median %.3g p99 %.3g max %.3g units (layer launches: "
          "median %.3g p99 %.3g max %.3g)" % (
              (rows, B, D, widths), np.median(u_new), p_new, u_new.max(),
              np.median(u_old), p_old, u_old.max()))
    assert_grad_units(got, want, mag, what="net bwd %s" % ((rows, B, D, widths),))
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)


# ---- 4. grid and accumulation ------------------------------------------------
@pytest.mark.parametrize("rows,B,D,widths,seed", ref.grid_cases())
def test_grid_caps_and_accumulation(ctx, nets, rows, B, D, widths, seed):
    p, obs, dout = ref.case_inputs("policy", rows, B, D, widths, seed)
    want, mag = ref.gradient("policy", p, obs, dout, B, D, widths)
    net = nets(B, D, widths)
    net.params = p
    for cap in (1, 3):
        net.set_grid_cap(cap)
        net.backward(obs, dout)
        g = net.grad
        info = net.info()
        assert info["grid"]["backward"] == cap and info["slabs"] == cap, info
        assert_grad_units(g, want, mag, what="net bwd cap %d %s" % (cap, widths))
        net.backward(obs, dout)
        np.testing.assert_array_equal(net.grad, g)
    # accumulate: two halves against the whole, and against their f32 sum
    net.set_grid_cap(0)
    h = rows // 2
    net.backward(obs[:h], dout[:h])
    g0 = net.grad
    net.backward(obs[h:], dout[h:])
    g1 = net.grad
    net.backward(obs[:h], dout[:h])
    net.backward(obs[h:], dout[h:], accumulate=True)
    both = net.grad
    np.testing.assert_array_equal(both, g0 + g1)
    assert_grad_units(both, want, mag, what="net bwd accumulate %s" % (widths,))
    assert net.info()["grid"]["backward"] == (rows - h) * B // 64
    # all-zero loss gradients: every term is zero, so is every entry
    net.backward(obs, np.zeros_like(dout))
    assert not net.grad.any()


# ---- 5. value net --------------------------------------------------------------
@pytest.mark.parametrize("rows,B,D,widths,seed", ref.value_cases())
def test_value_net_is_the_layer_launches(ctx, rows, B, D, widths, seed):
    """ValueNet runs layer_forward / layer_gradient / layer_backward, the
    launches of xh_model_forward / xh_model_gradient, with the same split-K
    counts: bit-identical."""
    from dependence_free_rl_amd import ValueNet
    from dependence_free_rl_amd.trainer import model_forward, model_gradient
    p, obs, dout = ref.case_inputs("value", rows, B, D, widths, seed)
    net = ValueNet(ctx, B, D, widths)
    try:
        net.params = p
        layers = _value_layers(B, D, widths)
        acts = model_forward(ctx, layers, p, obs.reshape(rows, -1))
        out = net.forward(obs)
        assert out.shape == (rows,)
        np.testing.assert_array_equal(out, acts[-1].ravel())
        net.backward(obs, dout)
        g = net.grad
        np.testing.assert_array_equal(
            g, model_gradient(ctx, layers, p, acts, dout.reshape(rows, 1)))
        want, mag = ref.gradient("value", p, obs, dout, B, D, widths)
        assert_grad_units(g, want, mag, what="value net %s" % ((rows, B, D),))
        net.backward(obs, dout, accumulate=True)
        np.testing.assert_array_equal(net.grad, g + g)
        # fewer rows after more: the scratch stays, the result does not change
        net.backward(obs[:1], dout[:1])
        net.backward(obs, dout)
        np.testing.assert_array_equal(net.grad, g)
    finally:
        net.close()


# ---- 6. step ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
@pytest.mark.parametrize("max_norm", [0.0, 0.5, 1e6])
def test_step_is_the_clip_and_optimizer_launches(ctx, nets, kind, max_norm):
    from dependence_free_rl_amd import clip_grad_norm
    from dependence_free_rl_amd.trainer import optimizer_apply
    B, D, widths = 8, 2, (64, 32)
    net = nets(B, D, widths)
    rng = np.random.default_rng(11)
    p = ref.make_params("policy", B, D, widths, 5)
    n = p.size
    net.params = p
    wd = 0.01 if kind == "sgd" else 0.0
    net.set_optimizer(kind, 0.05, weight_decay=wd, beta1=0.8, beta2=0.95)
    assert net.step_count == 0
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in (1, 2, 3):
        g = rng.normal(0, 0.1, n).astype(np.float32)
        net.grad = g
        if max_norm > 0:
            log = net.step(max_norm, clip_log=True)
            g, norm, scale = clip_grad_norm(ctx, g, max_norm)
            assert log[0] == norm and log[1] == float(scale), (log, norm, scale)
            assert (scale < 1) == (max_norm == 0.5)
        else:
            net.step()
        p, m, v = optimizer_apply(ctx, kind, p, g, 0.05, weight_decay=wd,
                                  beta1=0.8, beta2=0.95, t=float(t), m=m, v=v)
        assert net.step_count == t
        np.testing.assert_array_equal(net.params, p)
        if kind != "sgd":
            np.testing.assert_array_equal(net.moments[0], m)
        if kind == "adam":
            np.testing.assert_array_equal(net.moments[1], v)
    net.step_count = 7
    assert net.step_count == 7
    net.set_optimizer("sgd", 0.0)
    assert net.step_count == 0 and not net.moments[0].any()


# ---- 7. the chain ----------------------------------------------------------------
def _chain(ctx, iterations=3):
    from dependence_free_rl_amd import (VLOSS_CLIPPED, VLOSS_K3_SUM,
                                        VLOSS_LOGR_SUM, VLOSS_ROWS,
                                        VENV_POLICY, PolicyNet, ValueNet,
                                        VecEnv)
    B, D, N, T, MB = 8, 2, 24, 5, 32
    items, cap = ref.ITEMS[D]
    venv = VecEnv(ctx, N, bins=B, dims=D, rng_state=99, items=items, capacity=cap)
    pol, val = PolicyNet(ctx, B, D, (64, 64)), ValueNet(ctx, B, D)
    pol.init(3)
    val.init(4)
    pol.set_optimizer("adam", 1e-3)
    val.set_optimizer("sgd", 1e-3)
    venv.set_record(T)
    venv.set_action_mask(True)
    venv.observe()
    rng = np.random.default_rng(8)
    stats = []
    try:
        for it in range(iterations):
            venv.rewind()
            for _ in range(T):
                pol.forward(venv, out=venv.device_ptr(VENV_POLICY))
                venv.act(None, kind="logits", write_obs=True, fetch=False)
            states = venv.record_obs("state")  # [(T + 1) N][B][2D]
            values = val.forward(states).reshape(T + 1, N)
            adv = venv.advantages(values, returns=("adv", "td_target"))
            perm = rng.permutation(T * N).astype(np.int32)
            for epoch in range(2):
                for first in range(0, T * N, MB):
                    count = min(MB, T * N - first)
                    obs = venv.record_obs("state", rows=perm, first=first,
                                          count=count)
                    res = venv.policy_loss(
                        pol.forward(obs), adv["adv"], kind="logits",
                        loss="clipped", rows=perm, first=first, count=count,
                        legal=True, values=val.forward(obs),
                        target=adv["td_target"], want_stats=True,
                        accumulate=first > 0)
                    pol.backward(obs, res["grad"], accumulate=first > 0)
                    val.backward(obs, res["dvalue"], accumulate=first > 0)
                stats.append(res["stats"])
                before = pol.params
                pol.step(max_norm=0.5)
                val.step()
                assert (pol.params != before).any()
            e0, e1 = stats[-2], stats[-1]
            assert e0[VLOSS_ROWS] == e1[VLOSS_ROWS] == T * N
            # epoch 0: the minibatch logits are the rollout's, bit for bit
            assert e0[VLOSS_CLIPPED] == 0 and e0[VLOSS_LOGR_SUM] == 0 \
                and e0[VLOSS_K3_SUM] == 0, e0
            assert e1[VLOSS_LOGR_SUM] != 0 and e1[VLOSS_K3_SUM] != 0, e1
        out = pol.params, val.params, pol.moments, np.array(stats)
        assert pol.step_count == val.step_count == 2 * iterations
        for a in (out[0], out[1], out[2][0], out[2][1], out[3]):
            assert np.isfinite(a).all()
        return out
    finally:
        pol.close()
        val.close()
        venv.close()


def test_the_chain_end_to_end_twice(ctx):
    a, b = _chain(ctx), _chain(ctx)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2][0], b[2][0])
    np.testing.assert_array_equal(a[2][1], b[2][1])
    np.testing.assert_array_equal(a[3], b[3])


def test_a_trainers_parameters_load_into_the_nets(ctx):
    from dependence_free_rl_amd import (POLICY, VALUE, PolicyNet, Trainer,
                                        ValueNet, XhError, init_policy,
                                        init_value)
    from dependence_free_rl_amd.trainer import model_eval
    B, D, widths = 64, 2, (128, 128)
    tr = Trainer(ctx, bins=B, dims=D, num_envs=16, steps=4, widths=widths)
    pol, val = PolicyNet(ctx, B, D, widths), ValueNet(ctx, B, D)
    try:
        assert pol.num_params == tr.num_params(POLICY)
        assert val.num_params == tr.num_params(VALUE)
        tr.set_params(POLICY, init_policy(D, *widths, seed=21))
        tr.set_params(VALUE, init_value(B, D, seed=22))
        pol.params = tr.params(POLICY)
        val.params = tr.params(VALUE)
        np.testing.assert_array_equal(pol.params, tr.params(POLICY))
        obs = ref.make_obs(6, B, D, 23)
        p = pol.params
        want, mag = ref.forward("policy", p, obs, B, D, widths)
        bound = ref.forward_bound(D, widths, mag)
        ev = model_eval(ctx, _policy_layers(D, widths), p,
                        obs.reshape(6, B * 2 * D))
        got = pol.forward(obs)
        assert np.all(np.abs(got - want) <= bound)
        assert np.all(np.abs(ev - want) <= bound)
        assert np.all(np.abs(got - ev) <= 2 * bound)
        tr.set_params(POLICY, pol.params)  # and back
        with pytest.raises(XhError):
            PolicyNet(ctx, B, D, (128, 32))
        with pytest.raises(XhError):
            ValueNet(ctx, 12, D)
        with pytest.raises(XhError):
            pol.set("params", np.zeros(3, np.float32))
    finally:
        pol.close()
        val.close()
        tr.close()
