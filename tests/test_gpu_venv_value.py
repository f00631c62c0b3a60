"""The value net read straight from a venv's recorded window
(ValueNet.forward_record / backward_record, xh_net_forward_record /
xh_net_backward_record) on the GPU, against tests/venv_net_ref.py's float64
restatement on the observations record_obs returns for the same rows, and
against the layer path ValueNet.forward / backward(record_obs(...)) as the
comparator.  The windows, cases and seeds are tests/venv_value_ref.py's, which
tests/test_venv_value_ref.py conditions on the CPU.  No torch."""

import numpy as np
import pytest

import venv_net_ref as nr
import venv_value_ref as vr
from conftest import assert_close, assert_grad_units, grad_units

pytestmark = pytest.mark.gpu

N, T = vr.N, vr.T


def _bits(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _make_venv(ctx, B, D, builtin):
    """A VecEnv holding the recorded window vr.window(B, D, builtin)."""
    from dependence_free_rl_amd import VecEnv, _lib
    w = vr.window(B, D, builtin)
    items, cap = vr.item_set(D, builtin)
    kw = {} if builtin else dict(items=items, capacity=cap)
    v = VecEnv(ctx, N, bins=B, dims=D, rng_state=w["x0"], policy_draws=2, **kw)
    v.set(_lib.VENV_BINS, w["preset"])
    v.set_record(T)
    for _ in range(T):
        v.act_heuristic("random")
    assert v.record_pos() == T
    return v


@pytest.fixture(scope="module")
def wins(ctx):
    """(venv, window, {view: record_obs of the whole view}) per (B, D,
    builtin), made on first use and left unchanged; the device's window is the
    restatement's, bit for bit."""
    made = {}

    def get(B, D, builtin=False):
        key = (B, D, builtin)
        if key not in made:
            v, w = _make_venv(ctx, B, D, builtin), vr.window(B, D, builtin)
            obs = {view: v.record_obs(view) for view in ("state", "next")}
            for view in obs:
                _bits(obs[view], w[view], "%s view of %s" % (view, key))
            made[key] = (v, w, obs)
        return made[key]
    yield get
    for v, _, _ in made.values():
        v.close()


@pytest.fixture(scope="module")
def nets(ctx):
    from dependence_free_rl_amd import ValueNet
    made = {}

    def get(B, D):
        if (B, D) not in made:
            made[(B, D)] = ValueNet(ctx, B, D)
        made[(B, D)].set_grid_cap(0)
        return made[(B, D)]
    yield get
    for n in made.values():
        n.close()


# ---- 1. forward ---------------------------------------------------------------
@pytest.mark.parametrize("B,D,builtin", vr.WINDOWS)
def test_forward_is_within_the_derived_bound(ctx, wins, nets, B, D, builtin):
    venv, w, obs = wins(B, D, builtin)
    net = nets(B, D)
    p = vr.make_params(B, D, 40 + B + D)
    net.params = p
    for view, total in (("state", vr.STATE_ROWS), ("next", vr.NEXT_ROWS)):
        want, mag = nr.forward("value", p, obs[view], B, D, vr.WIDTHS)
        bound = vr.forward_bound(B, D, mag)
        got = net.forward_record(venv, view)
        assert got.shape == (total,) and got.dtype == np.float32
        info = net.info()  # describes the last call
        assert info["kernels"][0] == "net_value_fwd_kernel", info
        assert info["math"] == "f32_mfma_16x16x4", info
        layer = net.forward(obs[view])
        assert net.info()["kernels"][0] == "layer_forward"
        e_new = np.abs(got - want) / bound
        e_old = np.abs(layer - want) / bound
        print("value fwd record %s %s: max err / bound %.3g (layer path %.3g)"
              % ((B, D, builtin), view, e_new.max(), e_old.max()))
        assert np.all(e_new <= 1.0), (view, float(e_new.max()))
        assert np.all(e_old <= 1.0), (view, float(e_old.max()))
        assert np.all(np.abs(got.astype(np.float64) - layer) <= 2 * bound), view
    venv.synchronize()


# ---- 2. position and grid invariance ---------------------------------------------
@pytest.mark.parametrize("B,D", vr.SHAPES)
def test_a_rows_value_does_not_depend_on_position_or_grid(ctx, wins, nets, B, D):
    venv, _, _ = wins(B, D)
    net = nets(B, D)
    net.params = vr.make_params(B, D, 41 + B + D)
    rng = np.random.default_rng(5)
    for view, total in (("state", vr.STATE_ROWS), ("next", vr.NEXT_ROWS)):
        base = net.forward_record(venv, view)
        assert net.info()["grid"]["forward"] == -(-total // 64)
        _bits(net.forward_record(venv, view), base, "two runs")
        perm = rng.permutation(total).astype(np.int32)
        _bits(net.forward_record(venv, view, rows=perm), base[perm], "rows=perm")
        for count in (1, 9, 63, 65):
            _bits(net.forward_record(venv, view, first=7, count=count),
                  base[7:7 + count], "first / count %d" % count)
            _bits(net.forward_record(venv, view, rows=perm, first=5, count=count),
                  base[perm[5:5 + count]], "list, first / count %d" % count)
        for cap in (1, 3):
            net.set_grid_cap(cap)
            _bits(net.forward_record(venv, view), base, "grid cap %d" % cap)
            assert net.info()["grid"]["forward"] == min(cap, -(-total // 64))
        net.set_grid_cap(0)
    venv.synchronize()


# ---- 3. gradient --------------------------------------------------------------------
@pytest.mark.parametrize("B,D,count,seed", vr.grad_cases())
def test_gradient_against_the_reference_and_the_layer_path(ctx, wins, nets, B, D,
                                                           count, seed):
    venv, w, _ = wins(B, D)
    net = nets(B, D)
    p, rows, dout = vr.grad_inputs(B, D, count, seed)
    view = vr.grad_view(count)
    obs = venv.record_obs(view, rows=rows)
    _bits(obs, w[view][rows], "the case's rows")
    want, mag = nr.gradient("value", p, obs, dout, B, D, vr.WIDTHS)
    net.params = p
    net.grad = np.full(p.size, 7.0, np.float32)  # overwritten, not added to
    net.backward_record(venv, dout, view=view, rows=rows)
    got = net.grad
    net.backward(obs, dout)  # the comparator: the layer launches on these rows
    comp = net.grad
    u_new, _, _ = grad_units(got, want, mag)
    u_old, _, _ = grad_units(comp, want, mag)
    p_new, p_old = np.percentile(u_new, 99), np.percentile(u_old, 99)
    print("value bwd record %s: median %.3g p99 %.3g max %.3g units (layer "
          "path: median %.3g p99 %.3g max %.3g)" % (
              (B, D, count, view), np.median(u_new), p_new, u_new.max(),
              np.median(u_old), p_old, u_old.max()))
    assert_grad_units(got, want, mag,
                      what="value bwd record %s" % ((B, D, count, view),))
    assert p_new <= 2.0 * p_old + 2.0, (p_new, p_old)
    venv.synchronize()


# ---- 4. accumulation and determinism ---------------------------------------------
@pytest.mark.parametrize("B,D,count,seed", vr.grid_cases())
def test_grid_caps_accumulation_and_exact_zeros(ctx, wins, nets, B, D, count, seed):
    venv, w, _ = wins(B, D)
    net = nets(B, D)
    p, rows, dout = vr.grad_inputs(B, D, count, seed)
    want, mag = nr.gradient("value", p, w["state"][rows], dout, B, D, vr.WIDTHS)
    net.params = p
    for cap in (1, 3):
        net.set_grid_cap(cap)
        net.backward_record(venv, dout, rows=rows)
        g = net.grad
        info = net.info()
        assert info["grid"]["backward"] == cap and info["slabs"] == cap, info
        assert info["kernels"][1] == "net_value_bwd_kernel", info
        assert_grad_units(g, want, mag,
                          what="value bwd record cap %d %s" % (cap, (B, D)))
        net.backward_record(venv, dout, rows=rows)
        _bits(net.grad, g, "two runs at cap %d" % cap)
    net.set_grid_cap(0)
    # accumulate: the f32 sum of the two reduced gradients, one add per entry
    h = count // 2 + 5
    net.backward_record(venv, dout[:h], rows=rows, first=0, count=h)
    g0 = net.grad
    net.backward_record(venv, dout[h:], rows=rows, first=h, count=count - h)
    g1 = net.grad
    net.backward_record(venv, dout[:h], rows=rows, first=0, count=h)
    net.backward_record(venv, dout[h:], rows=rows, first=h, count=count - h,
                        accumulate=True)
    both = net.grad
    _bits(both, g0 + g1, "accumulate")
    assert_grad_units(both, want, mag, what="value bwd record accumulate %s"
                      % ((B, D),))
    # exact-zero dout rows contribute exact zeros: whichever row they name ...
    net.backward_record(venv, dout, rows=rows)
    g = net.grad
    zero = dout == 0
    assert zero.any()
    other = rows.copy()
    other[zero] = (other[zero] + N + 1) % vr.STATE_ROWS
    net.backward_record(venv, dout, rows=other)
    _bits(net.grad, g, "zero-dout rows moved")
    # ... and all of them zero: every entry is zero
    net.backward_record(venv, np.zeros_like(dout), rows=rows)
    assert not net.grad.any()
    venv.synchronize()


# ---- 5. bad rows and refusals -------------------------------------------------------
def test_rows_outside_the_view_are_left_out_and_reported(ctx, wins, nets):
    from dependence_free_rl_amd import XhError
    B, D = 8, 2
    venv, _, _ = wins(B, D)
    net = nets(B, D)
    net.params = vr.make_params(B, D, 77)
    rng = np.random.default_rng(6)
    for view, total in (("state", vr.STATE_ROWS), ("next", vr.NEXT_ROWS)):
        base = net.forward_record(venv, view)
        rows = rng.permutation(total)[:70].astype(np.int32)  # two tiles
        bad = np.array([3, 66])
        rows_bad = rows.copy()
        rows_bad[3], rows_bad[66] = -1, total
        sentinel = np.float32(-12345.5)
        out_dev = net._scratch("test_out", 70 * 4)
        net._upload(out_dev, np.full(70, sentinel, np.float32))
        assert net.forward_record(venv, view, rows=rows_bad, out=out_dev) is None
        got = net._download(out_dev, (70,))
        assert np.all(got[bad] == sentinel)
        good = np.ones(70, bool)
        good[bad] = False
        _bits(got[good], base[rows[good]], "the other rows")
        with pytest.raises(XhError, match="outside"):
            venv.synchronize()
        venv.synchronize()  # reported once
        # the gradient: those rows add nothing
        dout = rng.normal(0, 1, 70).astype(np.float32)
        net.backward_record(venv, dout, view=view, rows=rows_bad)
        g_bad = net.grad
        with pytest.raises(XhError, match="outside"):
            venv.synchronize()
        d0 = dout.copy()
        d0[bad] = 0.0
        net.backward_record(venv, d0, view=view, rows=rows)
        _bits(g_bad, net.grad, "bad rows add nothing (%s)" % view)
        assert g_bad.any()
        venv.synchronize()


def test_refusals_name_their_cause(ctx, wins, nets):
    from dependence_free_rl_amd import PolicyNet, ValueNet, VecEnv, XhError, _lib
    B, D = 8, 2
    venv, _, _ = wins(B, D)
    net = nets(B, D)
    out_dev = net._scratch("test_out", 256 * 4)
    lib = _lib.lib

    def refused(call, status, word):
        assert call() == status
        msg = lib.xh_last_error().decode()
        assert word in msg, msg

    pol = PolicyNet(ctx, B, D, (64, 32))
    wide = ValueNet(ctx, B, D, (32, 32))
    bins16 = ValueNet(ctx, 16, D)
    dims3 = ValueNet(ctx, B, 3)
    bare = VecEnv(ctx, N, bins=B, dims=D)
    try:
        for n, word in ((pol, "not a value net"), (wide, "widths"),
                        (bins16, "16 x 2"), (dims3, "8 x 3")):
            refused(lambda: lib.xh_net_forward_record(
                n.h, venv.h, _lib.VOBS_STATE, None, 0, 4, out_dev),
                _lib.XH_ERR_INVALID, word)
            refused(lambda: lib.xh_net_backward_record(
                n.h, venv.h, _lib.VOBS_STATE, None, 0, 4, out_dev, 0),
                _lib.XH_ERR_INVALID, word)
        with pytest.raises(XhError, match="widths"):
            wide.forward_record(venv)
        refused(lambda: lib.xh_net_forward_record(
            net.h, bare.h, _lib.VOBS_STATE, None, 0, 4, out_dev),
            _lib.XH_ERR_STATE, "no record")
        refused(lambda: lib.xh_net_backward_record(
            net.h, bare.h, _lib.VOBS_STATE, None, 0, 4, out_dev, 0),
            _lib.XH_ERR_STATE, "no record")
        with pytest.raises(XhError, match="no record"):
            net.forward_record(bare, count=4)
        refused(lambda: lib.xh_net_forward_record(
            net.h, venv.h, _lib.VOBS_STATE, None, 0, -1, out_dev),
            _lib.XH_ERR_INVALID, "count -1")
        refused(lambda: lib.xh_net_forward_record(
            net.h, venv.h, _lib.VOBS_STATE, None, 0, 4, None),
            _lib.XH_ERR_INVALID, "null out_dev")
        refused(lambda: lib.xh_net_backward_record(
            net.h, venv.h, _lib.VOBS_STATE, None, 0, 4, None, 0),
            _lib.XH_ERR_INVALID, "null dout_dev")
        refused(lambda: lib.xh_net_forward_record(
            net.h, venv.h, 7, None, 0, 4, out_dev), _lib.XH_ERR_INVALID, "view 7")
        # a run past the view without a list, as record_obs refuses it
        refused(lambda: lib.xh_net_forward_record(
            net.h, venv.h, _lib.VOBS_NEXT, None, vr.NEXT_ROWS - 1, 2, out_dev),
            _lib.XH_ERR_INVALID, "rows")
        ctx2 = type(ctx)(device=0)
        try:
            far = ValueNet(ctx2, B, D)
            refused(lambda: lib.xh_net_forward_record(
                far.h, venv.h, _lib.VOBS_STATE, None, 0, 4, out_dev),
                _lib.XH_ERR_INVALID, "different contexts")
            far.close()
        finally:
            ctx2.close()
        venv.synchronize()
    finally:
        for x in (pol, wide, bins16, dims3, bare):
            x.close()


# ---- 6. the chain -------------------------------------------------------------------
def _chain(ctx, record, iterations):
    """test_gpu_venv_net.py's end-to-end chain; record: the value calls are
    the record calls."""
    from dependence_free_rl_amd import VENV_POLICY, PolicyNet, ValueNet, VecEnv
    B, D, MB = 8, 2, 32
    items, cap = nr.ITEMS[D]
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
    try:
        for it in range(iterations):
            venv.rewind()
            for _ in range(T):
                pol.forward(venv, out=venv.device_ptr(VENV_POLICY))
                venv.act(None, kind="logits", write_obs=True, fetch=False)
            if record:
                values = val.forward_record(venv, "state")
            else:
                values = val.forward(venv.record_obs("state"))
            adv = venv.advantages(values.reshape(T + 1, N),
                                  returns=("adv", "td_target"))
            perm = rng.permutation(T * N).astype(np.int32)
            for epoch in range(2):
                for first in range(0, T * N, MB):
                    count = min(MB, T * N - first)
                    at = dict(rows=perm, first=first, count=count)
                    obs = venv.record_obs("state", **at)
                    v = val.forward_record(venv, "state", **at) if record \
                        else val.forward(obs)
                    res = venv.policy_loss(
                        pol.forward(obs), adv["adv"], kind="logits",
                        loss="clipped", legal=True, values=v,
                        target=adv["td_target"], want_stats=True,
                        accumulate=first > 0, **at)
                    pol.backward(obs, res["grad"], accumulate=first > 0)
                    if record:
                        val.backward_record(venv, res["dvalue"], "state",
                                            accumulate=first > 0, **at)
                    else:
                        val.backward(obs, res["dvalue"], accumulate=first > 0)
                pol.step(max_norm=0.5)
                val.step()
        venv.synchronize()
        out = pol.params, val.params, pol.moments
        for a in (out[0], out[1], out[2][0], out[2][1]):
            assert np.isfinite(a).all()
        return out
    finally:
        pol.close()
        val.close()
        venv.close()


def test_the_chain_on_the_record_calls(ctx):
    a, b = _chain(ctx, True, 3), _chain(ctx, True, 3)
    _bits(a[0], b[0], "policy parameters")
    _bits(a[1], b[1], "value parameters")
    _bits(a[2][0], b[2][0], "first moments")
    _bits(a[2][1], b[2][1], "second moments")
    fused, layer = _chain(ctx, True, 1), _chain(ctx, False, 1)
    assert (fused[1] != val_init(ctx)).any()
    assert_close(fused[1], layer[1], what="value parameters after one iteration")


def val_init(ctx):
    from dependence_free_rl_amd.trainer import init_value
    return init_value(8, 2, 64, 32, seed=4)
