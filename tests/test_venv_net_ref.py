"""The reference of the device-resident nets' GPU tests, checked on the host:
venv_net_ref's float64 forward and gradient against finite differences, and
the budgets of tests/test_gpu_venv_net.py against what plain float32
arithmetic gives on every input those tests use (so a budget the kernels miss
is the kernels' doing, not the inputs')."""
import numpy as np
import pytest

import venv_net_ref as ref
from conftest import assert_grad_units


@pytest.mark.parametrize("kind,B,D,widths", [("policy", 3, 2, (5, 4)),
                                             ("value", 3, 1, (6, 3))])
def test_float64_gradient_is_the_finite_difference(kind, B, D, widths):
    rng = np.random.default_rng(5)
    rows = 4
    n = sum(fi * fo + fo for fi, fo in zip(ref._sizes(kind, B, D, widths)[:-1],
                                           ref._sizes(kind, B, D, widths)[1:]))
    p = rng.normal(0, 0.7, n)
    obs = rng.normal(0, 1, (rows, B, 2 * D))
    dout = rng.normal(0, 1, (rows, B) if kind == "policy" else rows)
    g, mag = ref.gradient(kind, p, obs, dout, B, D, widths)
    assert np.all(mag >= np.abs(g) * (1 - 1e-12))

    def loss(q):
        out, m = ref.forward(kind, q, obs, B, D, widths)
        assert np.all(m >= np.abs(out) * (1 - 1e-12))
        return float((out * dout).sum())

    h = 1e-6
    for i in range(n):
        e = np.zeros(n)
        e[i] = h
        fd = (loss(p + e) - loss(p - e)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * max(1.0, abs(g[i])), (i, fd, g[i])


def test_forward_by_hand():
    # one bin, one dim: x = (0.5, 0.25); h1 = relu(2 * 0.5 - 4 * 0.25 + 1) = 1,
    # h2 = relu(-3 * 1 + 1) = 0 and relu(2 * 1 + 0) = 2, logit = 5 * 0 + 7 * 2 - 1
    p = np.array([2, -4, 1, -3, 2, 1, 0, 5, 7, -1], np.float64)
    obs = np.array([[[0.5, 0.25]]])
    out, mag = ref.forward("policy", p, obs, 1, 1, (1, 2))
    assert out.tolist() == [[13.0]]
    # mag: h1 3, h2 (3 * 3 + 1, 2 * 3), logit 5 * 10 + 7 * 6 + 1
    assert mag.tolist() == [[93.0]]


@pytest.mark.parametrize("rows,B,D,widths,seed",
                         ref.policy_cases() + ref.grid_cases())
def test_float32_policy_meets_the_gpu_budgets(rows, B, D, widths, seed):
    p, obs, dout = ref.case_inputs("policy", rows, B, D, widths, seed)
    out, mag = ref.forward("policy", p, obs, B, D, widths)
    out32, _ = ref.forward("policy", p, obs, B, D, widths, np.float32)
    assert out32.dtype == np.float32
    assert np.all(np.abs(out32 - out) <= ref.forward_bound(D, widths, mag))
    g, gmag = ref.gradient("policy", p, obs, dout, B, D, widths)
    g32, _ = ref.gradient("policy", p, obs, dout, B, D, widths, np.float32)
    assert g32.dtype == np.float32
    assert_grad_units(g32, g, gmag, what="f32 policy %s" % ((rows, B, D, widths),))
    # exact-zero rows and masked bins are in, and something is left
    assert (dout[1::4] == 0).all() and (dout != 0).any()


@pytest.mark.parametrize("rows,B,D,widths,seed", ref.value_cases())
def test_float32_value_meets_the_gpu_budgets(rows, B, D, widths, seed):
    p, obs, dout = ref.case_inputs("value", rows, B, D, widths, seed)
    g, gmag = ref.gradient("value", p, obs, dout, B, D, widths)
    g32, _ = ref.gradient("value", p, obs, dout, B, D, widths, np.float32)
    assert_grad_units(g32, g, gmag, what="f32 value %s" % ((rows, B, D, widths),))
