"""Pins tests/venv_items_ref.py (the restatement the GPU tests of general item
sets compare against) to the CPU oracle where the oracle can express the case:
its EnvCfg has two items, p_a and one capacity for every dim.  CPU only."""
import numpy as np
import pytest

from oracle import pyoracle as po
from venv_act_ref import ActRef, mixed_rows
from venv_items_ref import (DEFAULT_ITEMS, DEFAULT_WEIGHTS, ItemsRef,
                            pick_item, thresholds)

B, D, N, STEPS, X0 = 8, 2, 5, 40, 4242

# (item_a, item_b, p_a, cap)
CASES = [((4, 2), (1, 2), 0.4, 8), ((3, 1), (2, 2), 0.25, 6)]


class _OracleRef(ActRef):
    """ActRef on a given EnvCfg: the oracle's env, bernoulli(p_a), cap."""

    def __init__(self, cfg, N, x0):
        self.B, self.D, self.N = cfg.B, cfg.D, N
        self.Ng, self.offset, self.pd, self.k = N, 0, 2, 4
        self.cfg = cfg
        self.rng = po.Rng(x0)
        self.envs = [po.Env(cfg, self.rng) for _ in range(N)]


def _cfg(item_a, item_b, p_a, cap):
    cfg = po.env_cfg(B, D)
    cfg.cap, cfg.p_a = cap, p_a
    for d in range(D):
        cfg.item_a[d], cfg.item_b[d] = item_a[d], item_b[d]
    return cfg


def test_default_thresholds_are_exact():
    c = thresholds(DEFAULT_WEIGHTS)
    assert c.tolist() == [0.4, 1.0]
    assert thresholds([0.25, 0.75]).tolist() == [0.25, 1.0]


def test_thresholds_of_zero_weights():
    c = thresholds([0.0, 3.0, 0.0, 1.0, 0.0, 0.0])
    assert c[0] == 0.0 and c[1] == c[2] == 0.75
    assert c[3:].tolist() == [1.0, 1.0, 1.0]
    g = np.random.default_rng(0)
    drawn = {pick_item(c, u) for u in g.random(2000)}
    assert drawn == {1, 3}
    assert pick_item(c, 0.0) == 1 and pick_item(c, np.nextafter(1.0, 0)) == 3
    for K in (1, 5, 16):  # sixteenths and random weights: monotone, ends at 1
        for w in (np.ones(K), g.random(K) + 1e-3):
            c = thresholds(w)
            assert c[-1] == 1.0 and (np.diff(c) >= 0).all()


@pytest.mark.parametrize("case", CASES, ids=["default", "3x1-2x2-cap6"])
def test_the_restatement_is_the_oracle_bit_for_bit(case):
    item_a, item_b, p_a, cap = case
    if case == CASES[0]:
        assert [tuple(DEFAULT_ITEMS[D][0]), tuple(DEFAULT_ITEMS[D][1])] == [
            item_a, item_b]
    orc = _OracleRef(_cfg(*case), N, X0)
    ref = ItemsRef(B, D, N, X0, [item_a, item_b], [p_a, 1.0 - p_a], cap)
    rows = mixed_rows(3, STEPS, N, B)
    g = np.random.default_rng(1)
    ended = 0
    for s in range(STEPS):
        np.testing.assert_array_equal(ref.bins(), orc.bins())
        np.testing.assert_array_equal(ref.items(), orc.items())
        assert ref.obs().tobytes() == orc.obs().tobytes(), s
        assert ref.rng.state == orc.rng.state
        np.testing.assert_array_equal(ref.streams(), orc.streams())
        if s % 4 == 3:  # xh_venv_step's visit
            acts = g.integers(0, 2, N).astype(np.int32)
            want, got = orc.step(acts), ref.step(acts)
        else:
            want, got = orc.act(rows[s]), ref.act(rows[s])
        for name in ("action", "pchoice", "reward", "done"):
            np.testing.assert_array_equal(got[name], want[name], name)
        ended += int(want["done"].sum())
    assert ended > 0
    assert ref.rng.state == orc.rng.state


def test_apply_and_reset_of_the_single_env_are_the_oracles():
    case = CASES[1]
    rng = po.Rng(X0)
    env = po.Env(_cfg(*case), rng)
    ref = ItemsRef(B, D, 1, X0, [case[0], case[1]], [case[2], 1 - case[2]],
                   case[3])
    overs = 0
    for s in range(30):
        a = s % 2
        env.apply(a)
        over = ref.apply(a)
        assert over == bool((env.bins < 0).any())
        if over:
            overs += 1
            env.reset()
            ref.reset()
        np.testing.assert_array_equal(ref.envs[0].bins, env.bins)
        np.testing.assert_array_equal(ref.envs[0].item, env.item[:D])
        assert ref.rng.state == rng.state
    assert overs > 0
