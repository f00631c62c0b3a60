"""Pins tests/rollout_tie_ref.py -- the placed draws, the arrangements and the
window replay of tests/test_gpu_rollout_ties.py -- to the oracle: canonical()
bit for bit, the pick as lower_bound in sampling_ties.cumulative, the replay
against oracle Trainer rollouts.  CPU only."""
import numpy as np
import pytest

import rollout_tie_ref as rt
from sampling_ties import cumulative

from oracle import pyoracle as po

BINS = [8, 16, 32, 64, 128]


def softmax_rows(seed, N, B, spread=3.0):
    """Seeded f32 softmax rows as the kernels form them: expf, an f32 sum, a
    division (the summation order does not matter here)."""
    g = np.random.default_rng(seed)
    z = (g.standard_normal((N, B)) * spread).astype(np.float32)
    ex = np.exp(z).astype(np.float32)
    return (ex / ex.sum(axis=1, dtype=np.float32)[:, None]).astype(np.float32)


def test_canonical_is_the_oracles_bit_for_bit():
    g = np.random.default_rng(5)
    xs = [1, 2, rt.M - 1, rt.M - 2, 16807, rt.A_INV2] + [
        int(v) for v in g.integers(1, rt.M, 4000)]
    # the states whose draw is the largest there is, and the smallest
    xs += rt.streams_for(1.0, "below") + rt.streams_for(0.0, "above")
    for x in xs:
        r = po.Rng(x)
        u = r.canonical()
        assert rt.canonical(x) == (u, r.state), x
        assert 0.0 <= u < 1.0
    # two steps back is two steps back
    for x in xs[:50]:
        assert rt.canonical(x * rt.A_INV2 % rt.M)[1] == x


@pytest.mark.parametrize("B", BINS)
def test_streams_lie_where_asked(B):
    rows = softmax_rows(B, 6, B)
    for row in rows:
        cp = cumulative(row)
        for k in range(B - 1):
            for side in ("below", "above"):
                xs = rt.streams_for(float(cp[k]), side)
                assert xs, (B, k, side)
                gaps = []
                for x in xs:
                    u = po.Rng(x).canonical()
                    assert 0.0 < abs(u - cp[k]) < rt.TOL
                    assert (u < cp[k]) == (side == "below")
                    gaps.append(abs(u - cp[k]))
                assert gaps == sorted(gaps)
    assert not rt.streams_for(1.0, "above")
    assert all(po.Rng(x).canonical() < 1.0 for x in rt.streams_for(1.0, "below"))


@pytest.mark.parametrize("B", BINS)
def test_arrangement_straddles_every_boundary(B):
    """The builder finds a stream for every target; the two sides of boundary k
    pick k and k + 1 unless a neighbouring entry is closer than the tolerance;
    the draw next to 1 picks B - 1; the controls stay outside the branch; the
    pick is the oracle's Rng.discrete and lower_bound in the cumulative table."""
    N = 2 * B + 2
    q0 = softmax_rows(100 + B, N, B)
    plan = rt.build(q0)
    assert plan["missing"] == []
    assert plan["engineered"].sum() == 2 * B and plan["control"].sum() == 2
    differ = 0
    for e in range(N):
        cp = cumulative(q0[e])
        x, k = int(plan["streams"][e]), int(plan["k"][e])
        u = po.Rng(x).canonical()
        assert u == plan["u"][e]
        pick = po.Rng(x).discrete(q0[e])
        assert pick == int(np.searchsorted(cp, u, "left")) == plan["pick"][e]
        if plan["control"][e]:
            assert rt.CONTROL_MIN < abs(u - cp[k]) < rt.CONTROL_MAX
            assert plan["gap"][e] > rt.CONTROL_MIN
            continue
        assert 0.0 < plan["gap"][e] < rt.TOL
        if k == B - 1:
            assert pick == B - 1 and 1.0 - u < 4.7e-10
            continue
        assert 0.0 < abs(u - cp[k]) < rt.TOL
        below = e % 2 == 0
        assert (u < cp[k]) == below
        crowded = (k > 0 and cp[k] - cp[k - 1] < rt.TOL) or cp[k + 1] - cp[k] < rt.TOL
        if not crowded:
            assert pick == (k if below else k + 1), (e, k, pick)
        if not below and pick != plan["pick"][e - 1]:
            differ += 1
    print("B=%d: %d engineered envs, %d of %d boundaries straddled"
          % (B, 2 * B, differ, B - 1))
    assert differ >= (B - 1) * 3 // 4


@pytest.mark.parametrize("B,G", [(8, 8), (16, 4), (32, 2), (64, 8), (64, 4)])
def test_single_arrangement(B, G):
    """One env per wave of G envs asks; the others are far from every boundary;
    the asking env takes every position of the wave."""
    N = 2 * G * G + 1
    q0 = softmax_rows(200 + B, N, B)
    plan = rt.build_single(q0, G)
    assert plan["missing"] == []
    for w in range((N + G - 1) // G):
        envs = list(range(w * G, min(N, (w + 1) * G)))
        ask = [e for e in envs if plan["engineered"][e]]
        assert len(ask) <= 1 and (ask or w * G + w % G >= N)
        for e in envs:
            if e in ask:
                assert 0.0 < plan["gap"][e] < rt.TOL
            else:
                assert plan["gap"][e] > rt.FAR
    assert len({int(e) % G for e in np.nonzero(plan["engineered"])[0]}) == G


@pytest.mark.parametrize("B", BINS)
def test_a_zero_probability_bin_is_never_picked(B):
    """Exact zeros make consecutive boundaries equal; draws on either side of
    the repeated boundary pick the bins around the zeros."""
    N = 2 * B + 2
    q0 = softmax_rows(300 + B, N, B)
    zero = [1, 2, B // 2, B - 2]
    q0[:, zero] = 0.0
    plan = rt.build(q0)
    assert plan["missing"] == []
    for e in range(N):
        cp = cumulative(q0[e])
        assert cp[1] == cp[2] == cp[0] and cp[B // 2] == cp[B // 2 - 1]
        x = int(plan["streams"][e])
        pick = po.Rng(x).discrete(q0[e])
        assert pick == plan["pick"][e]
        assert q0[e, pick] > 0.0, (e, pick)
    # the repeated boundary from both sides
    assert plan["pick"][2] == 0 and plan["pick"][3] == 3
    assert plan["pick"][4] == 0 and plan["pick"][5] == 3


def test_zeros_at_the_ends_leave_no_room_for_some_targets():
    """A row that starts or ends with zeros has boundaries at 0 and at 1: the
    builder reports the targets no draw can reach, and only those."""
    B = 16
    N = 2 * B + 2
    q0 = softmax_rows(17, N, B)
    q0[:, [0, B - 1]] = 0.0
    plan = rt.build(q0)
    assert plan["missing"]
    for e in plan["missing"]:
        assert rt.no_draw_there(cumulative(q0[e]), plan["k"][e], plan["side"][e])
        assert not plan["engineered"][e] and plan["gap"][e] > rt.FAR
    for e in range(N):
        assert q0[e, plan["pick"][e]] > 0.0
        assert plan["pick"][e] == po.Rng(int(plan["streams"][e])).discrete(q0[e])


@pytest.mark.parametrize("B,D,N,T,scale", [(8, 2, 6, 8, 0.8), (32, 1, 4, 8, 1.6),
                                           (128, 3, 2, 8, 1.3)])
def test_replay_is_the_trainers_rollout(B, D, N, T, scale):
    """Two windows of an oracle PPO trainer: on the trainer's own distributions
    (model_eval of its states) the replay gives its picks, p[choice], done
    flags, states and, window after window, its stream positions."""
    x0 = 977
    g = np.random.default_rng(B)
    pm = po.perbin_model(2 * D, [16, 16], po.OR_SOFTMAX)
    vm = po.full_model(B * 2 * D, [64, 32], 1)
    pp = (g.standard_normal(po.nparams(pm)) * scale).astype(np.float32)
    vp = (g.standard_normal(po.nparams(vm)) * 0.1).astype(np.float32)
    orc = po.Trainer(po.OR_PPO, B, D, N, T, pm, pp, vm, vp, lr_pi=0.0, lr_v=0.0, x0=x0)
    cfg = po.env_cfg(B, D)
    streams = np.array([po.minstd_jump(x0, 2 * N + 4 * T * e) for e in range(N)], np.uint32)
    dones = 0
    for w in range(2):
        orc.rollout()
        sb = orc.buf(po.BUF_STEP_BINS).reshape(N, T, B, D).swapaxes(0, 1)
        si = orc.buf(po.BUF_STEP_ITEM).reshape(N, T, D).swapaxes(0, 1)
        q = np.zeros((T, N, B), np.float32)
        for t in range(T):
            for e in range(N):
                env = rt._env(cfg, None, sb[t, e], si[t, e])
                q[t, e] = po.model_eval(pm, pp, env.obs()[None, :])[0]
        ref = rt.replay(B, D, sb[0], si[0], streams, q)
        np.testing.assert_array_equal(ref["action"],
                                      orc.buf(po.BUF_STEP_CHOICE).reshape(N, T).T)
        np.testing.assert_array_equal(
            ref["pold"].view(np.uint32),
            orc.buf(po.BUF_STEP_PCHOICE).reshape(N, T).T.view(np.uint32))
        np.testing.assert_array_equal(ref["done"], orc.buf(po.BUF_STEP_DONE).reshape(N, T).T)
        np.testing.assert_array_equal(ref["bins"][:T], sb)
        np.testing.assert_array_equal(ref["items"][:T], si)
        np.testing.assert_array_equal(ref["bins"][T],
                                      orc.buf(po.BUF_FINAL_BINS).reshape(N, B, D))
        np.testing.assert_array_equal(ref["items"][T],
                                      orc.buf(po.BUF_FINAL_ITEM).reshape(N, D))
        # the picks are lower_bound(u) in the cumulative table of the row
        for t in range(T):
            for e in range(N):
                assert ref["action"][t, e] == np.searchsorted(
                    cumulative(q[t, e]), ref["u"][t, e], "left")
        # env e's state after the window: x_e 16807^(4 T N); the engine's, env 0's
        for e in range(N):
            assert ref["rng"][e] == po.minstd_jump(int(streams[e]), 4 * T * N)
        assert ref["rng"][0] == orc.rng
        streams = ref["rng"]
        dones += int(ref["done"].sum())
        orc.learn()
    # the 8-bin case is the one with resets: 16 steps fill its bins
    assert dones > 0 or B > 8
    assert len(set(ref["action"].ravel().tolist())) > 1
