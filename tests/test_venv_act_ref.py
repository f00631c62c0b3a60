"""Pins the host reference of xh_venv_act (tests/venv_act_ref.py) to the
oracle's own drivers: or_venv_run for the env transitions and the engine
order, a one-env PPO rollout of the oracle trainer for the picks and
p[choice], and the boundary-row construction of the GPU test.  CPU only."""
import numpy as np
import pytest

from sampling_ties import cumulative
from venv_act_ref import (BOUNDARY_N, BOUNDARY_X0, ActRef, boundary_rows,
                          mixed_rows, run)

from oracle import pyoracle as po


@pytest.mark.parametrize("B,D,N,offset,Ng", [(8, 2, 12, 0, 12),
                                            (32, 1, 9, 5, 20),
                                            (128, 3, 3, 0, 3)])
def test_reference_transitions_are_the_venv_drivers(B, D, N, offset, Ng):
    """The reference's own picks, fed to or_venv_run as actions, give its
    states, rewards, dones and final engine state."""
    S, x0 = 14, 991
    rows = mixed_rows(B + D, S, N, B)
    ref = run(B, D, N, x0, rows, n_global=Ng, offset=offset)
    drv = po.venv_run(B, D, N, x0, ref["action"], policy_draws=2, n_global=Ng,
                      offset=offset)
    np.testing.assert_array_equal(ref["bins"], drv["bins"])
    np.testing.assert_array_equal(ref["item"], drv["item"])
    np.testing.assert_array_equal(ref["reward"], drv["reward"])
    np.testing.assert_array_equal(ref["done"], drv["done"])
    assert ref["x_end"] == drv["x_end"]
    assert ref["done"].any() and not ref["done"].all(axis=0).all()
    # p[choice] is the bits of the row's entry
    s, e = np.indices(ref["action"].shape)
    np.testing.assert_array_equal(ref["pchoice"], rows[s, e, ref["action"]])
    # the stream positions: env e of step s stands at 2 Ng + 4 (s Ng + g)
    for s in (0, S):
        for e in (0, N - 1):
            assert ref["rng"][s, e] == po.minstd_jump(
                x0, 2 * Ng + 4 * (s * Ng + offset + e))


def test_argmax_draws_nothing():
    """ARGMAX on a policy_draws = 0 engine: first maxima, and the engine of a
    policy_draws = 0 or_venv_run."""
    B, D, N, S, x0 = 16, 2, 6, 10, 77
    rows = mixed_rows(3, S, N, B)
    rows[:, :, 5] = rows.max(axis=2)  # a repeated maximum
    ref = run(B, D, N, x0, rows, mode="argmax", policy_draws=0)
    np.testing.assert_array_equal(ref["action"], rows.argmax(axis=2))
    drv = po.venv_run(B, D, N, x0, ref["action"], policy_draws=0)
    np.testing.assert_array_equal(ref["bins"], drv["bins"])
    assert ref["x_end"] == drv["x_end"]


def test_one_env_run_is_the_trainers_rollout():
    """Rows from model_eval of a per-bin softmax model on Env.obs(): the
    picks and p[choice] of a one-env PPO rollout of the oracle trainer."""
    B, D, T, x0 = 8, 2, 24, 4242
    g = np.random.default_rng(1)
    pm = po.perbin_model(2 * D, [16, 16], po.OR_SOFTMAX)
    vm = po.full_model(B * 2 * D, [64, 32], 1)
    pp = (g.standard_normal(po.nparams(pm)) * 0.8).astype(np.float32)
    vp = (g.standard_normal(po.nparams(vm)) * 0.1).astype(np.float32)
    orc = po.Trainer(po.OR_PPO, B, D, 1, T, pm, pp, vm, vp, x0=x0)
    orc.rollout()
    ref = ActRef(B, D, 1, x0)
    acts, pch, dones = [], [], []
    for _ in range(T):
        rows = po.model_eval(pm, pp, ref.obs().reshape(1, -1))
        r = ref.act(rows)
        acts.append(r["action"][0])
        pch.append(r["pchoice"][0])
        dones.append(r["done"][0])
    np.testing.assert_array_equal(acts, orc.buf(po.BUF_STEP_CHOICE))
    np.testing.assert_array_equal(np.array(pch, np.float32),
                                  orc.buf(po.BUF_STEP_PCHOICE))
    np.testing.assert_array_equal(dones, orc.buf(po.BUF_STEP_DONE))
    assert ref.rng.state == orc.rng
    assert len(set(acts)) > 1


@pytest.mark.parametrize("B", [8, 64, 128])
def test_boundary_rows_straddle_the_draw(B):
    """The GPU test's construction: both rows' second boundary lies within
    1e-9 of u, on opposite sides, so or_discrete picks bins 1 and 2."""
    ref = ActRef(B, 2, BOUNDARY_N, BOUNDARY_X0)
    us, xs = ref.draws(), ref.streams()
    made = 0
    for e in range(BOUNDARY_N):
        pair = boundary_rows(us[e], B)
        if pair is None:
            continue
        made += 1
        ca, cn = cumulative(pair[0])[1], cumulative(pair[1])[1]
        assert abs(ca - us[e]) < 1e-9 and abs(cn - us[e]) < 1e-9
        assert (ca < us[e]) != (cn < us[e]) and ca != us[e] and cn != us[e]
        picks = {po.Rng(int(xs[e])).discrete(r) for r in pair}
        assert picks == {1, 2}
    assert made >= 4
