"""The trainer rollouts' samplers with the draws PLACED on the boundaries of
discrete_distribution's cumulative table.

Every rollout claims libstdc++'s sequential discrete_distribution pick on its
own f32 probabilities: a fast pick from tree-ordered double sums, replaced by a
sequential restatement whenever a cumulative entry lies within 1e-9 of the
draw.  A free-running draw enters that branch about once in 1e7 steps, so the
restatements of sample_discrete<B> (xh_device.h), sample_step128_x
(policy_kernels.hip) and pack_step_groups (rollout_pack_kernels.hip) are run
here on purpose: a probe rollout records step 0's distributions
(record_distrib), tests/rollout_tie_ref.py finds for every env the minstd state
whose next draw lies within 8e-10 of a chosen boundary of the env's OWN
recorded row, a twin trainer with the same parameters and states receives those
states through set_buffer(BUF_RNG) and runs the window, and the window must
equal -- exactly, no env left out -- the replay of libstdc++'s pick and the
env's transition on the distributions the run itself recorded.

The full arrangement puts env 2k below and env 2k + 1 above boundary k for
every k (in the packed kernel: every (lane, register) position, and a tail
wave); two controls sit just outside the branch; a trainer whose env count must
be a multiple of 64 / B gets free-running envs up to that multiple.  The
single arrangement has one asking env per wave, its neighbours more than 1e-4
from all their boundaries: a segment that does not ask keeps its fast pick
while a neighbour restates.

What this does not tell apart: the fast path's partial sums from the sequential
ones.  They differ by about 1e-16 and the 2^31 streams cannot place a draw in a
window that narrow, so the test holds the restatement's RESULT (and the fast
pick's, in the envs that do not ask), not which path produced it."""
import numpy as np
import pytest

import rollout_tie_ref as rt

pytestmark = pytest.mark.gpu

X0, CAP = 20251, 8
SPLIT, WAVE, STEP = "rollout_split_kernel", "rollout_wave_kernel", "rollout_step_kernel"

# id: (B, D, H1, H2), environment, (kernel, logit_table, envs_per_wave), envs a
# wave's sampler holds (the single arrangement's G; None: one env per wave)
SHAPE64, SHAPE128 = (64, 2, 128, 128), (128, 3, 128, 128)
CASES = {
    "pack8": (SHAPE64, {}, (SPLIT, True, 8), 8),
    "pack16": (SHAPE64, {"XH_ROLLOUT_PACK_LANES": "16"}, (SPLIT, True, 4), 4),
    "table-wave": (SHAPE64, {"XH_ROLLOUT_TABLE": "1"}, (SPLIT, True, 1), None),
    "split-forward": (SHAPE64, {"XH_ROLLOUT_TABLE": "0"}, (SPLIT, False, 1), None),
    "f32-wave": (SHAPE64, {"XH_ROLLOUT_KERNEL": "f32"}, (WAVE, False, 0), None),
    "4-wave": (SHAPE64, {"XH_ROLLOUT_KERNEL": "4"}, (STEP, False, 0), None),
    "128-split": (SHAPE128, {}, ("rollout_split128_kernel", False, 0), None),
    "128-f32": (SHAPE128, {"XH_ROLLOUT_KERNEL": "f32"}, ("rollout_wave128_kernel", False, 0),
                None),
    "128-4": (SHAPE128, {"XH_ROLLOUT_KERNEL": "4"}, ("rollout_step128_kernel", False, 0), None),
    "32-split": ((32, 1, 64, 64), {}, (SPLIT, False, 2), 2),
    "32-4": ((32, 1, 64, 64), {"XH_ROLLOUT_KERNEL": "4"}, (STEP, False, 0), 2),
    "16": ((16, 2, 64, 64), {}, (STEP, False, 0), 4),
    "8-64-32": ((8, 2, 64, 32), {}, (STEP, False, 0), 8),
    "8-128-64": ((8, 2, 128, 64), {}, (STEP, False, 0), 8),
}
# the last layer's gain over the seeded initialisation: the logits of the seeded
# states then spread by about 5 units in every shape (and stay below 20)
GAIN = {SHAPE64: 2.5, SHAPE128: 6.0, (32, 1, 64, 64): 15.0, (16, 2, 64, 64): 7.0,
        (8, 2, 64, 32): 24.0, (8, 2, 128, 64): 7.0}
FULL = list(CASES)
SINGLE = [c for c in CASES if CASES[c][3]]
ENV_VARS = ("XH_ROLLOUT_PACK_LANES", "XH_ROLLOUT_TABLE", "XH_ROLLOUT_KERNEL", "XH_E0_REUSE",
            "XH_TRAIN_KERNEL")


def _env(monkeypatch, env):
    for k in ENV_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _params(shape, zeros=False):
    """A seeded initialisation with the last layer scaled so that the logits
    spread by a few units; zeros: hidden unit 0 of both layers carries
    -300 relu(1 - bin[0] / 2) to the logit: -300 and -150 for bin[0] = 0 and 1,
    far below expf's underflow, and nothing for the other bins (no logit grows:
    the kernels do not subtract the maximum)."""
    from dependence_free_rl_amd import init_policy, init_value
    B, D, H1, H2 = shape
    pp = init_policy(D, H1, H2, seed=31 + B).copy()
    F0 = 2 * D
    ob1 = H1 * F0
    oW2 = ob1 + H1
    ob2 = oW2 + H2 * H1
    ow3 = ob2 + H2
    assert pp.size == ow3 + H2 + 1
    pp[ow3:ow3 + H2] *= GAIN[shape]
    if zeros:
        pp[0:F0] = 0.0
        pp[0] = -4.0  # the observation is bin / capacity
        pp[ob1] = 1.0
        pp[oW2:oW2 + H1] = 0.0
        pp[oW2] = 1.0
        pp[ob2] = 0.0
        pp[ow3] = -300.0
    return pp, init_value(B, D, seed=32 + B)


def _states(shape, N, lo=0):
    """Seeded slot-0 states: bins anywhere in [lo, capacity], items of the item
    table."""
    from oracle import pyoracle as po
    B, D = shape[:2]
    g = np.random.RandomState(1000 + B)
    cfg = po.env_cfg(B, D)
    table = np.array([[cfg.item_a[d] for d in range(D)],
                      [cfg.item_b[d] for d in range(D)]], np.int8)
    bins = g.randint(lo, CAP + 1, (N, B, D)).astype(np.int8)
    for e in range(N):  # dimension 0 takes every value in every env (D = 1 has only these)
        bins[e, :, 0] = lo + g.permutation(B) % (CAP + 1 - lo)
    return bins, table[g.randint(0, 2, N)]


def _trainer(ctx, shape, N, T, pp, vp, states):
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    B, D, H1, H2 = shape
    tr = Trainer(ctx, algo="ppo", bins=B, dims=D, num_envs=N, steps=T, widths=(H1, H2),
                 rng_state=X0, record_distrib=True, lr_policy=0.0, lr_value=0.0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if states is not None:
        tr.set_env_state(0, *states)
    return tr


def _window(tr):
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_BINS, BUF_DONE, BUF_ITEMS,
                                                BUF_POLD, BUF_QOLD, BUF_RNG)
    return {"bins": tr.buffer(BUF_BINS), "items": tr.buffer(BUF_ITEMS),
            "action": tr.buffer(BUF_ACTION), "pold": tr.buffer(BUF_POLD),
            "done": tr.buffer(BUF_DONE), "q": tr.buffer(BUF_QOLD), "rng": tr.buffer(BUF_RNG),
            "info": tr.kernel_info()["rollout_step"]}


def _check_info(info, want):
    kernel, table, epw = want
    assert info["kernel"] == kernel, info
    assert bool(info["logit_table"]) == table, info
    assert info["envs_per_wave"] == epw, info


def _check_rows(q0, shape, zeros, envs=None):
    """Host checks of the probe's rows before the device is trusted with them:
    finite, normalised and -- in `envs` (default all) -- spread by a unit at
    least and mostly distinct."""
    B, D = shape[:2]
    assert np.isfinite(q0).all() and (q0 >= 0).all()
    np.testing.assert_allclose(q0.sum(-1, dtype=np.float64), 1.0, atol=1e-5)
    want = min(B // 4, (CAP + 1) ** D)
    for e, row in enumerate(q0):
        if envs is not None and not envs[e]:
            continue
        assert len(np.unique(row)) >= want, (e, len(np.unique(row)))
        pos = row[row > 0]
        assert pos.max() / pos.min() > np.e, (e, pos.max() / pos.min())  # a unit at least
    if zeros:
        nz = (q0 == 0).sum(-1)
        assert (nz >= 4).all() and (nz < B - 4).all(), nz
        # two equal consecutive boundaries in every row
        assert all((np.diff(rt.boundaries(r)) == 0).any() for r in q0)


def _run(ctx, monkeypatch, case, arrangement="full", T=3, zeros=False, second=False):
    shape, env, want, G = CASES[case]
    B, D = shape[:2]
    per = 64 // B if B <= 64 else 1  # the trainer's env count: a multiple of this
    if arrangement == "full":
        N = -(-(2 * B + 2) // per) * per
    else:
        N = -(-(2 * G * G + 1) // per) * per  # every position asks twice; a tail
    _env(monkeypatch, env)
    pp, vp = _params(shape, zeros)
    # second: bins that take the first window's items, so that few envs enter
    # the second window behind a reset (all bins but a few at capacity)
    states = _states(shape, N, lo=4 if second else 0)

    # the probe: step 0's distributions of the window the draws go into
    probe = _trainer(ctx, shape, N, T, pp, vp, states)
    probe.rollout()
    kept = None
    if second:
        kept = ~_window(probe)["done"].any(axis=0)  # no reset in the first window
        probe.learn()
        probe.rollout()
    pw = _window(probe)
    probe.close()
    _check_info(pw["info"], want)
    q0 = pw["q"][0]
    _check_rows(q0, shape, zeros, kept)
    if second:
        start = pw["bins"][0], pw["items"][0][:, :D]
        assert kept.sum() >= 3 * N // 4, kept.sum()
        assert (start[0] != states[0]).any(axis=(1, 2)).all()  # every env has moved on
    else:
        start = states
        np.testing.assert_array_equal(pw["bins"][0], states[0])
        np.testing.assert_array_equal(pw["items"][0][:, :D], states[1])

    plan = rt.build(q0) if arrangement == "full" else rt.build_single(q0, G)
    eng = plan["engineered"]
    for e in plan["missing"]:  # rows with zeros at an end: no draw on that side
        assert zeros and rt.no_draw_there(rt.boundaries(q0[e]), plan["k"][e], plan["side"][e])
    assert (plan["gap"][eng] > 0).all() and (plan["gap"][eng] < rt.TOL).all()
    assert (plan["gap"][~eng] > rt.CONTROL_MIN).all()
    if arrangement == "full":
        assert eng.sum() + len(plan["missing"]) == 2 * B and plan["control"].sum() == 2
        assert (plan["gap"][plan["control"]] < rt.CONTROL_MAX).all()
        assert (plan["gap"][2 * B + 2:] > rt.FAR).all()
    else:
        waves = -(-N // G)
        assert eng.sum() >= 2 * G and {int(e) % G for e in np.nonzero(eng)[0]} == set(range(G))
        for w in range(waves):
            envs = np.arange(w * G, min(N, (w + 1) * G))
            assert eng[envs].sum() <= 1
            assert (plan["gap"][envs[~eng[envs]]] > rt.FAR).all()

    # the twin: the same window with the placed streams
    from dependence_free_rl_amd.trainer import BUF_RNG
    twin = _trainer(ctx, shape, N, T, pp, vp, states)
    if second:
        twin.rollout()
        twin.learn()
    twin.set_buffer(BUF_RNG, plan["streams"])
    twin.rollout()
    tw = _window(twin)
    twin.close()
    _check_info(tw["info"], want)

    np.testing.assert_array_equal(tw["q"][0].view(np.uint32), q0.view(np.uint32))
    np.testing.assert_array_equal(tw["bins"][0], start[0])
    np.testing.assert_array_equal(tw["items"][0][:, :D], start[1])
    ref = rt.replay(B, D, start[0], start[1], plan["streams"], tw["q"])
    np.testing.assert_array_equal(ref["u"][0], plan["u"])
    np.testing.assert_array_equal(ref["action"][0], plan["pick"])

    # the straddle, on the host: what the replay says the two sides pick
    differ = pairs = 0
    if arrangement == "full":
        for k in range(B - 1):
            if eng[2 * k] and eng[2 * k + 1]:
                pairs += 1
                d = ref["action"][0, 2 * k] != ref["action"][0, 2 * k + 1]
                differ += int(d)
                assert (tw["action"][0, 2 * k] != tw["action"][0, 2 * k + 1]) == d, k
        assert differ >= pairs // 2  # the draws do straddle
        top = [e for e in (2 * B - 2, 2 * B - 1) if eng[e]]
        assert all(q0[e, ref["action"][0, e]] > 0 for e in top)
    print("rollout ties %s %s%s%s: N=%d, %d engineered envs (max gap %.2e), %d of %d "
          "boundaries picked differently from their two sides, %d resets"
          % (case, arrangement, " zeros" if zeros else "", " second-window" if second else "",
             N, int(eng.sum()), float(plan["gap"][eng].max()), differ, pairs,
             int(ref["done"].sum())))
    if zeros:
        assert (tw["q"][0][np.arange(N), tw["action"][0]] > 0).all()

    bad = np.nonzero(tw["action"][0] != ref["action"][0])[0]
    assert bad.size == 0, "step-0 picks differ in envs %s: boundary %s side %s device %s replay %s" % (
        bad[:16], plan["k"][bad[:16]], plan["side"][bad[:16]], tw["action"][0][bad[:16]],
        ref["action"][0][bad[:16]])
    np.testing.assert_array_equal(tw["action"], ref["action"])
    np.testing.assert_array_equal(tw["pold"].view(np.uint32), ref["pold"].view(np.uint32))
    np.testing.assert_array_equal(tw["done"], ref["done"])
    np.testing.assert_array_equal(tw["bins"][1:], ref["bins"][1:])
    np.testing.assert_array_equal(tw["items"][1:, :, :D], ref["items"][1:])
    assert not tw["items"][1:, :, D:].any()
    np.testing.assert_array_equal(tw["rng"], ref["rng"])
    return tw, ref, plan


@pytest.mark.parametrize("case", FULL)
def test_every_boundary_from_both_sides(ctx, monkeypatch, case):
    _run(ctx, monkeypatch, case)


@pytest.mark.parametrize("case", SINGLE)
def test_single_asking_segment(ctx, monkeypatch, case):
    _run(ctx, monkeypatch, case, arrangement="single")


def test_exact_zeros_packed(ctx, monkeypatch):
    """Bins whose logit lies below expf's underflow: equal consecutive
    boundaries, and a zero-probability bin is never picked."""
    _run(ctx, monkeypatch, "pack8", zeros=True)


@pytest.mark.parametrize("T", [3, 1])
def test_second_window_packed(ctx, monkeypatch, T):
    """The draws at step 0 of the second window: the launch that also moves
    slot T to slot 0 (src_slot)."""
    _run(ctx, monkeypatch, "pack8", T=T, second=True)
