"""The 64-bin 2-D table rollout with several envs per wave
(dependence_free_rl_amd/csrc/rollout_pack_kernels.hip on rollout_pack_layout.h;
DESIGN.md §3.0g): a wave steps 64 / L envs, lane = L-th part of an env's bins,
instead of one env with lane = bin.

Bit identity with the one-env-per-wave table kernel is the yardstick: every
case runs the default path and XH_ROLLOUT_TABLE=1 (rollout_split_kernel's table
launch) in the same process and compares for exact equality every window's
bins and items (all T + 1 slots), actions, p_old and done flags, the rng
states, the recorded distributions / last-step logits where the case records
them, the env state the next window starts from, and after the iterations both
nets' parameters and the state digests.  From the second iteration on the
launch also moves slot T to slot 0 (src_slot).

The policy prefers the fuller bins (one hidden unit per layer carries
12 (1 - bin[0] / capacity) to the logit, on top of the seeded initialisation),
so episodes last a few steps and every case sees resets; each case asserts its
done count.  The learning rate is divided by the rows (lr_scale_rows, as the
benchmark runs), so the updates keep that preference over the iterations."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, D, WIDTHS = 64, 2, (128, 128)
H1, H2 = WIDTHS
X0 = 4711
KERNEL = "rollout_split_kernel"
CAP = 8
PACKED = (4, 8, 16)  # envs per wave a packed layout can have

_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    pp = init_policy(D, *WIDTHS, seed=71).copy()
    F0 = 2 * D
    oW1, ob1 = 0, H1 * F0
    oW2 = ob1 + H1
    ob2 = oW2 + H2 * H1
    ow3 = ob2 + H2
    assert pp.size == ow3 + H2 + 1
    # hidden unit 0 of both layers: relu(1 - bin[0] / 8) -> 12 x that in the logit
    pp[oW1:oW1 + F0] = (-1.0, 0.0, 0.0, 0.0)
    pp[ob1] = 1.0
    pp[oW2:oW2 + H1] = 0.0
    pp[oW2] = 1.0
    pp[ob2] = 0.0
    pp[ow3] = 12.0
    return pp, init_value(B, D, seed=72)


def _env(monkeypatch, table):
    if table is None:
        monkeypatch.delenv("XH_ROLLOUT_TABLE", raising=False)
    else:
        monkeypatch.setenv("XH_ROLLOUT_TABLE", str(table))
    monkeypatch.delenv("XH_E0_REUSE", raising=False)


def _run(ctx, monkeypatch, table, algo="ppo", N=48, T=4, iters=2, record=False, forced=None,
         states=None):
    skey = None if states is None else b"".join(
        bytes([e]) + b.tobytes() + i.tobytes() for e, (b, i) in sorted(states.items()))
    key = (table, algo, N, T, iters, record, None if forced is None else forced.tobytes(), skey)
    if key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_BINS, BUF_DONE, BUF_ITEMS,
                                                BUF_LOGITS, BUF_POLD, BUF_PROBS, BUF_QOLD,
                                                BUF_RNG)
    _env(monkeypatch, table)
    pp, vp = _params()
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0, lr_scale_rows=True)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if record:
        tr.set_record_last_step(True)
    if states:
        for e, (bins, item) in states.items():
            tr.set_env_state(e, bins[None], item[None])
    if forced is not None:
        tr.set_forced_actions(forced)
    out = {"windows": [], "info": []}
    for _ in range(iters):
        tr.rollout()
        out["info"].append(tr.kernel_info()["rollout_step"])
        w = {"bins": tr.buffer(BUF_BINS), "items": tr.buffer(BUF_ITEMS),
             "action": tr.buffer(BUF_ACTION), "pold": tr.buffer(BUF_POLD),
             "done": tr.buffer(BUF_DONE), "rng": tr.buffer(BUF_RNG)}
        if record:
            w["logits"] = tr.buffer(BUF_LOGITS)
            w["probs"] = tr.buffer(BUF_PROBS)
        if algo == "klppo":
            w["qold"] = tr.buffer(BUF_QOLD)
        out["windows"].append(w)
        tr.learn()
    out["env_state"] = tr.env_state()
    out["rng"] = tr.buffer(BUF_RNG)
    out["pp"], out["vp"] = tr.params(POLICY), tr.params(VALUE)
    out["digest"] = tr.state_digest()
    tr.close()
    _runs[key] = out
    return out


def _same(a, b):
    assert len(a["windows"]) == len(b["windows"])
    for i, (wa, wb) in enumerate(zip(a["windows"], b["windows"])):
        assert wa.keys() == wb.keys()
        for k in wa:
            np.testing.assert_array_equal(wa[k], wb[k], err_msg="window %d %s" % (i, k))
            if wa[k].dtype.kind == "f":  # the bits, not only the values
                np.testing.assert_array_equal(wa[k].view(np.uint32), wb[k].view(np.uint32),
                                              err_msg="window %d %s bits" % (i, k))
    for x, y in zip(a["env_state"], b["env_state"]):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a["rng"], b["rng"])
    np.testing.assert_array_equal(a["pp"].view(np.uint32), b["pp"].view(np.uint32))
    np.testing.assert_array_equal(a["vp"].view(np.uint32), b["vp"].view(np.uint32))
    assert a["digest"] == b["digest"]


def _dones(run):
    return [int(w["done"].sum()) for w in run["windows"]]


def _pair(ctx, monkeypatch, packed=True, what="", **kw):
    """The default path against XH_ROLLOUT_TABLE=1; packed: the default is
    expected to run the packed kernel (else both run the same kernel)."""
    new = _run(ctx, monkeypatch, None, **kw)
    old = _run(ctx, monkeypatch, 1, **kw)
    for k in new["info"]:
        assert k["kernel"] == KERNEL or not packed
        assert (k["logit_table"] and k["envs_per_wave"] in PACKED) == packed, k
    for k in old["info"]:
        assert k["envs_per_wave"] <= 1, k
        assert k["logit_table"] == packed, k
    _same(new, old)
    nd = _dones(new)
    print("rollout pack %s %s: resets per window %s" % (what, kw, nd))
    return new, nd


@pytest.mark.parametrize("T,iters", [(4, 8), (9, 4)])
def test_ppo(ctx, monkeypatch, T, iters):
    """The headline window and one longer than 8 steps; every window after the
    first starts from slot T (src_slot), and every window holds resets."""
    _, nd = _pair(ctx, monkeypatch, what="ppo", algo="ppo", N=48, T=T, iters=iters)
    assert min(nd) > 0, nd


# tail waves: below, at and above one wave's envs for every packed layout, and
# a count that is a multiple of none with workgroups owning several waves
@pytest.mark.parametrize("N,iters", [(1, 8), (3, 4), (5, 4), (7, 4), (9, 4), (15, 4), (17, 4),
                                     (300, 2)])
def test_tail_waves(ctx, monkeypatch, N, iters):
    new, nd = _pair(ctx, monkeypatch, what="tail", algo="ppo", N=N, T=4, iters=iters)
    G = new["info"][0]["envs_per_wave"]
    assert {G - 1, G + 1} <= {1, 3, 5, 7, 9, 15, 17}
    assert sum(nd) > 0, nd


def _near_full(n, seed):
    """Slot-0 states with 0 .. 3 left in every bin dimension under item (4, 2):
    most actions end the episode."""
    rng = np.random.RandomState(seed)
    return {e: (rng.randint(0, 4, (B, D)).astype(np.int8), np.array([4, 2], np.int8))
            for e in range(n)}


def test_forced_actions(ctx, monkeypatch):
    """Teacher forcing on four bins, from nearly full bins: every window holds
    overflows."""
    forced = np.random.RandomState(11).randint(0, 4, (4, 10)).astype(np.int32)
    new, nd = _pair(ctx, monkeypatch, what="forced", N=10, T=4, iters=3, forced=forced,
                    states=_near_full(10, 6))
    for w in new["windows"]:
        np.testing.assert_array_equal(w["action"], forced)
    assert min(nd) > 0, nd


def test_klppo_with_distributions(ctx, monkeypatch):
    new, nd = _pair(ctx, monkeypatch, what="klppo", algo="klppo", N=48, T=4, iters=3)
    q = new["windows"][0]["qold"]
    assert q.shape == (4, 48, B)
    np.testing.assert_allclose(q.sum(-1), 1.0, atol=1e-5)
    assert min(nd) > 0, nd


def test_record_last_step(ctx, monkeypatch):
    new, nd = _pair(ctx, monkeypatch, what="record", N=48, T=4, iters=3, record=True)
    w = new["windows"][-1]
    assert np.isfinite(w["logits"]).all()
    np.testing.assert_allclose(w["probs"].sum(-1), 1.0, atol=1e-5)
    assert min(nd) > 0, nd


def test_actor_critic(ctx, monkeypatch):
    _, nd = _pair(ctx, monkeypatch, what="ac", algo="ac", N=48, T=4, iters=3)
    assert min(nd) > 0, nd


def test_wide_slot_keeps_forward(ctx, monkeypatch):
    """A slot 0 set with a bin below -capacity: the trainer runs the per-row
    forward from then on, whatever XH_ROLLOUT_TABLE says."""
    st = _near_full(10, 5)
    st[3][0][17, 1] = -CAP - 1
    new, nd = _pair(ctx, monkeypatch, packed=False, what="wide", N=10, T=4, iters=2, states=st)
    assert new["info"][1]["kernel"] == KERNEL and not new["info"][1]["logit_table"]
    assert sum(nd) > 0, nd


def test_kernel_info(ctx, monkeypatch):
    new = _run(ctx, monkeypatch, None, N=48, T=4, iters=8)
    one = _run(ctx, monkeypatch, 1, N=48, T=4, iters=8)
    fwd = _run(ctx, monkeypatch, 0, N=48, T=4, iters=2)
    for k in new["info"]:
        assert k["kernel"] == KERNEL and k["logit_table"] and k["envs_per_wave"] in PACKED
    for k in one["info"]:
        assert k["kernel"] == KERNEL and k["logit_table"] and k["envs_per_wave"] == 1
    for k in fwd["info"]:
        assert k["kernel"] == KERNEL and not k["logit_table"] and k["envs_per_wave"] == 1
