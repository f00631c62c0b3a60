"""The compaction pass's duplicate search on LDS lane masks
(dependence_free_rl_amd/csrc/spec8_pack_kernels.hip: pack_classify_mask_kernel,
pack_write_mask_kernel; spec8_pack_layout.h; DESIGN.md §3.0e, "the duplicate
search") against the former kernels (XH_SP8_PACK_DEDUP=loop) and against a
numpy restatement of the layout.

Two trainers of one seed run rollout + learn(), one per kernel set: the packed
batch (Trainer.pack_buffer(): header and every record byte), every epoch's
policy gradient and both nets' parameters are equal bit for bit, PPO and
actor-critic.  Shapes: N = 1, T = 1; N = 7, T = 3 (21 env-steps: a partly
filled chunk, both items, a partly filled last group); N = 48, T = 4;
N = 300, T = 4 (19 chunks: the scan's offsets cross workgroups); N = 48,
T = 9.  The hand-set states of test_gpu_spec8_pack.py's fallback case (64,
exactly 16 and exactly 17 distinct legal states, negatives among them, and
fresh envs: packed and wide classes of both items in one batch), and a batch
with a bin at -9 and one at -128 (no word in the table: those env-steps take
the loop inside the new kernels).  The restatement builds the expected header
and records from BUF_BINS / BUF_ITEMS / BUF_ACTION / BUF_POLD / BUF_ADV:
first-occurrence order, counts, cu, the class order, the empty tail segments.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, D, WIDTHS = 64, 2, (128, 128)
X0 = 4711
ITEM_A = (4, 2)  # the 2-D environment's item_a (xh_host.h: make_env)
SEG_ROWS, SEGS, GROUP = 16, 4, 256
STATES, COUNTS, SEG_RECS = 0, 128, 192

_runs = {}


def _params():
    from dependence_free_rl_amd import init_policy, init_value
    return init_policy(D, *WIDTHS, seed=61), init_value(B, D, seed=62)


def _learn(ctx, monkeypatch, algo, N, T, dedup, states=None, iters=1, cache=True,
           flat_policy=False):
    """rollout + learn() `iters` times; the last learn()'s packed batch, its
    inputs and its results.  flat_policy: all policy parameters 0, every bin
    as likely as any other."""
    key = (algo, N, T, dedup, states is not None and id(states), iters, flat_policy)
    if cache and key in _runs:
        return _runs[key]
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_ADV, BUF_BINS, BUF_ITEMS,
                                                BUF_POLD, BUF_POLICY_GRADS)
    for k in ("XH_SP8_PACK", "XH_TRAIN_TABLE", "XH_TRAIN_KERNEL", "XH_E0_REUSE"):
        monkeypatch.delenv(k, raising=False)
    if dedup is None:
        monkeypatch.delenv("XH_SP8_PACK_DEDUP", raising=False)
    else:
        monkeypatch.setenv("XH_SP8_PACK_DEDUP", dedup)
    pp, vp = _params()
    if flat_policy:
        pp = np.zeros_like(pp)
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    if states:
        _, items = tr.env_state()
        for e, st in states.items():
            tr.set_env_state(e, st[None], items[e:e + 1])
    for _ in range(iters):
        tr.rollout()
        tr.learn()
    hdr, rec = tr.pack_buffer()
    out = {"hdr": hdr, "rec": rec, "stats": tr.pack_stats(),
           "bins": tr.buffer(BUF_BINS)[:T].copy(), "items": tr.buffer(BUF_ITEMS)[:T].copy(),
           "action": tr.buffer(BUF_ACTION).copy(), "pold": tr.buffer(BUF_POLD).copy(),
           "adv": tr.buffer(BUF_ADV).copy(),
           "grads": tr.buffer(BUF_POLICY_GRADS).copy(),
           "policy": tr.params(POLICY).copy(), "value": tr.params(VALUE).copy()}
    tr.close()
    if cache:
        _runs[key] = out
    return out


def _expected(run):
    """spec8_pack_layout.h, restated: (header, records) of the batch."""
    T, N = run["action"].shape
    nt = T * N
    bins = run["bins"].reshape(nt, B, D)
    items = run["items"].reshape(nt, 4)
    action, pold, adv = (run[k].reshape(nt) for k in ("action", "pold", "adv"))
    steps = []   # per env-step: its states in first-occurrence order, counts, slots
    cls = [[], [], [], []]  # packed a, packed b, wide a, wide b: env-steps in batch order
    for e in range(nt):
        order, count, slot = [], {}, np.zeros(B, np.int64)
        for lane in range(B):
            s = (int(bins[e, lane, 0]), int(bins[e, lane, 1]))
            if s not in count:
                count[s] = 0
                order.append(s)
            count[s] += 1
            slot[lane] = order.index(s)
        steps.append((order, [count[s] for s in order], slot))
        is_a = (int(items[e, 0]), int(items[e, 1])) == ITEM_A
        cls[(2 if len(order) > SEG_ROWS else 0) + (0 if is_a else 1)].append(e)
    na, nb, ua, ub = (len(c) for c in cls)
    ga, gb = -(-na // SEGS), -(-nb // SEGS)
    groups = ga + gb + ua + ub
    hdr = np.array([na, nb, ua, ub, ga, gb, groups, 0], np.int32)
    # a record: 64 rows x (b0, b1) int8, 64 counts, 4 x PkSeg (cu, pold, adv, step)
    st = np.zeros((groups, SEGS * SEG_ROWS, 2), np.int8)
    cn = np.zeros((groups, SEGS * SEG_ROWS), np.uint8)
    seg = np.zeros((groups, SEGS, 4), np.int32)
    pold_bits, adv_bits = pold.view(np.int32), adv.view(np.int32)
    one = int(np.float32(1.0).view(np.int32))
    for k, base in ((0, 0), (1, ga)):
        for p, e in enumerate(cls[k]):
            g, q = base + p // SEGS, p % SEGS
            order, count, slot = steps[e]
            for i, s in enumerate(order):
                st[g, SEG_ROWS * q + i] = s
                cn[g, SEG_ROWS * q + i] = count[i]
            seg[g, q] = (SEG_ROWS * q + slot[action[e] & 63], pold_bits[e], adv_bits[e], e)
        if cls[k]:  # the empty segments behind the class's last env-step
            p = len(cls[k]) - 1
            for q in range(p % SEGS + 1, SEGS):
                seg[base + p // SEGS, q] = (-1, one, 0, -1)
    for k, base in ((2, ga + gb), (3, ga + gb + ua)):
        for p, e in enumerate(cls[k]):
            g = base + p
            st[g] = bins[e]
            cn[g] = 1
            seg[g, :] = (action[e], pold_bits[e], adv_bits[e], e)
    rec = np.concatenate([st.reshape(groups, -1).view(np.uint8), cn,
                          seg.reshape(groups, -1).view(np.uint8)], axis=1)
    assert rec.shape == (groups, GROUP)
    assert (STATES, COUNTS, SEG_RECS) == (0, st[0].size, st[0].size + cn[0].size)
    return hdr, rec, [len(s[0]) for s in steps]


def _same(a, b, what):
    np.testing.assert_array_equal(a["hdr"], b["hdr"], err_msg=what + ": header")
    assert a["rec"].shape == b["rec"].shape, what
    bad = np.nonzero((a["rec"] != b["rec"]).any(axis=1))[0]
    assert bad.size == 0, "%s: %d records differ, first %d:\n%s\n%s" % (
        what, bad.size, bad[0], a["rec"][bad[0]], b["rec"][bad[0]])
    for k in ("grads", "policy", "value"):
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s" % (what, k)


def _check(ctx, monkeypatch, algo, N, T, states=None, iters=1, flat_policy=False):
    new = _learn(ctx, monkeypatch, algo, N, T, None, states, iters, flat_policy=flat_policy)
    old = _learn(ctx, monkeypatch, algo, N, T, "loop", states, iters, flat_policy=flat_policy)
    what = "%s N=%d T=%d" % (algo, N, T)
    # the same batch went in
    for k in ("bins", "items", "action", "pold", "adv"):
        assert new[k].tobytes() == old[k].tobytes(), "%s: %s" % (what, k)
    _same(new, old, what + " masks against loop")
    hdr, rec, distinct = _expected(new)
    for run, name in ((new, "masks"), (old, "loop")):
        np.testing.assert_array_equal(run["hdr"], hdr, err_msg="%s %s: header" % (what, name))
        bad = np.nonzero((run["rec"] != rec).any(axis=1))[0]
        assert bad.size == 0, "%s %s: %d records differ from the layout, first %d:\n%s\n%s" % (
            what, name, bad.size, bad[0], run["rec"][bad[0]], rec[bad[0]])
    stats = new["stats"]
    assert stats["packed"] == hdr[0] + hdr[1] and stats["unpacked"] == hdr[2] + hdr[3]
    assert stats["groups"] == hdr[6] and stats["packed"] + stats["unpacked"] == N * T
    assert np.isfinite(new["grads"]).all() and np.isfinite(new["policy"]).all()
    print("pack dedup %s: header %s, distinct states per env-step %d .. %d" % (
        what, hdr.tolist(), min(distinct), max(distinct)))
    return new, hdr, np.array(distinct).reshape(T, N)


SHAPES = [(1, 1), (7, 3), (48, 4), (300, 4), (48, 9)]


@pytest.mark.parametrize("algo", ["ppo", "ac"])
@pytest.mark.parametrize("N,T", SHAPES)
def test_equal_to_loop_and_layout(ctx, monkeypatch, algo, N, T):
    _, hdr, _ = _check(ctx, monkeypatch, algo, N, T)
    assert hdr[2] == 0 and hdr[3] == 0  # the environment's states: all packed
    if (N, T) == (1, 1):
        # one segment, three empty ones behind it
        assert hdr[0] + hdr[1] == 1 and hdr[6] == 1, hdr
    if (N, T) == (7, 3):
        # both classes present, a last group partly filled (this seed: 9 + 12
        # env-steps; item_b's partly filled last group is N = 1's)
        assert hdr[0] > 0 and hdr[1] > 0 and (hdr[0] % 4 != 0 or hdr[1] % 4 != 0), hdr


# ---- hand-set states (test_gpu_spec8_pack.py's fallback case, restated)
FN, FT = 24, 2
LEGAL = [(a, b) for a in range(-8, 9) for b in range(-8, 9)]


def _mixed_states():
    """Envs 0-5: 64 distinct legal bin states, 6-11: exactly 16, 12-17:
    exactly 17 (negative values among all of them); 18-23 stay fresh."""
    rng = np.random.RandomState(2024)
    out = {}
    for e in range(18):
        d = (64, 16, 17)[e // 6]
        pick = rng.permutation(len(LEGAL))[:d]
        st = np.array([LEGAL[i] for i in pick], np.int8)
        if not (st < 0).any():
            st[0] = (-3, 5)
            assert len({tuple(x) for x in st}) == d
        rows = np.concatenate([np.arange(d), rng.randint(0, d, B - d)])
        out[e] = st[rng.permutation(rows)]
    return out


MIXED = _mixed_states()


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_mixed_batch(ctx, monkeypatch, algo):
    _, hdr, d = _check(ctx, monkeypatch, algo, FN, FT, states=MIXED)
    # slot 0 holds the states as set
    assert (d[0, :6] == 64).all() and (d[0, 6:12] == 16).all() and (d[0, 12:18] == 17).all()
    assert (d[0, 18:] == 1).all()
    # packed and wide env-steps of both items in one batch
    assert (hdr[:4] > 0).all(), hdr
    assert hdr[2] + hdr[3] == int((d > 16).sum())


def _outside_states():
    """The mixed batch's envs 0-17; envs 18-20 fresh but for one bin at -9,
    envs 21-23 fresh but for one bin at -128 (the lowest int8) in either or
    both dimensions: which of them the policy leaves alone for a window is
    its own affair, the test asks for one."""
    out = dict(MIXED)
    low = {21: (-128, 8), 22: (-128, -128), 23: (2, -128)}
    for e in range(18, 24):
        st = np.full((B, D), 8, np.int8)
        st[(5, 17, 63)[e % 3]] = low.get(e, (-9, 3))
        out[e] = st
    return out


OUTSIDE = _outside_states()


@pytest.mark.parametrize("algo", ["ppo", "ac"])
def test_states_outside_the_table(ctx, monkeypatch, algo):
    """A slot-0 bin below -8 keeps the first learn() off the packed path; the
    bin stays until an action takes it, so the second window's batch holds it
    and packs: those env-steps take the loop inside the new kernels.  The
    policy's parameters are all 0 (a uniform pick among the 64 bins): the
    seeded policy of the other cases takes a bin at -128 at once, which ends
    the episode, so no later window would hold one."""
    new, hdr, _ = _check(ctx, monkeypatch, algo, FN, FT, states=OUTSIDE, iters=2,
                         flat_policy=True)
    flat = new["bins"].reshape(-1, B, D)
    steps9 = int((flat == -9).any(axis=(1, 2)).sum())
    steps128 = int((flat == -128).any(axis=(1, 2)).sum())
    print("env-steps with a bin at -9: %d, at -128: %d" % (steps9, steps128))
    assert steps9 >= 1 and steps128 >= 1
    assert int((flat >= -8).all(axis=(1, 2)).sum()) >= 1  # and env-steps on the masks


def test_deterministic(ctx, monkeypatch):
    for shape, states in (((300, 4), None), ((FN, FT), MIXED)):
        a = _learn(ctx, monkeypatch, "ppo", *shape, None, states)
        b = _learn(ctx, monkeypatch, "ppo", *shape, None, states, cache=False)
        _same(a, b, "two runs N=%d T=%d" % shape)


def test_not_packed_is_an_error(ctx, monkeypatch):
    from dependence_free_rl_amd import POLICY, VALUE, Trainer
    monkeypatch.setenv("XH_SP8_PACK", "0")
    pp, vp = _params()
    tr = Trainer(ctx, algo="ppo", bins=B, dims=D, num_envs=4, steps=2, widths=WIDTHS,
                 rng_state=X0)
    tr.set_params(POLICY, pp)
    tr.set_params(VALUE, vp)
    tr.rollout()
    tr.learn()
    with pytest.raises(Exception):
        tr.pack_buffer()
    tr.close()
