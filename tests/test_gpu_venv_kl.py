"""GPU tests of the KL-PPO side of the VecEnv chain: the distribution record
xh_venv_act writes (xh_venv_set_record_distrib), XH_LOSS_KL_REGULATED and
kl_stats of xh_venv_policy_loss, and xh_venv_kl_beta -- against
tests/venv_kl_ref.py (pinned on the CPU by tests/test_venv_kl_ref.py) and the
library's own oracle-pinned xh_action_loss_grad.

Shapes: tests/venv_loss_ref.py's -- 8 bins (one lane per row), 32 bins with N
= 70, 64 bins with N = 40 (partial waves), 128 bins with N = 5 (eight lanes
per row), 16 bins -- with T = 4 steps, and 600 rows of 8 bins (more than one
workgroup's 256 rows: several block partials)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import venv_kl_ref as kr
import venv_loss_ref as vr
from test_gpu_venv_loss import Dev, _bits, _rpw, _venv

pytestmark = pytest.mark.gpu

f32 = np.float32
CASES = vr.CASES
IDS = ["B%d-D%d-N%d" % c for c in CASES]
SETS = [(c, None) for c in CASES] + [(CASES[0], 600)]
SET_IDS = ["B%d-n%s" % (c[0], n or vr.T * c[2]) for c, n in SETS]
BETA = 0.05


@functools.lru_cache(maxsize=None)
def _inputs(sel):
    """A shape's inputs (clipped_inputs + the sampling distributions q),
    computed once and left unchanged."""
    inp = vr.clipped_inputs(*sel)
    inp["q"] = kr.kl_inputs(sel)
    for v in inp.values():
        v.setflags(write=False)
    return inp


def _policy_rows(g, kind, shape):
    if kind == "logits":
        return (g.standard_normal(shape) * 3.0).astype(f32)
    return (g.random(shape) * 5.0 + 1e-3).astype(f32)


def _args(dev, inp, policy, count, B, kind, loss, **over):
    """An xh_venv_loss on device copies of a shape's inputs, with its
    distributions; grad prefilled with -77.5 in a block of its own."""
    _lib = dev.lib
    a = _lib.VenvLoss()
    a.policy = dev.put(np.ascontiguousarray(policy, f32))
    a.kind = {"probs": _lib.ACT_PROBS, "logits": _lib.ACT_LOGITS}[kind]
    a.loss = {"log": _lib.LOSS_SOFTMAX_GRADIENT_LOG,
              "clipped": _lib.LOSS_CLIPPED, "kl": _lib.LOSS_KL_REGULATED}[loss]
    a.first, a.count, a.total = 0, count, len(inp["ch"])
    a.adv, a.action = dev.put(inp["adv"]), dev.put(inp["ch"])
    a.p_old = dev.put(inp["p_old"])
    a.distrib = dev.put(inp["q"])
    a.eps, a.scale, a.value_scale, a.beta = vr.EPS, 1.0, 1.0, BETA
    a.grad = dev.put(np.full((max(count, 1), B), -77.5, f32))
    for k, v in over.items():
        setattr(a, k, v)
    return a


# --------------------------------------------------------------------- 1 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_record(ctx, case, kind):
    """distrib[t][e] is the p[] the pick was made from: its entry at the
    action has PCHOICE's bits, logits rows are the loss head's probs_out of the
    same logits bit for bit, probs rows are the input bits, a refused env (a
    NaN entry) has a zero row, argmax records too; the accessors give 0 / NULL
    while the block is off and set_record_distrib returns its status codes."""
    from dependence_free_rl_amd import XhError, _lib
    B, D, N = case
    T, lib = vr.T, _lib.lib
    g = np.random.default_rng(B + N)
    rows = _policy_rows(g, kind, (T, N, B))
    rows[1, 3, B - 2] = np.nan
    env = _venv(ctx, case)
    # off: nothing to see, and no record to attach the block to
    assert lib.xh_venv_record_distrib_bytes(env.h) == 0
    assert lib.xh_venv_record_distrib_ptr(env.h) is None
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_ERR_STATE
    assert lib.xh_venv_set_record_distrib(env.h, 0) == _lib.XH_OK
    env.set_record(T, states=False)
    assert "distrib" not in env.record()
    env.act(np.abs(rows[0]) + f32(0.5), kind=kind, fetch=False)
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_ERR_STATE
    assert lib.xh_venv_record_distrib_bytes(env.h) == 0
    env.rewind()
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_OK
    assert lib.xh_venv_record_distrib_bytes(env.h) == T * N * B * 4
    assert lib.xh_venv_record_distrib_ptr(env.h)
    buf = np.zeros(T * N * B + 1, f32)
    assert lib.xh_venv_get_record_distrib(env.h, buf.ctypes.data,
                                          buf.nbytes) == _lib.XH_ERR_INVALID
    env.set_record(T, states=False)          # a new record drops the block
    assert lib.xh_venv_record_distrib_bytes(env.h) == 0
    assert lib.xh_venv_get_record_distrib(env.h, buf.ctypes.data,
                                          buf.nbytes - 4) == _lib.XH_ERR_INVALID
    env.set_record(T, states=False, distrib=True)
    assert env.record()["distrib"].shape == (0, N, B)

    for t in range(T):
        env.act(rows[t], kind=kind, fetch=False)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()  # the refused env
    rec = env.record()
    dist = rec["distrib"]
    assert dist.shape == (T, N, B) and dist.dtype == f32
    tt, ee = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    _bits(dist[tt, ee, rec["action"]], rec["pchoice"], "distrib[action]")
    assert rec["pchoice"][1, 3] == 0.0 and not dist[1, 3].any()
    keep = np.ones(T * N, bool)
    keep[N + 3] = False
    flat = dist.reshape(T * N, B)
    if kind == "logits":
        adv = np.ones(T * N, f32)
        probs = env.policy_loss(rows.reshape(T * N, B), adv, kind="logits",
                                loss="log", want_probs=True)["probs"]
        _bits(flat[keep], probs[keep], "the loss head's softmax")
        assert np.all(np.abs(flat[keep].sum(axis=1) - 1) < 1e-5)
    else:
        _bits(flat[keep], rows.reshape(T * N, B)[keep], "the input rows")
    # rewind keeps the block; argmax records the same p
    env.rewind()
    assert lib.xh_venv_record_distrib_bytes(env.h) == T * N * B * 4
    env.act(rows[0], kind=kind, mode="argmax", fetch=False)
    rec2 = env.record()
    assert rec2["distrib"].shape == (1, N, B)
    _bits(rec2["distrib"][0], dist[0], "argmax records p")
    _bits(rec2["distrib"][0, np.arange(N), rec2["action"][0]],
          rec2["pchoice"][0], "argmax: distrib[action]")
    np.testing.assert_array_equal(rec2["action"][0], rows[0].argmax(axis=1))
    assert lib.xh_venv_set_record_distrib(env.h, 0) == _lib.XH_OK
    assert lib.xh_venv_record_distrib_bytes(env.h) == 0
    assert lib.xh_venv_record_distrib_ptr(env.h) is None
    assert sorted(env.record()) == ["action", "done", "pchoice", "reward"]
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 2 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_recording_changes_nothing_else(ctx, case, kind):
    """Two venvs with the same seed and policy rows, one recording the
    distributions: the same actions, pchoice, reward, done, bins, items and
    stream states after T steps, and the same six record arrays."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    rows = _policy_rows(np.random.default_rng(B * N), kind, (vr.T, N, B))
    out = []
    for distrib in (False, True):
        env = _venv(ctx, case)
        env.set_record(vr.T, states=True, distrib=distrib)
        for t in range(vr.T):
            env.act(rows[t], kind=kind, fetch=False)
        env.synchronize()
        rec = env.record()
        assert ("distrib" in rec) == distrib
        out.append([env.get(w) for w in (
            _lib.VENV_ACTIONS, _lib.VENV_PCHOICE, _lib.VENV_REWARD,
            _lib.VENV_DONE, _lib.VENV_BINS, _lib.VENV_ITEMS, _lib.VENV_RNG)] +
            [rec[k] for k in ("action", "pchoice", "reward", "done", "bins",
                              "items")])
        env.close()
    for x, y in zip(*out):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    assert out[0][3].shape == (N,) and len(out[0]) == 13


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_probs_parity_with_action_loss_grad(ctx, sel):
    """XH_ACT_PROBS with the caller's distrib at scale 1: grad is
    xh_action_loss_grad(XH_LOSS_KL_REGULATED)'s output on the same rows bit
    for bit, and the restatement's; also through a permuted index list, and
    for runs of 1, 64 / LPE - 1 and 64 / LPE + 1 rows from first > 0."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    probs, ch, adv, q = inp["probs"], inp["ch"], inp["adv"], inp["q"]
    want = np.zeros((n, B), f32)
    _lib.check(_lib.lib.xh_action_loss_grad(
        ctx.h, _lib.LOSS_KL_REGULATED, n, B, ch.ctypes.data, q.ctypes.data,
        adv.ctypes.data, probs.ctypes.data, BETA, want.ctypes.data))
    assert np.count_nonzero(want) >= n
    _bits(want, kr.kl_grad_f32(probs, q, ch, inp["p_old"], adv, BETA),
          "the restatement")
    env = _venv(ctx, case)
    kw = dict(kind="probs", loss="kl", action=ch, p_old=inp["p_old"],
              distrib=q, beta=BETA)
    _bits(env.policy_loss(probs, adv, **kw)["grad"], want, "all rows")
    rows = np.random.default_rng(n).permutation(n).astype(np.int32)
    _bits(env.policy_loss(probs[rows], adv, rows=rows, **kw)["grad"],
          want[rows], "index list")
    for count in (1, _rpw(B) - 1, _rpw(B) + 1):
        if count < 1 or 3 + count > n:
            continue
        got = env.policy_loss(probs[3:3 + count], adv, first=3, count=count,
                              **kw)["grad"]
        _bits(got, want[3:3 + count], "count %d" % count)
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 4 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_logits_gradient_bits(ctx, sel):
    """grad for logits is the restatement applied to the kernel's own
    probs_out, bit for bit, at scale 1 and at 1 / count, with beta by value
    and through beta_dev (the same bits), and in place (grad == policy)."""
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    env = _venv(ctx, case)
    dev = Dev(ctx)
    beta_dev = dev.put(np.array([BETA], f32))
    kw = dict(kind="logits", loss="kl", action=inp["ch"], p_old=inp["p_old"],
              distrib=inp["q"], want_probs=True)
    first = None
    for scale in (1.0, 1.0 / n):
        got = env.policy_loss(inp["z"], inp["adv"], scale=scale, beta=BETA,
                              **kw)
        want = kr.kl_grad_f32(got["probs"], inp["q"], inp["ch"], inp["p_old"],
                              inp["adv"], BETA, f32(scale))
        _bits(got["grad"], want, "scale %g" % scale)
        assert np.count_nonzero(got["grad"]) == n * B
        by_ptr = env.policy_loss(inp["z"], inp["adv"], scale=scale,
                                 beta=beta_dev, **kw)
        _bits(by_ptr["grad"], got["grad"], "beta_dev, scale %g" % scale)
        first = first if first is not None else got["grad"]
    # the regulation is there: beta 0 gives another gradient
    zero = env.policy_loss(inp["z"], inp["adv"], beta=0.0, **kw)["grad"]
    assert np.count_nonzero(zero != first) > n
    a = _args(dev, inp, inp["z"], n, B, "logits", "kl")
    a.grad = a.policy
    dev.lib.check(dev.lib.lib.xh_venv_policy_loss(env.h, C.byref(a)))
    env.synchronize()
    _bits(dev.get(a.policy, f32, (n, B)), first, "in place")
    dev.free()
    env.close()


# --------------------------------------------------------------------- 5 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_epoch_zero(ctx, case, kind):
    """The recorded policy rows fed back with the record's own distributions
    (distrib=None): p == q bit for bit, so KL_SUM and KL_SQSUM are exactly
    0.0, ROWS is T N, and the gradient is the "log" loss's bit for bit
    whatever beta is."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    g = np.random.default_rng(B + N)
    rows = _policy_rows(g, kind, (vr.T, N, B))
    env = _venv(ctx, case)
    env.set_record(vr.T, states=False, distrib=True)
    for t in range(vr.T):
        env.act(rows[t], kind=kind, fetch=False)
    rec = env.record()
    n = vr.T * N
    adv = (g.choice([-1.0, 1.0], n) * g.uniform(0.25, 2.0, n)).astype(f32)
    z = rows.reshape(n, B)
    log = env.policy_loss(z, adv, kind=kind, loss="log")["grad"]
    assert np.count_nonzero(log) == n * B
    for beta in (0.0, 0.1, 1.0, 37.5):
        got = env.policy_loss(z, adv, kind=kind, loss="kl", beta=beta,
                              want_probs=True, want_kl=True)
        _bits(got["probs"], rec["distrib"].reshape(n, B), "p == q")
        st = got["kl_stats"]
        assert st.shape == (_lib.VKL_COUNT,)
        assert st[_lib.VKL_KL_SUM] == 0.0 and st[_lib.VKL_KL_SQSUM] == 0.0
        assert st[_lib.VKL_ROWS] == n
        _bits(got["grad"], log, "beta %g" % beta)
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 6 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_kl_statistics(ctx, sel):
    """KL_SUM within 1e-12 of the sum of its terms' magnitudes of the float64
    restatement on the kernel's own probs_out (the bound of the cancelling
    double sums in test_gpu_venv_loss.py::test_statistics), KL_SQSUM within
    1e-12 relative, ROWS exact; two runs give the same bits; three uneven
    minibatches with accumulate equal the three calls' rows added in call
    order bit for bit; skipped rows count nowhere; kl_stats under the clipped
    loss gives the same numbers and leaves grad and stats at their bits."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    inp = _inputs(sel)
    n = len(inp["ch"])
    q = inp["q"]
    assert (q == 0).sum() >= n // 5
    p_old = inp["p_old"].copy()
    p_old[[2, n // 2]] = [0.0, np.nan]     # two skipped rows
    env = _venv(ctx, case)
    kw = dict(kind="logits", action=inp["ch"], p_old=p_old, distrib=q,
              eps=vr.EPS, want_probs=True, want_kl=True)
    runs = [env.policy_loss(inp["z"], inp["adv"], loss="kl", beta=BETA, **kw)
            for _ in range(2)]
    got = runs[0]
    st = got["kl_stats"]
    assert st.tobytes() == runs[1]["kl_stats"].tobytes()
    want, mag = kr.kl_stats_f64(got["probs"], q, p_old)
    print("kl_stats: got %r want %r, sum |terms| %.6g" % (st, want, mag))
    print("  |KL_SUM - want| = %.3g (bound %.3g); KL_SQSUM rel %.3g" % (
        abs(st[_lib.VKL_KL_SUM] - want[kr.KL_SUM]), 1e-12 * mag,
        abs(st[_lib.VKL_KL_SQSUM] / want[kr.KL_SQSUM] - 1)))
    assert np.isfinite(st).all() and want[kr.KL_SUM] > 0
    assert st[_lib.VKL_ROWS] == want[kr.ROWS] == n - 2
    assert abs(st[_lib.VKL_KL_SUM] - want[kr.KL_SUM]) <= 1e-12 * mag
    assert abs(st[_lib.VKL_KL_SQSUM] - want[kr.KL_SQSUM]) <= \
        1e-12 * want[kr.KL_SQSUM]
    assert not got["grad"][2].any() and not got["grad"][n // 2].any()
    # three uneven minibatches
    cuts = [0, n // 5, n // 5 + n // 2 + 1, n]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        parts.append(env.policy_loss(inp["z"][lo:hi], inp["adv"], loss="kl",
                                     beta=BETA, first=lo, count=hi - lo,
                                     **kw)["kl_stats"])
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        acc = env.policy_loss(inp["z"][lo:hi], inp["adv"], loss="kl",
                              beta=BETA, first=lo, count=hi - lo,
                              accumulate=i > 0, **kw)["kl_stats"]
    chain = (parts[0] + parts[1]) + parts[2]
    assert acc.tobytes() == chain.tobytes()
    assert acc[_lib.VKL_ROWS] == n - 2
    # under the clipped loss: the same numbers, grad and stats untouched by it
    plain = env.policy_loss(inp["z"], inp["adv"], loss="clipped",
                            action=inp["ch"], p_old=p_old, eps=vr.EPS,
                            want_stats=True)
    both = env.policy_loss(inp["z"], inp["adv"], loss="clipped",
                           want_stats=True, **kw)
    assert both["kl_stats"].tobytes() == st.tobytes()
    _bits(both["grad"], plain["grad"], "clipped grad with kl_stats")
    assert both["stats"].tobytes() == plain["stats"].tobytes()
    assert both["stats"][_lib.VLOSS_SKIPPED] == 2
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 7 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_beta_rule(ctx, case):
    """xh_venv_kl_beta on the device's kl_stats: {beta before, d, beta after}
    are the f32 restatement's bits for a d_targ that halves, one that doubles,
    one in the dead band, both clamps and ROWS == 0; and in a two-epoch loop
    through beta_dev the second epoch's gradient uses the updated value."""
    from dependence_free_rl_amd import _lib
    B = case[0]
    lib = _lib.lib
    inp = _inputs((case, None))
    n = len(inp["ch"])
    env = _venv(ctx, case)
    dev = Dev(ctx)
    a = _args(dev, inp, inp["z"], n, B, "logits", "kl")
    a.kl_stats = dev.put(np.zeros(_lib.VKL_COUNT))
    a.beta_dev = dev.put(np.array([0.04], f32))
    a.probs_out = dev.put(np.zeros((n, B), f32))
    _lib.check(lib.xh_venv_policy_loss(env.h, C.byref(a)))
    env.synchronize()
    st = dev.get(a.kl_stats, np.float64, (_lib.VKL_COUNT,))
    probs = dev.get(a.probs_out, f32, (n, B))
    d = st[_lib.VKL_KL_SUM] / st[_lib.VKL_ROWS]
    assert st[_lib.VKL_ROWS] == n and 1e-4 < d < 10
    log = dev.put(np.zeros(3, f32))
    empty = dev.put(np.zeros(_lib.VKL_COUNT))
    seen = set()
    for stats, d_targ, beta in (
            (a.kl_stats, 10 * d, 0.04),      # halves
            (a.kl_stats, d / 10, 0.04),      # doubles
            (a.kl_stats, d, 0.04),           # the dead band
            (a.kl_stats, d / 10, 0.08),      # doubles into the upper clamp
            (a.kl_stats, 10 * d, 1e-25),     # halves into the lower clamp
            (a.kl_stats, d, 1.0),            # dead band, clamped from above
            (empty, d, 0.04),                # ROWS == 0: d is NaN
            (empty, d, 0.0)):                # ... and only the clamp acts
        b = dev.put(np.array([beta], f32))
        _lib.check(lib.xh_venv_kl_beta(env.h, stats, d_targ, b, log))
        got = dev.get(log, f32, (3,))
        s = st if stats == a.kl_stats else np.zeros(3)
        want = kr.beta_rule_f32(s[_lib.VKL_KL_SUM], s[_lib.VKL_ROWS], d_targ,
                                beta)
        want = np.array(want, f32)
        num = ~np.isnan(want)  # a NaN d is a NaN here; its sign is not pinned
        assert got[num].tobytes() == want[num].tobytes(), (got, want)
        assert np.isnan(got[~num]).all(), (got, want)
        assert dev.get(b, f32, (1,))[0] == got[2]
        seen.add((float(got[2]) > float(got[0])) - (float(got[2]) <
                                                    float(got[0])))
        if stats == empty:
            assert math.isnan(got[1])
    assert seen == {-1, 0, 1}
    # the Python call, from a host row and a float
    after, mean = env.kl_beta(st, d / 10, 0.04)
    assert after == f32(0.08) and f32(mean) == f32(d)

    # two epochs through beta_dev: the gradient uses the beta before the
    # update, the next epoch's the updated one
    want0 = kr.kl_grad_f32(probs, inp["q"], inp["ch"], inp["p_old"],
                           inp["adv"], 0.04)
    _bits(dev.get(a.grad, f32, (n, B)), want0, "epoch 1")
    _lib.check(lib.xh_venv_kl_beta(env.h, a.kl_stats, d / 10, a.beta_dev,
                                   None))
    _lib.check(lib.xh_venv_policy_loss(env.h, C.byref(a)))
    env.synchronize()
    assert dev.get(a.beta_dev, f32, (1,))[0] == f32(0.08)
    want1 = kr.kl_grad_f32(probs, inp["q"], inp["ch"], inp["p_old"],
                           inp["adv"], 0.08)
    _bits(dev.get(a.grad, f32, (n, B)), want1, "epoch 2")
    assert np.count_nonzero(want1 != want0) > n
    dev.free()
    env.close()


# --------------------------------------------------------------------- 8 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_refusals_and_side_effects(ctx, case):
    """Each XH_ERR_INVALID case launches nothing (the outputs keep their
    fill); after loss and beta calls of every form the venv's state, record
    and cursor are what they were."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    g = np.random.default_rng(N)
    rows = (g.standard_normal((vr.T, N, B)) * 2.0).astype(f32)
    env = _venv(ctx, case)
    env.set_record(vr.T + 1, distrib=True)
    for t in range(vr.T):
        env.act(rows[t], kind="logits", fetch=False)

    def state():
        rec = env.record()
        return ([env.get(w) for w in (_lib.VENV_BINS, _lib.VENV_ITEMS,
                                      _lib.VENV_RNG, _lib.VENV_ACTIONS,
                                      _lib.VENV_PCHOICE, _lib.VENV_REWARD,
                                      _lib.VENV_DONE)] +
                [rec[k] for k in sorted(rec)] + [np.array(env.record_pos())])

    before = state()
    assert len(before) == 7 + 7 + 1
    n = vr.T * N
    inp = {k: v[:n] for k, v in _inputs((case, None)).items()}
    assert len(inp["ch"]) == n
    dev = Dev(ctx)
    count = 9
    z = inp["z"][:count]
    fill = np.full((count, B), -77.5, f32)

    def refused(code=INV, **over):
        b = _args(dev, inp, z, count, B, "logits", "kl")
        b.probs_out = dev.put(fill)
        b.kl_stats = dev.put(np.full(_lib.VKL_COUNT, -3.0))
        grad, probs, kls = b.grad, b.probs_out, b.kl_stats
        for k, v in over.items():
            setattr(b, k, v(b) if callable(v) else v)
        assert lib.xh_venv_policy_loss(env.h, C.byref(b)) == code, over
        _bits(dev.get(grad, f32, (count, B)), fill, str(over))
        _bits(dev.get(probs, f32, (count, B)), fill, str(over))
        assert (dev.get(kls, np.float64, (_lib.VKL_COUNT,)) == -3.0).all()

    other = _venv(ctx, case)     # a venv without recorded distributions
    for loss, kls in (("kl", None), ("clipped", "keep"), ("kl", "keep")):
        b = _args(dev, inp, z, count, B, "logits", loss, distrib=None)
        if kls:
            b.kl_stats = dev.put(np.zeros(_lib.VKL_COUNT))
        assert lib.xh_venv_policy_loss(other.h, C.byref(b)) == INV, loss
        assert b"distrib" in lib.xh_last_error()
        _bits(dev.get(b.grad, f32, (count, B)), fill, loss)
    other.close()
    for beta in (float("nan"), float("inf"), -1e-3):
        refused(beta=beta)
    refused(distrib=lambda b: b.distrib + 4)            # misaligned
    refused(distrib=lambda b: b.grad)                   # over grad
    refused(distrib=lambda b: b.grad + 16)
    refused(distrib=lambda b: b.probs_out - 16 * B)     # reaches probs_out
    refused(loss=_lib.LOSS_GRADIENT_LOG)
    refused(total=n + 1, distrib=None)   # more rows than the record holds
    # a bad beta is not read through beta_dev, nor under another loss
    ok = _args(dev, inp, z, count, B, "logits", "kl", beta=float("nan"),
               beta_dev=dev.put(np.array([BETA], f32)))
    assert lib.xh_venv_policy_loss(env.h, C.byref(ok)) == _lib.XH_OK
    ok = _args(dev, inp, z, count, B, "logits", "clipped", beta=-1.0)
    assert lib.xh_venv_policy_loss(env.h, C.byref(ok)) == _lib.XH_OK
    # xh_venv_kl_beta
    st = dev.put(np.array([1.0, 2.0, 1.0]))
    beta = dev.put(np.array([0.04], f32))
    assert lib.xh_venv_kl_beta(env.h, None, 0.01, beta, None) == INV
    assert lib.xh_venv_kl_beta(env.h, st, 0.01, None, None) == INV
    for d_targ in (0.0, -0.01, float("nan"), float("inf")):
        assert lib.xh_venv_kl_beta(env.h, st, d_targ, beta, None) == INV
    env.synchronize()
    assert dev.get(beta, f32, (1,))[0] == f32(0.04)

    # calls of every form: nothing of the venv's moves
    adv = inp["adv"]
    zz = rows.reshape(n, B)
    env.policy_loss(zz, adv, loss="kl", beta=BETA, want_probs=True,
                    want_kl=True, want_stats=True)
    perm = g.permutation(n)[:N + 3].astype(np.int32)
    env.policy_loss(zz[perm], adv, loss="kl", rows=perm, beta=beta,
                    want_kl=True, accumulate=True)
    env.policy_loss(zz, adv, loss="clipped", want_kl=True)
    env.policy_loss(np.abs(zz) + f32(0.01), adv, kind="probs", loss="kl",
                    distrib=inp["q"], beta=0.5, scale=1.0 / n)
    env.kl_beta(env._dev["vl_kl"][0], 0.01, beta)
    env.kl_beta(np.array([1.0, 4.0, 1.0]), 0.01, 0.04)
    env.synchronize()
    after = state()
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    env.act(rows[0], kind="logits", fetch=False)
    assert env.record_pos() == vr.T + 1
    assert env.record()["distrib"].shape == (vr.T + 1, N, B)
    env.synchronize()
    dev.free()
    env.close()
