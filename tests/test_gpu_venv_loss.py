"""GPU tests of xh_venv_policy_loss, the loss head of a caller's network on a
recorded window, against tests/venv_loss_ref.py (pinned on the CPU by
tests/test_venv_loss_ref.py) and the library's own oracle-pinned
xh_action_loss_grad.

Shapes: test_gpu_venv_learn.py's -- 8 bins (one lane per row), 32 bins with N
= 70, 64 bins with N = 40, 128 bins with N = 5 (eight lanes per row), 16 bins
-- with T = 4 steps, so T * N rows; 600 rows of 8 bins (more than one
workgroup's 256: several block partials) and 72 rows of 16 bins (more than
that shape's 64 rows per wave); and runs of 1, 64 / LPE - 1 and 64 / LPE + 1
rows (a partial wave, one row into the next wave) wherever the set has that
many rows."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import venv_loss_ref as vr

pytestmark = pytest.mark.gpu

f32 = np.float32
CASES = vr.CASES
IDS = ["B%d-D%d-N%d" % c for c in CASES]
SETS = [(c, None) for c in CASES] + [(CASES[0], 600), (CASES[4], 72)]
SET_IDS = ["B%d-n%s" % (c[0], n or vr.T * c[2]) for c, n in SETS]
X0 = 4242


@functools.lru_cache(maxsize=None)
def _inputs(sel):
    """A shape's clipped-loss inputs, computed once and left unchanged."""
    inp = vr.clipped_inputs(*sel)
    for v in inp.values():
        v.setflags(write=False)
    return inp


def _venv(ctx, case):
    from dependence_free_rl_amd import VecEnv
    B, D, N = case
    return VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=X0)


def _rpw(B):
    return 64 // max(B // 16, 1)


def _bits(got, want, what=""):
    got = np.ascontiguousarray(got, f32)
    want = np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32),
                                  err_msg=what)


class Dev:
    """Device blocks of the test's own (the caller's side of the pointers)."""

    def __init__(self, ctx):
        from dependence_free_rl_amd import _lib
        self.ctx, self.lib, self.ptrs = ctx, _lib, []

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.lib.check(self.lib.tensor_alloc(self.ctx.h, (nbytes + 3) // 4 + 4,
                                             C.byref(p)))
        self.ptrs.append(p.value)
        return p.value

    def put(self, a, ptr=None):
        a = np.ascontiguousarray(a)
        assert a.nbytes % 4 == 0
        ptr = ptr or self.alloc(a.nbytes)
        self.lib.check(self.lib.tensor_copy(self.ctx.h, ptr, a.ctypes.data,
                                            a.nbytes // 4, self.lib.COPY_H2D))
        return ptr

    def get(self, ptr, dtype, shape):
        out = np.zeros(shape, dtype)
        self.lib.check(self.lib.tensor_copy(self.ctx.h, out.ctypes.data, ptr,
                                            out.nbytes // 4,
                                            self.lib.COPY_D2H))
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.check(self.lib.tensor_free(self.ctx.h, p))
        self.ptrs = []


def _args(dev, inp, policy, count, B, kind, loss, fill=None, **over):
    """An xh_venv_loss on device copies of a shape's inputs; grad (prefilled
    with `fill`) in a block of its own."""
    _lib = dev.lib
    a = _lib.VenvLoss()
    a.policy = dev.put(np.ascontiguousarray(policy, f32))
    a.kind = {"probs": _lib.ACT_PROBS, "logits": _lib.ACT_LOGITS}[kind]
    a.loss = {"log": _lib.LOSS_SOFTMAX_GRADIENT_LOG,
              "clipped": _lib.LOSS_CLIPPED}[loss]
    a.first, a.count, a.total = 0, count, len(inp["ch"])
    a.adv, a.action = dev.put(inp["adv"]), dev.put(inp["ch"])
    a.p_old = dev.put(inp["p_old"])
    a.eps, a.scale, a.value_scale = vr.EPS, 1.0, 1.0
    g = np.full((max(count, 1), B), -77.5 if fill is None else fill, f32)
    a.grad = dev.put(g)
    for k, v in over.items():
        setattr(a, k, v)
    return a


# --------------------------------------------------------------------- 1 --
@pytest.mark.parametrize("loss", ["log", "clipped"])
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_probs_parity_with_action_loss_grad(ctx, sel, loss):
    """XH_ACT_PROBS at scale 1: grad is xh_action_loss_grad's output on the
    same rows bit for bit, with a distrib whose entry at the choice is p_old;
    also through an index list, and for runs of 1, 64 / LPE - 1 and 64 / LPE +
    1 rows from first > 0."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    probs, ch, adv = inp["probs"], inp["ch"], inp["adv"]
    distrib = np.full((n, B), 0.5, f32)
    distrib[np.arange(n), ch] = inp["p_old"]
    want = np.zeros((n, B), f32)
    kind = {"log": _lib.LOSS_SOFTMAX_GRADIENT_LOG,
            "clipped": _lib.LOSS_CLIPPED}[loss]
    _lib.check(_lib.lib.xh_action_loss_grad(
        ctx.h, kind, n, B, ch.ctypes.data, distrib.ctypes.data,
        adv.ctypes.data, probs.ctypes.data, vr.EPS, want.ctypes.data))
    assert np.count_nonzero(want) >= n
    _bits(want, vr.grad_f32(probs, ch, inp["p_old"], adv, "probs", loss),
          "the restatement")
    env = _venv(ctx, case)
    kw = dict(kind="probs", loss=loss, action=ch, p_old=inp["p_old"],
              eps=vr.EPS)
    _bits(env.policy_loss(probs, adv, **kw)["grad"], want, "all rows")
    g = np.random.default_rng(n)
    rows = g.permutation(n).astype(np.int32)
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


# --------------------------------------------------------------------- 2 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_probs_out_is_the_softmax(ctx, sel):
    """probs_out for logits within (B + 4) 2^-24 (relative) of a float64
    softmax: one-ulp expf on both sides, an f32 sum of B positive terms, one
    division (test_logits_softmax_and_picks derives the bound)."""
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    env = _venv(ctx, case)
    got = env.policy_loss(inp["z"], inp["adv"], kind="logits", loss="clipped",
                          action=inp["ch"], p_old=inp["p_old"],
                          want_probs=True)["probs"]
    rel = np.abs(got.astype(np.float64) / inp["p64"] - 1)
    print("B=%d: max rel error of probs_out %.3g (bound %.3g)"
          % (B, rel.max(), (B + 4) * vr.U32))
    assert np.all(np.abs(got - inp["p64"]) <= (B + 4) * vr.U32 * inp["p64"])
    env.close()


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("loss", ["log", "clipped"])
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_logits_gradient_bits(ctx, sel, loss):
    """grad for logits is the restatement applied to the kernel's own
    probs_out, bit for bit, at scale 1 and at scale 1 / count; the runs of 1,
    64 / LPE - 1 and 64 / LPE + 1 rows too."""
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    env = _venv(ctx, case)
    kw = dict(kind="logits", loss=loss, action=inp["ch"], p_old=inp["p_old"],
              eps=vr.EPS, want_probs=True)
    for first, count in [(0, n)] + [(2, c) for c in (1, _rpw(B) - 1,
                                                     _rpw(B) + 1)
                                    if 1 <= c <= n - 2]:
        sl = slice(first, first + count)
        for scale in (1.0, 1.0 / count):
            got = env.policy_loss(inp["z"][sl], inp["adv"], first=first,
                                  count=count, scale=scale, **kw)
            want = vr.grad_f32(got["probs"], inp["ch"][sl], inp["p_old"][sl],
                               inp["adv"][sl], "logits", loss, vr.EPS,
                               f32(scale))
            _bits(got["grad"], want, "rows %d+%d scale %g"
                  % (first, count, scale))
            assert np.count_nonzero(got["grad"]) == count * B
    env.close()


# --------------------------------------------------------------------- 4 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_logits_gradient_against_float64(ctx, sel):
    """|g - g64| <= (3 (B + 4) + 8) 2^-24 p_k |d64| for the clipped loss: p_k
    and p_ch carry the softmax bound (B + 4) 2^-24 each, d carries it once
    more through p_ch, and every operation rounds once.  No row is excluded
    (tests/test_venv_loss_ref.py shows none has to be)."""
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    rows = np.arange(n)
    p64 = inp["p64"]
    p_ch = p64[rows, inp["ch"]]
    assert vr.excluded_rows(p_ch, inp["p_old"], inp["adv"]).sum() == 0
    d64 = vr.d_clipped_f64(p_ch, inp["p_old"], inp["adv"], vr.EPS)
    hot = np.zeros((n, B))
    hot[rows, inp["ch"]] = 1.0
    g64 = (hot * p64 - p64 * p_ch[:, None]) * d64[:, None]
    env = _venv(ctx, case)
    got = env.policy_loss(inp["z"], inp["adv"], kind="logits", loss="clipped",
                          action=inp["ch"], p_old=inp["p_old"],
                          eps=vr.EPS)["grad"]
    bound = (3 * (B + 4) + 8) * vr.U32 * p64 * np.abs(d64)[:, None]
    ratio = np.abs(got.astype(np.float64) - g64) / bound
    print("B=%d n=%d: max |g - g64| / bound = %.4f" % (B, n, ratio.max()))
    assert np.all(ratio <= 1.0)
    env.close()


# --------------------------------------------------------------------- 5 --
def _exact_advantages(g, n):
    """f32 advantages of both signs with 0.25 <= |A| < 2: multiples of 2^-26
    below 2, so any sum of fewer than 2^20 of them is exact in double and
    every summation order gives math.fsum's bits."""
    return (g.choice([-1.0, 1.0], n) * g.uniform(0.25, 2.0, n)).astype(f32)


@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_epoch_zero(ctx, case, kind):
    """The recorded policy rows fed back with the record's own action and
    p_old, over all rows: p[choice] is the record's PCHOICE bit for bit, so
    every ratio is exactly 1.0f -- no row clipped, log-ratio and k3 sums
    exactly 0.0, and the surrogate's sum is the sum of the advantages."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    g = np.random.default_rng(B + N)
    if kind == "logits":
        rows = (g.standard_normal((vr.T, N, B)) * 3.0).astype(f32)
    else:
        rows = (g.random((vr.T, N, B)) * 5.0 + 1e-3).astype(f32)
    env = _venv(ctx, case)
    env.set_record(vr.T, states=False)
    for t in range(vr.T):
        env.act(rows[t], kind=kind, fetch=False)
    rec = env.record()
    n = vr.T * N
    adv = _exact_advantages(g, n)
    got = env.policy_loss(rows.reshape(n, B), adv, kind=kind, loss="clipped",
                          eps=vr.EPS, want_probs=True, want_stats=True)
    pch = got["probs"][np.arange(n), rec["action"].reshape(-1)]
    _bits(pch, rec["pchoice"].reshape(-1), "p[choice] against PCHOICE")
    st = got["stats"]
    assert st[_lib.VLOSS_ROWS] == n and st[_lib.VLOSS_SKIPPED] == 0
    assert st[_lib.VLOSS_CLIPPED] == 0
    assert st[_lib.VLOSS_LOGR_SUM] == 0.0 and st[_lib.VLOSS_LOGR_SQSUM] == 0.0
    assert st[_lib.VLOSS_K3_SUM] == 0.0
    assert st[_lib.VLOSS_SURR_SUM] == math.fsum(float(x) for x in adv)
    # ratio 1: d = -A / p_ch, the unclipped branch
    want = vr.grad_f32(got["probs"], rec["action"].reshape(-1),
                       rec["pchoice"].reshape(-1), adv, kind, "clipped")
    _bits(got["grad"], want)
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 6 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3]],
                         ids=[IDS[0], IDS[2], IDS[3]])
def test_gather_and_in_place(ctx, case):
    """An index list with duplicates and descending runs, taken from first >
    0, equals the same rows computed one call per row; grad == policy (in
    place) gives the same bits."""
    B = case[0]
    inp = _inputs((case, None))
    n = len(inp["ch"])
    lst = np.array([5, 5, n - 1, n - 2, n - 3, 0, 7, 7, 7, 2, 1, 0, n - 1, 4,
                    9, 8, 3], np.int32)
    first, count = 2, len(lst) - 3
    take = lst[first:first + count]
    z = (np.random.default_rng(B).standard_normal((count, B)) * 2).astype(f32)
    env = _venv(ctx, case)
    kw = dict(kind="logits", loss="clipped", action=inp["ch"],
              p_old=inp["p_old"], eps=vr.EPS)
    got = env.policy_loss(z, inp["adv"], rows=lst, first=first, count=count,
                          **kw)["grad"]
    for j, q in enumerate(take):
        one = env.policy_loss(z[j:j + 1], inp["adv"], first=int(q), count=1,
                              **kw)["grad"]
        _bits(got[j:j + 1], one, "row %d (index %d)" % (j, q))
    dev = Dev(ctx)
    a = _args(dev, inp, z, count, B, "logits", "clipped", first=first,
              rows_dev=dev.put(lst))
    a.grad = a.policy
    dev.lib.check(dev.lib.lib.xh_venv_policy_loss(env.h, C.byref(a)))
    env.synchronize()
    _bits(dev.get(a.policy, f32, (count, B)), got, "in place")
    dev.free()
    env.close()


# --------------------------------------------------------------------- 7 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_refused_rows(ctx, case):
    """A window in which xh_venv_act refused an env (a NaN logit): the row has
    a zero gradient and a zero dvalue and counts in SKIPPED only; it is not an
    error of the loss call."""
    from dependence_free_rl_amd import XhError, _lib
    B, D, N = case
    g = np.random.default_rng(N)
    rows = (g.standard_normal((vr.T, N, B)) * 2.0).astype(f32)
    rows[1, 3, B - 2] = np.nan
    env = _venv(ctx, case)
    env.set_record(vr.T, states=False)
    for t in range(vr.T):
        env.act(rows[t], kind="logits", fetch=False)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()  # the refusal, reported when it happened
    rec = env.record()
    n, q = vr.T * N, N + 3
    assert rec["pchoice"].reshape(-1)[q] == 0.0
    assert np.count_nonzero(rec["pchoice"] == 0) == 1
    adv = _exact_advantages(g, n)
    values = (g.integers(-256, 257, n) / 64.0).astype(f32)
    target = (g.integers(-256, 257, n) / 64.0).astype(f32)
    got = env.policy_loss(rows.reshape(n, B), adv, kind="logits",
                          loss="clipped", values=values, target=target,
                          value_scale=0.5, want_stats=True)
    env.synchronize()  # a skipped row is not an error
    assert not got["grad"][q].any() and got["dvalue"][q] == 0.0
    keep = np.arange(n) != q
    assert np.isfinite(got["grad"][keep]).all()
    assert got["grad"][keep].any(axis=1).all()
    dval, dv = vr.dvalue_f32(values, target, 0.5, rec["pchoice"].reshape(-1))
    _bits(got["dvalue"], dval)
    st = got["stats"]
    assert st[_lib.VLOSS_SKIPPED] == 1 and st[_lib.VLOSS_ROWS] == n - 1
    assert np.isfinite(st).all()
    assert st[_lib.VLOSS_SURR_SUM] == math.fsum(float(x) for x in adv[keep])
    assert st[_lib.VLOSS_VERR_SUM] == math.fsum(float(x) for x in dv[keep])
    env.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_bad_rows_and_bad_arguments(ctx, case):
    """An index of total or -1, or a caller's action of B, leaves its
    prefilled output rows untouched and synchronize reports XH_ERR_INVALID
    once; a misaligned pointer, a partial overlap and each argument error
    return their codes and launch nothing."""
    from dependence_free_rl_amd import _lib
    B = case[0]
    inp = dict(_inputs((case, None)))
    n = len(inp["ch"])
    inp["ch"] = inp["ch"].copy()
    inp["ch"][6] = B
    lst = np.array([4, n, 0, -1, 6, 2, n - 1], np.int32)
    bad = np.array([0, 1, 0, 1, 1, 0, 0], bool)
    count = len(lst)
    z = (np.random.default_rng(B).standard_normal((count, B)) * 2).astype(f32)
    env = _venv(ctx, case)
    dev = Dev(ctx)
    lib = _lib.lib
    fill = np.full((count, B), -77.5, f32)
    a = _args(dev, inp, z, count, B, "logits", "clipped",
              rows_dev=dev.put(lst))
    a.probs_out = dev.put(fill)
    a.values_new = dev.put(np.ones(count, f32))
    a.target = dev.put(np.zeros(n, f32))
    a.dvalue = dev.put(fill[:, 0].copy())
    assert lib.xh_venv_policy_loss(env.h, C.byref(a)) == _lib.XH_OK
    with pytest.raises(_lib.XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()
    env.synchronize()  # reported once
    grad = dev.get(a.grad, f32, (count, B))
    probs = dev.get(a.probs_out, f32, (count, B))
    dval = dev.get(a.dvalue, f32, (count,))
    _bits(grad[bad], fill[bad])
    _bits(probs[bad], fill[bad])
    _bits(dval[bad], fill[bad, 0])
    ok = lst[~bad]
    _bits(grad[~bad], vr.grad_f32(probs[~bad], inp["ch"][ok], inp["p_old"][ok],
                                  inp["adv"][ok], "logits", "clipped"))
    _bits(dval[~bad], np.ones(4, f32))

    # ---- argument errors: nothing is launched, the outputs keep their fill
    def refused(code, **over):
        b = _args(dev, inp, z, count, B, "logits", "clipped")
        grad = b.grad
        for k, v in over.items():
            setattr(b, k, v(b) if callable(v) else v)
        assert lib.xh_venv_policy_loss(env.h, C.byref(b)) == code, over
        _bits(dev.get(grad, f32, (count, B)), fill, str(over))
        _bits(dev.get(b.policy & ~15 if b.policy else grad, f32, (count, B)),
              z if b.policy else fill, str(over))

    INV = _lib.XH_ERR_INVALID
    assert lib.xh_venv_policy_loss(env.h, None) == INV
    for name in ("policy", "adv", "grad"):
        refused(INV, **{name: None})
    refused(INV, kind=2)
    refused(INV, loss=_lib.LOSS_KL_REGULATED)
    refused(INV, loss=_lib.LOSS_GRADIENT_LOG)
    refused(INV, first=-1)
    refused(INV, count=-1)
    refused(INV, first=n - count + 1)        # a run past total
    for eps in (0.0, -0.1, float("nan"), float("inf")):
        refused(INV, eps=eps)
    one = dev.put(np.ones(n, f32))
    refused(INV, values_new=one)              # neither target nor dvalue
    refused(INV, values_new=one, target=one)  # no dvalue
    refused(INV, values_new=one, dvalue=one)  # no target
    refused(INV, policy=lambda b: b.policy + 4)
    refused(INV, grad=lambda b: b.grad + 8)
    refused(INV, probs_out=lambda b: dev.alloc(count * B * 4) + 4)
    refused(INV, grad=lambda b: b.policy + 16)       # a partial overlap
    refused(INV, probs_out=lambda b: b.policy)       # only grad may alias
    refused(INV, probs_out=lambda b: b.grad + 16 * B)
    refused(_lib.XH_ERR_STATE, action=None)          # no record to take it from
    refused(_lib.XH_ERR_STATE, p_old=None)
    b = _args(dev, inp, z, 0, B, "logits", "clipped")
    assert lib.xh_venv_policy_loss(env.h, C.byref(b)) == _lib.XH_OK  # count 0
    # eps is not read by the log loss (rows 0 .. 5: row 6 has the bad action)
    b = _args(dev, inp, z, count - 1, B, "logits", "log", eps=0.0)
    assert lib.xh_venv_policy_loss(env.h, C.byref(b)) == _lib.XH_OK
    env.synchronize()
    dev.free()
    env.close()


# --------------------------------------------------------------------- 8 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_statistics(ctx, sel):
    """Every entry within 1e-12 (relative) of the float64 restatement on the
    kernel's own probabilities -- LOGR_SUM, which cancels, within 1e-12 of the
    sum of its terms' magnitudes; two runs give the same bits; accumulate over
    three minibatches is the three calls' rows added in call order, bit for
    bit; the value-error sums (exact in double for these inputs) and dvalue
    are the restatement's bits."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    inp = _inputs(sel)
    n = len(inp["ch"])
    g = np.random.default_rng(n)
    values = (g.integers(-256, 257, n) / 64.0).astype(f32)
    target = (g.integers(-256, 257, n) / 64.0).astype(f32)
    env = _venv(ctx, case)
    kw = dict(kind="logits", loss="clipped", action=inp["ch"],
              p_old=inp["p_old"], eps=vr.EPS, target=target, value_scale=0.25,
              want_probs=True, want_stats=True)
    runs = [env.policy_loss(inp["z"], inp["adv"], values=values, **kw)
            for _ in range(2)]
    got = runs[0]
    assert got["stats"].tobytes() == runs[1]["stats"].tobytes()
    dval, dv = vr.dvalue_f32(values, target, 0.25, inp["p_old"])
    _bits(got["dvalue"], dval)
    want, logr_mag = vr.stats_f64(got["probs"], inp["ch"], inp["p_old"],
                                  inp["adv"], vr.EPS, dv)
    st = got["stats"]
    assert st.shape == (_lib.VLOSS_COUNT,)
    tol = 1e-12 * np.abs(want)
    tol[_lib.VLOSS_LOGR_SUM] = 1e-12 * logr_mag
    print("stats: |got - want| / tol =",
          np.abs(st - want) / np.where(tol > 0, tol, 1.0))
    assert np.all(np.abs(st - want) <= tol)
    for k in (_lib.VLOSS_ROWS, _lib.VLOSS_SKIPPED, _lib.VLOSS_CLIPPED,
              _lib.VLOSS_VERR_SUM, _lib.VLOSS_VERR_SQSUM):
        assert st[k] == want[k], k
    assert st[_lib.VLOSS_ROWS] == n and 0 < st[_lib.VLOSS_CLIPPED] < n
    # three uneven minibatches
    cuts = [0, n // 5, n // 5 + n // 2 + 1, n]
    parts, acc = [], None
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        args = (inp["z"][lo:hi], inp["adv"])
        mkw = dict(kw, first=lo, count=hi - lo, values=values[lo:hi])
        parts.append(env.policy_loss(*args, **mkw)["stats"])
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        mkw = dict(kw, first=lo, count=hi - lo, values=values[lo:hi])
        acc = env.policy_loss(inp["z"][lo:hi], inp["adv"], accumulate=i > 0,
                              **mkw)["stats"]
    chain = (parts[0] + parts[1]) + parts[2]
    assert acc.tobytes() == chain.tobytes()
    env.close()


# --------------------------------------------------------------------- 9 --
@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_nothing_else_moved(ctx, case):
    """The venv's bins, items, stream states, actions, record and cursor are
    what they were after loss calls of every form, and the next act() still
    records into the next slot."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    g = np.random.default_rng(N)
    rows = (g.standard_normal((vr.T + 1, N, B)) * 2.0).astype(f32)
    env = _venv(ctx, case)
    env.set_record(vr.T + 1)
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
    n = vr.T * N
    adv = _exact_advantages(g, n)
    z = rows[:vr.T].reshape(n, B)
    env.policy_loss(z, adv, want_probs=True, want_stats=True)
    perm = g.permutation(n)[:N + 3].astype(np.int32)
    env.policy_loss(z[perm], adv, loss="log", rows=perm, values=adv[perm],
                    target=adv, want_stats=True, accumulate=True)
    env.policy_loss(np.abs(z) + f32(0.01), adv, kind="probs", scale=1.0 / n)
    env.synchronize()
    after = state()
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    env.act(rows[vr.T], kind="logits", fetch=False)
    assert env.record_pos() == vr.T + 1
    rec = env.record()
    for x, y in zip(before[7:-1], [rec[k] for k in sorted(rec)]):
        np.testing.assert_array_equal(x, y[:vr.T])
    env.synchronize()
    env.close()
