"""GPU tests of xh_venv_policy_loss_ex: the entropy bonus and PPO2's clipped
value loss of the VecEnv loss head, against tests/venv_ppo_ref.py (pinned on
the CPU by tests/test_venv_ppo_ref.py) and the existing restatements of the
loss's own rows (venv_loss_ref.py, venv_kl_ref.py).

Shapes: test_gpu_venv_loss.py's -- venv_loss_ref.CASES with T = 4 (8 .. 128
bins, one to eight lanes per row, 76 .. 280 rows), 600 rows of 8 bins (several
block partials), 72 rows of 16 bins (more than one wave of rows), and runs of
1, 64 / LPE - 1 and 64 / LPE + 1 rows from first > 0.  No row is excluded.

The device's logarithm is logf and the host's is numpy's: both within an ulp
but not the same bits, so the bonus is compared with float64 on the kernel's
own probs_out within venv_ppo_ref.entropy_bound; everything around it (the
loss's own row, the value head, the statistics' exact entries) is bit for
bit."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import venv_kl_ref as kr
import venv_loss_ref as vr
import venv_mask_ref as mr
import venv_ppo_ref as pr
from test_gpu_venv_loss import (CASES, IDS, SET_IDS, SETS, Dev, _args, _bits,
                                _inputs, _rpw, _venv)

pytestmark = pytest.mark.gpu

f32 = np.float32
U = vr.U32
COEFS = tuple(float(np.float32(c)) for c in (0.01, 0.37))  # as the ABI holds them
BETA = 0.3


@functools.lru_cache(maxsize=None)
def _q(sel):
    q = kr.kl_inputs(sel)
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def _vals(n):
    inp = pr.vclip_inputs(n)
    for v in inp.values():
        v.setflags(write=False)
    return inp


def _runs(B, n, first=2):
    return [(0, n)] + [(first, c) for c in (1, _rpw(B) - 1, _rpw(B) + 1)
                       if 1 <= c <= n - first]


def _within(got, want64, tol, what):
    err = np.abs(got.astype(np.float64) - want64)
    ratio = (err / np.where(tol > 0, tol, 1.0)).max()
    print("%s: max |got - want| / tol = %.4f" % (what, ratio))
    assert np.all(err <= tol), what
    return ratio


def _ent_check(got, g, c, kind, scale, what):
    """grad == (g + e64) * scale within (the entropy bound + 2 u |g + e|) *
    scale, e64 the float64 term on the kernel's own probabilities."""
    p = got["probs"]
    e64, _ = pr.entropy_grad_f64(p, c, kind)
    s = float(f32(scale))
    want = (g.astype(np.float64) + e64) * s
    tol = (pr.entropy_bound(p, c, kind) + 2 * U * np.abs(want / s)) * s
    return _within(got["grad"], want, tol, what)


# --------------------------------------------------------------------- 1 --
def _raw_outputs(env, dev, inp, q, vals, B, kind, loss, call):
    """One raw call with every output asked for, each in a prefilled block of
    its own; returns the outputs' bytes."""
    _lib = dev.lib
    n = len(inp["ch"])
    a = _args(dev, inp, inp["z"] if kind == "logits" else inp["probs"], n, B,
              kind, "log" if loss == "kl" else loss)
    if loss == "kl":
        a.loss, a.beta = _lib.LOSS_KL_REGULATED, BETA
    fill = np.full((n, B), -77.5, f32)
    a.distrib = dev.put(q)
    a.probs_out = dev.put(fill)
    a.values_new, a.target = dev.put(vals["vn"]), dev.put(vals["tg"])
    a.dvalue, a.value_scale = dev.put(fill[:, 0].copy()), 0.5
    a.stats = dev.put(np.full(_lib.VLOSS_COUNT, -1.0))
    a.kl_stats = dev.put(np.full(_lib.VKL_COUNT, -1.0))
    assert call(a) == _lib.XH_OK, _lib.lib.xh_last_error()
    env.synchronize()
    out = [dev.get(a.grad, f32, (n, B)), dev.get(a.dvalue, f32, (n,)),
           dev.get(a.probs_out, f32, (n, B)),
           dev.get(a.stats, np.float64, (_lib.VLOSS_COUNT,)),
           dev.get(a.kl_stats, np.float64, (_lib.VKL_COUNT,))]
    assert out[3][_lib.VLOSS_ROWS] == n and out[4][_lib.VKL_ROWS] == n
    return [o.tobytes() for o in out]


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_extension_off_is_the_plain_call(ctx, sel):
    """_ex with x NULL and with a zeroed x: grad, dvalue, probs_out, stats and
    kl_stats bit for bit as xh_venv_policy_loss, under each loss kind; with
    masked (the caller's words) as xh_venv_policy_loss_masked."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp, q = _inputs(sel), _q(sel)
    n = len(inp["ch"])
    vals = _vals(n)
    lib = _lib.lib
    env, dev = _venv(ctx, case), Dev(ctx)
    g = np.random.default_rng(n + B)
    legal = g.random((n, B)) < 0.6
    legal[np.arange(n), inp["ch"]] = True
    legal[::9] = False  # no legal bin: left unmasked
    words = dev.put(mr.pack(legal))
    zeroed = _lib.VenvLossExt()
    masked = _lib.VenvLossExt()
    masked.masked, masked.legal_dev = 1, words
    for kind, loss in (("logits", "clipped"), ("probs", "log"),
                       ("logits", "kl")):
        def run(call):
            return _raw_outputs(env, dev, inp, q, vals, B, kind, loss, call)
        plain = run(lambda a: lib.xh_venv_policy_loss(env.h, C.byref(a)))
        assert run(lambda a: lib.xh_venv_policy_loss_ex(
            env.h, C.byref(a), None)) == plain, (kind, loss, "NULL")
        assert run(lambda a: lib.xh_venv_policy_loss_ex(
            env.h, C.byref(a), C.byref(zeroed))) == plain, (kind, loss, "0")
        pm = run(lambda a: lib.xh_venv_policy_loss_masked(
            env.h, C.byref(a), words))
        assert pm != plain
        assert run(lambda a: lib.xh_venv_policy_loss_ex(
            env.h, C.byref(a), C.byref(masked))) == pm, (kind, loss, "masked")
        dev.free()
        words = dev.put(mr.pack(legal))
        masked.legal_dev = words
    dev.free()
    env.close()


# --------------------------------------------------------------------- 2 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_entropy_alone(ctx, sel, kind):
    """adv = 0 under the log loss makes the loss's own row exact zeros, so
    grad is e * scale: within the bound of tests/venv_ppo_ref.py plus one
    rounding for scale of float64 on the kernel's own probs_out; c in {0.01,
    0.37}, scale 1 and 1 / count, and the short runs from first > 0."""
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    pol = inp["z"] if kind == "logits" else inp["probs"]
    zero = np.zeros(n, f32)
    env = _venv(ctx, case)
    kw = dict(kind=kind, loss="log", action=inp["ch"], p_old=inp["p_old"],
              want_probs=True)
    worst = 0.0
    for first, count in _runs(B, n):
        sl = slice(first, first + count)
        for c in COEFS:
            for scale in (1.0, 1.0 / count):
                got = env.policy_loss(pol[sl], zero, first=first, count=count,
                                      scale=scale, ent_coef=c, **kw)
                p = got["probs"]
                e64, _ = pr.entropy_grad_f64(p, c, kind)
                s = float(f32(scale))
                tol = (pr.entropy_bound(p, c, kind) + U * np.abs(e64)) * s
                worst = max(worst, _within(
                    got["grad"], e64 * s, tol, "rows %d+%d c=%g scale=%g"
                    % (first, count, c, scale)))
                assert np.count_nonzero(got["grad"]) >= count * (B - 1)
        off = env.policy_loss(pol[sl], zero, first=first, count=count, **kw)
        assert not off["grad"].any()  # the loss's own row: exact zeros
    print("B=%d %s: worst ratio %.4f" % (B, kind, worst))
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("loss", ["log", "clipped", "kl"])
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_entropy_with_each_loss(ctx, sel, loss):
    """grad = (g + e64) * scale, g the existing restatement of the loss's row
    on the kernel's probs_out ("kl": the caller's distributions), within the
    entropy bound plus 2 * 2^-24 |g + e|; both kinds, scale 1 and 1 / count.
    The clipped loss also in place (grad == policy) and through a shuffled
    index list, bit for bit."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    q = _q(sel)
    env = _venv(ctx, case)
    c = COEFS[1]
    for kind in ("logits", "probs"):
        pol = inp["z"] if kind == "logits" else inp["probs"]
        kw = dict(kind=kind, loss=loss, action=inp["ch"], p_old=inp["p_old"],
                  eps=vr.EPS, want_probs=True, ent_coef=c)
        if loss == "kl":
            kw.update(beta=BETA, distrib=q)
        for scale in (1.0, 1.0 / n):
            got = env.policy_loss(pol, inp["adv"], scale=scale, **kw)
            if loss == "kl":
                g = kr.kl_grad_f32(got["probs"], q, inp["ch"], inp["p_old"],
                                   inp["adv"], BETA)
            else:
                g = vr.grad_f32(got["probs"], inp["ch"], inp["p_old"],
                                inp["adv"], kind, loss, vr.EPS)
            _ent_check(got, g, c, kind, scale,
                       "B=%d %s %s scale=%g" % (B, kind, loss, scale))
        # the bonus moved the row: it is not the plain call's
        plain = env.policy_loss(pol, inp["adv"], scale=1.0 / n,
                                **dict(kw, ent_coef=0.0))
        assert np.count_nonzero(plain["grad"] != got["grad"]) > n
    if loss == "clipped":
        kw = dict(kind="logits", loss="clipped", action=inp["ch"],
                  p_old=inp["p_old"], eps=vr.EPS, ent_coef=c)
        full = env.policy_loss(inp["z"], inp["adv"], **kw)["grad"]
        rows = np.random.default_rng(n).permutation(n).astype(np.int32)
        _bits(env.policy_loss(inp["z"][rows], inp["adv"], rows=rows,
                              **kw)["grad"], full[rows], "index list")
        dev = Dev(ctx)
        a = _args(dev, inp, inp["z"], n, B, "logits", "clipped")
        a.grad = a.policy
        x = _lib.VenvLossExt()
        x.ent_coef = c
        _lib.check(_lib.lib.xh_venv_policy_loss_ex(env.h, C.byref(a),
                                                   C.byref(x)))
        env.synchronize()
        _bits(dev.get(a.policy, f32, (n, B)), full, "in place")
        dev.free()
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 4 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3]],
                         ids=[IDS[0], IDS[2], IDS[3]])
def test_ent_coef_dev(ctx, case):
    """A device float gives the bits of the same value passed by field, and a
    device 0.0f the bits of no bonus."""
    B = case[0]
    inp = _inputs((case, None))
    env, dev = _venv(ctx, case), Dev(ctx)
    kw = dict(kind="logits", loss="clipped", action=inp["ch"],
              p_old=inp["p_old"], eps=vr.EPS)
    for c in COEFS + (0.0,):
        by_field = env.policy_loss(inp["z"], inp["adv"], ent_coef=float(f32(c)),
                                   **kw)["grad"]
        ptr = dev.put(np.array([c], f32))
        by_ptr = env.policy_loss(inp["z"], inp["adv"], ent_coef=ptr,
                                 **kw)["grad"]
        _bits(by_ptr, by_field, "c=%g" % c)
    with pytest.raises(ValueError, match="ent_coef"):
        env.policy_loss(inp["z"], inp["adv"], ent_coef=1, **kw)
    env.synchronize()
    dev.free()
    env.close()


# --------------------------------------------------------------------- 5 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_masked_with_the_bonus(ctx, case, kind):
    """_ex with masked and the bonus equals _ex unmasked on the premasked rows
    (-inf or 0) bit for bit; every entry at a masked bin is exactly 0; and
    under logits a row whose legal set is one bin has an all-zero entropy
    term."""
    B = case[0]
    inp = _inputs((case, None))
    n = len(inp["ch"])
    g = np.random.default_rng(3 * n + B)
    legal = g.random((n, B)) < 0.5
    legal[::6] = False
    legal[np.arange(n), inp["ch"]] = True   # the taken bin is legal (every
    legal[5::13] = False                    # 6th row: the only one); no
    single = legal.sum(axis=1) == 1         # legal bin: left unmasked
    eff = mr.eff(legal)
    pol = inp["z"] if kind == "logits" else inp["probs"]
    pre = mr.premask(pol, eff, kind)
    env = _venv(ctx, case)
    c = COEFS[1]
    kw = dict(kind=kind, loss="clipped", action=inp["ch"], p_old=inp["p_old"],
              eps=vr.EPS, want_probs=True, ent_coef=c)
    got = env.policy_loss(pol, inp["adv"], legal=legal, **kw)
    want = env.policy_loss(pre, inp["adv"], **kw)
    _bits(got["grad"], want["grad"], "grad")
    _bits(got["probs"], want["probs"], "probs")
    assert not got["grad"][~eff].any() and not got["probs"][~eff].any()
    assert np.isfinite(got["grad"]).all()
    zero = np.zeros(n, f32)
    alone = env.policy_loss(pol, zero, legal=legal, **dict(kw, loss="log"))
    assert not alone["grad"][~eff].any()
    assert alone["grad"][~single].any(axis=1).all()
    if kind == "logits":
        assert single.sum() >= 3 and not alone["grad"][single].any()
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 6 --
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_epoch_zero(ctx, case):
    """A recorded window fed back, no parameter moved, the bonus on: stats
    still shows every ratio exactly 1 (the bonus does not disturb p_ch), a
    uniform row of logits has an entropy term within the bound of 0, and the
    KL loss on the recorded distributions is (g + e64) * scale."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    g = np.random.default_rng(B + N)
    rows = (g.standard_normal((vr.T, N, B)) * 3.0).astype(f32)
    rows[1, 2] = f32(0.75)  # a uniform row
    env = _venv(ctx, case)
    env.set_record(vr.T, states=False, distrib=True)
    for t in range(vr.T):
        env.act(rows[t], kind="logits", fetch=False)
    rec = env.record()
    n = vr.T * N
    ch, pch = rec["action"].reshape(-1), rec["pchoice"].reshape(-1)
    adv = (g.choice([-1.0, 1.0], n) * g.uniform(0.25, 2.0, n)).astype(f32)
    z = rows.reshape(n, B)
    c = COEFS[1]
    got = env.policy_loss(z, adv, kind="logits", loss="clipped", eps=vr.EPS,
                          want_probs=True, want_stats=True, ent_coef=c)
    _bits(got["probs"][np.arange(n), ch], pch, "p[choice] against PCHOICE")
    st = got["stats"]
    assert st[_lib.VLOSS_ROWS] == n and st[_lib.VLOSS_CLIPPED] == 0
    assert st[_lib.VLOSS_LOGR_SUM] == 0.0 and st[_lib.VLOSS_LOGR_SQSUM] == 0.0
    _ent_check(got, vr.grad_f32(got["probs"], ch, pch, adv, "logits",
                                "clipped"), c, "logits", 1.0, "clipped")
    alone = env.policy_loss(z, np.zeros(n, f32), kind="logits", loss="log",
                            want_probs=True, ent_coef=c)
    u = N + 2
    assert np.all(alone["probs"][u] == alone["probs"][u, 0])
    bound = pr.entropy_bound(alone["probs"], c, "logits")
    assert np.all(np.abs(alone["grad"][u]) <= bound[u])
    assert alone["grad"].any(axis=1).sum() >= n - 1
    kl = env.policy_loss(z, adv, kind="logits", loss="kl", beta=BETA,
                         scale=1.0 / n, want_probs=True, ent_coef=c)
    q = rec["distrib"].reshape(n, B)
    _bits(kl["probs"], q, "p against the recorded distributions")
    _ent_check(kl, kr.kl_grad_f32(kl["probs"], q, ch, pch, adv, BETA), c,
               "logits", 1.0 / n, "kl, recorded")
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 7 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_value_clip(ctx, sel):
    """dvalue is the f32 restatement bit for bit on the binary-fraction
    inputs (every regime in both signs), at value_scale 1 and 0.5, through an
    index list, over the short runs and with skipped rows (zeros); the
    XH_VLOSS_VERR_* sums are those of a call without v_old."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    v = _vals(n)
    assert sorted(set(v["regime"].tolist())) == list(range(10))
    p_old = inp["p_old"].copy()
    p_old[[1, n // 2]] = 0  # skipped rows
    env = _venv(ctx, case)
    kw = dict(kind="logits", loss="clipped", action=inp["ch"], p_old=p_old,
              eps=vr.EPS, target=v["tg"])
    for scale in (1.0, 0.5):
        want, zero, _, _ = pr.vclip_f32(v["vn"], v["tg"], v["vo"], pr.VCLIP,
                                        scale, p_old)
        assert 0 < zero.sum() < n
        for first, count in _runs(B, n, first=1):
            sl = slice(first, first + count)
            got = env.policy_loss(inp["z"][sl], inp["adv"], first=first,
                                  count=count, values=v["vn"][sl],
                                  v_old=v["vo"], vclip=pr.VCLIP,
                                  value_scale=scale, **kw)
            _bits(got["dvalue"], want[sl], "rows %d+%d scale %g"
                  % (first, count, scale))
        rows = np.random.default_rng(n).permutation(n).astype(np.int32)
        got = env.policy_loss(inp["z"][rows], inp["adv"], rows=rows,
                              values=v["vn"][rows], v_old=v["vo"],
                              vclip=pr.VCLIP, value_scale=scale, **kw)
        _bits(got["dvalue"], want[rows], "index list")
    base = dict(kw, values=v["vn"], value_scale=0.5, want_stats=True)
    plain = env.policy_loss(inp["z"], inp["adv"], **base)
    clip = env.policy_loss(inp["z"], inp["adv"], v_old=v["vo"],
                           vclip=pr.VCLIP, **base)
    assert plain["stats"].tobytes() == clip["stats"].tobytes()
    assert plain["stats"][_lib.VLOSS_VERR_SQSUM] > 0
    _bits(plain["grad"], clip["grad"], "the policy's gradient")
    assert np.count_nonzero(plain["dvalue"] != clip["dvalue"]) > 0
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 8 --
@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_ext_stats(ctx, sel):
    """ROWS, VCLIP_ROWS and (on binary fractions) VLOSS_SUM are exact;
    ENTROPY_SUM is within (B + 2) 2^-24 sum H of the fsum of the float64
    entropies of probs_out ((B + 1) u on each row's f32 sum, the rest for the
    double sums); two runs give the same bits; accumulate over two
    half-minibatches is the two calls' rows added in call order and, in the
    exact entries, the whole; without the bonus or the value head their sums
    are 0."""
    from dependence_free_rl_amd import _lib
    case, _ = sel
    B = case[0]
    inp = _inputs(sel)
    n = len(inp["ch"])
    v = _vals(n)
    env = _venv(ctx, case)
    c = COEFS[0]
    kw = dict(kind="logits", loss="clipped", action=inp["ch"],
              p_old=inp["p_old"], eps=vr.EPS, target=v["tg"], v_old=v["vo"],
              vclip=pr.VCLIP, ent_coef=c, want_probs=True, want_ext=True)
    runs = [env.policy_loss(inp["z"], inp["adv"], values=v["vn"], **kw)
            for _ in range(2)]
    got = runs[0]
    st = got["ext_stats"]
    assert st.shape == (_lib.VEXT_COUNT,)
    assert st.tobytes() == runs[1]["ext_stats"].tobytes()
    want = pr.ext_stats_f64(got["probs"], inp["p_old"], True, v["vn"],
                            v["tg"], v["vo"])
    print("ext_stats", st, want, "entropy error / tol = %.4f" % (
        abs(st[pr.ENTROPY_SUM] - want[pr.ENTROPY_SUM]) /
        ((B + 2) * U * want[pr.ENTROPY_SUM])))
    assert st[_lib.VEXT_ROWS] == want[pr.ROWS] == n
    assert st[_lib.VEXT_VCLIP_ROWS] == want[pr.VCLIP_ROWS] > 0
    assert st[_lib.VEXT_VLOSS_SUM] == want[pr.VLOSS_SUM] > 0
    assert (abs(st[_lib.VEXT_ENTROPY_SUM] - want[pr.ENTROPY_SUM]) <=
            (B + 2) * U * want[pr.ENTROPY_SUM])
    h = n // 2 + 1
    cuts = [(0, h), (h, n)]
    parts = [env.policy_loss(inp["z"][lo:hi], inp["adv"], first=lo,
                             count=hi - lo, values=v["vn"][lo:hi],
                             **kw)["ext_stats"] for lo, hi in cuts]
    for i, (lo, hi) in enumerate(cuts):
        acc = env.policy_loss(inp["z"][lo:hi], inp["adv"], first=lo,
                              count=hi - lo, values=v["vn"][lo:hi],
                              accumulate=i > 0, **kw)["ext_stats"]
    assert acc.tobytes() == (parts[0] + parts[1]).tobytes()
    for k in (_lib.VEXT_ROWS, _lib.VEXT_VCLIP_ROWS, _lib.VEXT_VLOSS_SUM):
        assert acc[k] == st[k], k
    # n positive terms: any order of double additions is within n 2^-53
    assert (abs(acc[_lib.VEXT_ENTROPY_SUM] - st[_lib.VEXT_ENTROPY_SUM]) <=
            n * 2.0 ** -53 * st[_lib.VEXT_ENTROPY_SUM])
    # without the bonus / the clip / the value head
    k2 = dict(kw, ent_coef=0.0)
    no_ent = env.policy_loss(inp["z"], inp["adv"], values=v["vn"],
                             **k2)["ext_stats"]
    assert no_ent[_lib.VEXT_ENTROPY_SUM] == 0.0
    assert no_ent[_lib.VEXT_VLOSS_SUM] == st[_lib.VEXT_VLOSS_SUM]
    k3 = dict(kw, v_old=None, vclip=None)
    no_clip = env.policy_loss(inp["z"], inp["adv"], values=v["vn"],
                              **k3)["ext_stats"]
    plain = pr.ext_stats_f64(got["probs"], inp["p_old"], True, v["vn"],
                             v["tg"], None)
    assert no_clip[_lib.VEXT_VCLIP_ROWS] == 0
    assert no_clip[_lib.VEXT_VLOSS_SUM] == plain[pr.VLOSS_SUM]
    assert no_clip[_lib.VEXT_ENTROPY_SUM] == st[_lib.VEXT_ENTROPY_SUM]
    k4 = dict(k3, target=None)
    no_head = env.policy_loss(inp["z"], inp["adv"], **k4)["ext_stats"]
    assert no_head[_lib.VEXT_VLOSS_SUM] == 0.0 and no_head[_lib.VEXT_ROWS] == n
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 9 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_skipped_and_bad_rows(ctx, case):
    """A p_old == 0 row gives zeros and is counted nowhere in ext_stats; an
    index of total or -1 leaves its prefilled output rows untouched and
    synchronize reports XH_ERR_INVALID once, as the plain call does."""
    from dependence_free_rl_amd import _lib
    B = case[0]
    inp = dict(_inputs((case, None)))
    n = len(inp["ch"])
    v = _vals(n)
    inp["p_old"] = inp["p_old"].copy()
    inp["p_old"][4] = 0
    lst = np.array([4, n, 0, -1, 6, 2, n - 1], np.int32)
    bad = np.array([0, 1, 0, 1, 0, 0, 0], bool)
    skip = np.array([1, 0, 0, 0, 0, 0, 0], bool)
    count = len(lst)
    z = (np.random.default_rng(B).standard_normal((count, B)) * 2).astype(f32)
    env, dev = _venv(ctx, case), Dev(ctx)
    fill = np.full((count, B), -77.5, f32)
    a = _args(dev, inp, z, count, B, "logits", "clipped",
              rows_dev=dev.put(lst))
    a.probs_out = dev.put(fill)
    ok = np.where(bad, 0, lst)
    a.values_new = dev.put(v["vn"][ok])
    a.target = dev.put(v["tg"])
    a.dvalue = dev.put(fill[:, 0].copy())
    x = _lib.VenvLossExt()
    x.ent_coef, x.v_old, x.vclip = COEFS[1], dev.put(v["vo"]), pr.VCLIP
    x.ext_stats = dev.put(np.full(_lib.VEXT_COUNT, -1.0))
    assert _lib.lib.xh_venv_policy_loss_ex(env.h, C.byref(a),
                                           C.byref(x)) == _lib.XH_OK
    with pytest.raises(_lib.XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()
    env.synchronize()  # reported once
    grad = dev.get(a.grad, f32, (count, B))
    probs = dev.get(a.probs_out, f32, (count, B))
    dval = dev.get(a.dvalue, f32, (count,))
    st = dev.get(x.ext_stats, np.float64, (_lib.VEXT_COUNT,))
    _bits(grad[bad], fill[bad])
    _bits(probs[bad], fill[bad])
    _bits(dval[bad], fill[bad, 0])
    assert not grad[skip].any() and not dval[skip].any()
    live = ~bad & ~skip
    q = lst[live]
    got = {"grad": grad[live], "probs": probs[live]}
    _ent_check(got, vr.grad_f32(probs[live], inp["ch"][q], inp["p_old"][q],
                                inp["adv"][q], "logits", "clipped"),
               COEFS[1], "logits", 1.0, "the live rows")
    wantv, zero, e1, e2 = pr.vclip_f32(v["vn"][q], v["tg"][q], v["vo"][q],
                                       pr.VCLIP, 1.0)
    _bits(dval[live], wantv)
    assert st[_lib.VEXT_ROWS] == live.sum()
    assert st[_lib.VEXT_VCLIP_ROWS] == zero.sum()
    assert st[_lib.VEXT_VLOSS_SUM] == math.fsum(
        float(b) ** 2 if z_ else float(a_) ** 2
        for a_, b, z_ in zip(e1, e2, zero))
    _, H = pr.entropy_grad_f64(probs[live], 1.0, "logits")
    assert (abs(st[_lib.VEXT_ENTROPY_SUM] - math.fsum(H)) <=
            (B + 2) * U * math.fsum(H))
    dev.free()
    env.close()


# -------------------------------------------------------------------- 10 --
@pytest.mark.parametrize("case", [CASES[2]], ids=[IDS[2]])
def test_refusals(ctx, case):
    """Each XH_ERR_INVALID of xh_venv_policy_loss_ex with its message, what
    the plain call refuses with its code, and nothing launched (the outputs
    keep their fill)."""
    from dependence_free_rl_amd import _lib
    B = case[0]
    inp = _inputs((case, None))
    n = len(inp["ch"])
    v = _vals(n)
    env, dev = _venv(ctx, case), Dev(ctx)
    lib, INV = _lib.lib, _lib.XH_ERR_INVALID
    fill = np.full((n, B), -77.5, f32)
    vo = dev.put(v["vo"])
    cdev = dev.put(np.array([0.1], f32))

    def call(code, msg, head=True, loss_over=None, **over):
        a = _args(dev, inp, inp["z"], n, B, "logits", "clipped")
        if head:
            a.values_new, a.target = dev.put(v["vn"]), dev.put(v["tg"])
            a.dvalue = dev.put(fill[:, 0].copy())
        for k, val in (loss_over or {}).items():
            setattr(a, k, val)
        x = _lib.VenvLossExt()
        for k, val in over.items():
            setattr(x, k, val)
        assert lib.xh_venv_policy_loss_ex(env.h, C.byref(a),
                                          C.byref(x)) == code, over
        if msg:
            assert msg in lib.xh_last_error(), (over, lib.xh_last_error())
        env.synchronize()
        _bits(dev.get(a.grad, f32, (n, B)), fill, str(over))

    for c in (-0.5, float("nan"), float("inf"), -float("inf")):
        call(INV, b"ent_coef", ent_coef=c)
    call(INV, b"values_new", head=False, v_old=vo, vclip=pr.VCLIP)
    for vc in (0.0, -0.25, float("nan"), float("inf")):
        call(INV, b"vclip", v_old=vo, vclip=vc)
    call(INV, b"legal_dev", legal_dev=vo)
    call(INV, b"legal_dev", legal_dev=vo, ent_coef=0.1)
    # what the plain call refuses, extension on or off
    for ext in ({}, {"ent_coef": 0.1}):
        call(INV, b"eps", loss_over={"eps": 0.0}, **ext)
        call(INV, b"null", loss_over={"adv": None}, **ext)
        call(INV, None, loss_over={"loss": _lib.LOSS_KL_REGULATED}, **ext)
        call(_lib.XH_ERR_STATE, None, loss_over={"action": None}, **ext)
        call(_lib.XH_ERR_STATE, None, masked=1, **ext)  # no recorded words
    assert lib.xh_venv_policy_loss_ex(env.h, None, None) == INV
    assert lib.xh_venv_policy_loss_ex(None, None, None) == INV
    assert b"null" in lib.xh_last_error()
    # a negative ent_coef is not read beside ent_coef_dev; vclip not without
    # v_old
    a = _args(dev, inp, inp["z"], n, B, "logits", "clipped")
    x = _lib.VenvLossExt()
    x.ent_coef, x.ent_coef_dev, x.vclip = -1.0, cdev, -1.0
    assert lib.xh_venv_policy_loss_ex(env.h, C.byref(a),
                                      C.byref(x)) == _lib.XH_OK
    env.synchronize()
    by_ptr = dev.get(a.grad, f32, (n, B))
    want = env.policy_loss(inp["z"], inp["adv"], kind="logits",
                           loss="clipped", action=inp["ch"],
                           p_old=inp["p_old"], eps=vr.EPS,
                           ent_coef=float(f32(0.1)))["grad"]
    _bits(by_ptr, want)
    dev.free()
    env.close()
