"""Global-norm gradient clipping on the device (xh_trainer_set_grad_clip,
xh_trainer_get_grad_clip_log, xh_clip_grad_norm) against a host restatement.

What one clipped optimizer step must satisfy, with g the reduced gradient the
trainer reports (XH_BUF_POLICY_GRADS row k / XH_BUF_VALUE_GRAD, not scaled):

* norm: want = sqrt(fsum(g^2)) * r in double (r = 1 / (T * N) with
  lr_scale_rows, else 1).  |norm - want| <= (n + 8) * 2^-53 * want: the terms
  are non-negative, so a double sum of n rounded products in any order is
  within (n + 1) * 2^-53 of the exact sum relatively; the root halves that
  and the device's root and product and the host's add one 2^-53 each:
  (n / 2 + 5) * 2^-53 <= (n + 8) * 2^-53.  Derived, not measured.
* scale: within one float32 ulp of float32(max_norm / want) where want >
  max_norm, else exactly 1 (max_norm is half or twice a norm, never near it).
* parameters: optimizer_apply(p_prev, float32(g * scale_logged)) chained by
  the test over the steps of a learn(), bit for bit: opt_update is one shared
  device function, and the control test below establishes on the unclipped
  path that the chain reproduces the trainer exactly (measured on the parent
  commit as well: 0 ulp, every optimizer).

Run A (unclipped) and run B (clipped, same seed) share the rollout and the
value gradient bit for bit, so max_norm = half of A's value norm clips B's
value step by construction.  B's clipped value step changes the values, the
advantages and with them the first policy gradient in the last bits, so for
the policy the test asserts what the construction guarantees: the logged norm
is that of B's own buffer gradient and, at half of A's first-epoch norm, the
first epoch is clipped.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR_P, LR_V, WD_V = 1e-3, 1e-4, 1e-4
X0 = 90210


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b, what=""):
    np.testing.assert_array_equal(_u32(a), _u32(b), err_msg=what)


def _host_norm(g, r=1.0):
    t = np.asarray(g, np.float64).ravel()
    return math.sqrt(math.fsum((t * t).tolist())) * r


def _check_norm(dev, want, n, what):
    bound = (n + 8) * 2.0 ** -53 * want
    print("%s: norm device %.17g host %.17g err %.3g bound %.3g"
          % (what, dev, want, abs(dev - want), bound))
    assert abs(dev - want) <= bound, (what, dev, want, bound)


def _check_scale(dev, want_norm, max_norm, what):
    mx = np.float32(max_norm)
    want = (np.float32(np.float64(mx) / want_norm) if want_norm > np.float64(mx)
            else np.float32(1.0))
    print("%s: scale device %.9g host %.9g" % (what, dev, want))
    assert abs(np.float64(np.float32(dev)) - np.float64(want)) <= \
        np.float64(np.spacing(want)), (what, dev, want)
    assert np.float32(dev) == np.float64(dev), (what, "not a float32", dev)
    return want


# ------------------------------------------------ 1. the kernels alone ----
_VECTORS = {}


def _vector(n):
    """(g, host norm) of the seeded normal vector of n entries, made once."""
    if n not in _VECTORS:
        g = np.random.default_rng(1000 + n).normal(size=n).astype(np.float32)
        _VECTORS[n] = (g, _host_norm(g))
    return _VECTORS[n]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 8961, 17281,
                               2 ** 20 + 3])
def test_clip_grad_norm_kernels(ctx, n):
    """A partial wave, workgroup edges, the real nets' odd parameter counts
    and more partials than one pass of the summing wave holds."""
    from dependence_free_rl_amd import clip_grad_norm
    g, want = _vector(n)
    for factor in (0.5, 2.0):
        mx = float(np.float32(factor * want))
        out, norm, scale = clip_grad_norm(ctx, g, mx)
        what = "n=%d max=%.2f norm" % (n, factor)
        _check_norm(norm, want, n, what)
        _check_scale(scale, want, mx, what)
        assert (scale < 1) == (factor < 1), (what, scale)
        assert out.dtype == np.float32 and out.shape == g.shape
        _same_bits(out, g * np.float32(scale), what)
        out2, norm2, scale2 = clip_grad_norm(ctx, g, mx)
        assert (norm2, scale2) == (norm, scale), what
        _same_bits(out2, out, what + " (second call)")


def test_clip_grad_norm_zero_inf_nan(ctx):
    from dependence_free_rl_amd import XhError, clip_grad_norm
    z = np.zeros(300, np.float32)
    out, norm, scale = clip_grad_norm(ctx, z, 1.0)
    assert (norm, scale) == (0.0, 1.0)
    _same_bits(out, z)
    g = _vector(257)[0].copy()
    g[100] = np.inf
    out, norm, scale = clip_grad_norm(ctx, g, 1.0)
    assert norm == np.inf and scale == 0.0
    with np.errstate(invalid="ignore"):
        want = g * np.float32(0.0)
    assert np.isnan(out[100]) and np.isnan(want[100])
    keep = np.arange(g.size) != 100
    _same_bits(out[keep], want[keep])
    g[100] = np.nan
    out, norm, scale = clip_grad_norm(ctx, g, 1.0)
    assert np.isnan(norm) and scale == 1.0  # the comparison is false
    assert np.isnan(out[100])
    _same_bits(out[keep], g[keep])
    out, norm, scale = clip_grad_norm(ctx, np.zeros(0, np.float32), 1.0)
    assert out.size == 0 and (norm, scale) == (0.0, 1.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(XhError, match="status 1"):
            clip_grad_norm(ctx, z, bad)


# ------------------------------------------------ trainers and the chain ----
def _trainer(ctx, algo="ppo", B=8, D=2, N=16, T=4, widths=(128, 64),
             kind="adam", kind_v="sgd", **kw):
    from dependence_free_rl_amd import (POLICY, VALUE, Trainer, init_full_policy,
                                        init_policy, init_value)
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=widths, rng_state=X0, **kw)
    if algo == "pg":
        tr.set_params(POLICY, init_full_policy(B, D, widths, seed=21))
    else:
        tr.set_params(POLICY, init_policy(D, *widths, seed=21))
        tr.set_params(VALUE, init_value(B, D, seed=22))
        tr.set_optimizer(VALUE, kind_v, LR_V, WD_V if kind_v == "sgd" else 0.0)
    tr.set_optimizer(POLICY, kind, LR_P, WD_V if kind == "sgd" else 0.0)
    tr.kinds = (kind, kind_v)
    tr.has_value = algo != "pg"
    tr.rows = tr.T * tr.N
    return tr


class Chain:
    """The trainer's two optimizers restated with optimizer_apply: state and
    adam's step counter carried across learn() calls as the trainer's are."""

    def __init__(self, ctx, tr):
        from dependence_free_rl_amd import POLICY, VALUE
        self.ctx, self.tr = ctx, tr
        self.p = {POLICY: tr.params(POLICY)}
        if tr.has_value:
            self.p[VALUE] = tr.params(VALUE)
        self.m = {POLICY: None, VALUE: None}
        self.v = {POLICY: None, VALUE: None}
        self.t = {POLICY: 1, VALUE: 1}

    def _lr(self, lr):
        lr = np.float32(lr)
        if self.tr.cfg.lr_scale_rows:  # opt_step: (float)((double)lr / rows)
            lr = np.float32(np.float64(lr) / np.float64(self.tr.rows))
        return float(lr)

    def step(self, which, g, scale=None):
        from dependence_free_rl_amd import POLICY
        from dependence_free_rl_amd.trainer import optimizer_apply
        kind = self.tr.kinds[0 if which == POLICY else 1]
        lr = LR_P if which == POLICY else LR_V
        g = np.ascontiguousarray(g, np.float32)
        if scale is not None:
            assert np.float32(scale) == scale
            g = g * np.float32(scale)  # one float32 multiply per entry
        self.p[which], self.m[which], self.v[which] = optimizer_apply(
            self.ctx, kind, self.p[which], g, self._lr(lr),
            WD_V if kind == "sgd" else 0.0, t=float(self.t[which]),
            m=self.m[which], v=self.v[which])
        self.t[which] += 1


def _iteration(tr):
    """rollout + learn; the gradients the optimizers read and the result."""
    from dependence_free_rl_amd import POLICY, VALUE
    from dependence_free_rl_amd.trainer import BUF_POLICY_GRADS, BUF_VALUE_GRAD
    tr.rollout()
    tr.learn()
    rec = {"pg": tr.buffer(BUF_POLICY_GRADS), "p": tr.params(POLICY)}
    if tr.has_value:
        rec["vg"] = tr.buffer(BUF_VALUE_GRAD)
        rec["v"] = tr.params(VALUE)
    return rec


def _chain_iteration(chain, tr, rec, plog=None, vlog=None, what=""):
    """Advance the chain over one learn() (value step, then the policy
    epochs) and compare the parameters bit for bit."""
    from dependence_free_rl_amd import POLICY, VALUE
    if tr.has_value:
        chain.step(VALUE, rec["vg"], None if vlog is None else vlog[0, 1])
        _same_bits(rec["v"], chain.p[VALUE], what + " value parameters")
    for k, g in enumerate(rec["pg"]):
        chain.step(POLICY, g, None if plog is None else plog[k, 1])
    _same_bits(rec["p"], chain.p[POLICY], what + " policy parameters")


def _check_log(tr, log, grads, max_norm, what):
    """Every row of a clip log against the host norm of its buffer gradient."""
    r = 1.0 / tr.rows if tr.cfg.lr_scale_rows else 1.0
    assert log.shape == (len(grads), 2) and log.dtype == np.float64
    for k, g in enumerate(grads):
        want = _host_norm(g, r)
        _check_norm(log[k, 0], want, g.size, "%s step %d" % (what, k))
        _check_scale(log[k, 1], want, max_norm, "%s step %d" % (what, k))


# ------------------------------------------------- 2. control, clip off ----
def control_chain(ctx, kinds=(("adam", "sgd"),), iters=2):
    """The unclipped trainer against the optimizer_apply chain; returns the
    largest ulp distance seen (uses nothing this feature added, so it also
    runs against the parent commit's library)."""
    from dependence_free_rl_amd import POLICY, VALUE
    worst = 0
    for kind, kind_v in kinds:
        tr = _trainer(ctx, kind=kind, kind_v=kind_v)
        chain = Chain(ctx, tr)
        for it in range(iters):
            rec = _iteration(tr)
            chain.step(VALUE, rec["vg"])
            for g in rec["pg"]:
                chain.step(POLICY, g)
            for a, b in ((rec["v"], chain.p[VALUE]), (rec["p"], chain.p[POLICY])):
                d = np.abs(_u32(a).astype(np.int64) - _u32(b).astype(np.int64))
                worst = max(worst, int(d.max()))
            print("control %s/%s iteration %d: worst ulp distance %d"
                  % (kind, kind_v, it, worst))
        tr.close()
    return worst


def test_control_unclipped_chain_is_bit_exact(ctx):
    """PPO, B=8, D=2, N=16, T=4, widths (128, 64), adam for the policy and sgd
    with weight decay for the value net, 2 iterations: the chain of
    optimizer_apply calls over XH_BUF_VALUE_GRAD / XH_BUF_POLICY_GRADS gives
    the trainer's parameters bit for bit (0 ulp, also measured with the
    parent commit's library), the yardstick the clipped chains are held to."""
    assert control_chain(ctx) == 0


# ---------------------------------------------------- 3. clipped chain ----
def _run_a(ctx, **kw):
    """Run A, unclipped: one iteration's record and its host norms."""
    tr = _trainer(ctx, **kw)
    r = 1.0 / tr.rows if tr.cfg.lr_scale_rows else 1.0
    rec = _iteration(tr)
    rec["pnorms"] = [_host_norm(g, r) for g in rec["pg"]]
    if tr.has_value:
        rec["vnorm"] = _host_norm(rec["vg"], r)
    tr.close()
    return rec


def _clipped_run(ctx, a, what, iters=2, factor=0.5, **kw):
    """Run B on A's seed, both nets clipped at factor x A's first norms; every
    step's log and the parameter chain are checked.  Returns the trainer
    (open), its chain, the last record and the last logs."""
    from dependence_free_rl_amd import POLICY, VALUE
    tr = _trainer(ctx, **kw)
    pmax = float(np.float32(factor * a["pnorms"][0]))
    tr.set_grad_clip(POLICY, pmax)
    if tr.has_value:
        vmax = float(np.float32(factor * a["vnorm"]))
        tr.set_grad_clip(VALUE, vmax)
    chain = Chain(ctx, tr)
    rec = plog = vlog = None
    for it in range(iters):
        rec = _iteration(tr)
        plog = tr.grad_clip_log(POLICY)
        _check_log(tr, plog, rec["pg"], pmax, "%s it %d policy" % (what, it))
        if tr.has_value:
            vlog = tr.grad_clip_log(VALUE)
            _check_log(tr, vlog, [rec["vg"]], vmax, "%s it %d value" % (what, it))
        if it == 0 and factor < 1:
            assert plog[0, 1] < 1, (what, plog)
            if tr.has_value:
                _same_bits(rec["vg"], a["vg"], what + " value gradient")
                assert vlog[0, 1] < 1, (what, vlog)
        _chain_iteration(chain, tr, rec, plog, vlog, "%s it %d" % (what, it))
    return tr, chain, rec, plog, vlog


SHAPES = {"b8": dict(B=8, widths=(128, 64)),
          "b64": dict(B=64, widths=(128, 128), N=16)}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_clipped_chain(ctx, kind, shape):
    kw = dict(SHAPES[shape], kind=kind)
    a = _run_a(ctx, **kw)
    tr, _, _, _, _ = _clipped_run(ctx, a, "%s %s" % (kind, shape), **kw)
    tr.close()


def test_clipped_chain_lr_scale_rows(ctx):
    """norm = ||g|| / (T * N): the optimizer steps on the mean gradient."""
    kw = dict(SHAPES["b8"], kind="adam", lr_scale_rows=True)
    a = _run_a(ctx, **kw)
    assert a["pnorms"][0] == _host_norm(a["pg"][0]) / 64.0
    tr, _, _, _, _ = _clipped_run(ctx, a, "lr_scale_rows", **kw)
    tr.close()


# ---------------------------------------------------- 4. never clipped ----
def test_never_clipped_is_bit_identical(ctx):
    from dependence_free_rl_amd import POLICY, VALUE, _lib
    kw = dict(SHAPES["b8"], kind="adam")
    a = _run_a(ctx, **kw)
    top = 2.0 * max(a["pnorms"] + [a["vnorm"]])
    tr = _trainer(ctx, **kw)
    tr.set_stats(4)
    tr.set_grad_clip(POLICY, top)
    tr.set_grad_clip(VALUE, top)
    rec = _iteration(tr)
    for key in ("pg", "vg", "p", "v"):
        _same_bits(rec[key], a[key], key)
    plog, vlog = tr.grad_clip_log(POLICY), tr.grad_clip_log(VALUE)
    assert (plog[:, 1] == 1.0).all() and (vlog[:, 1] == 1.0).all()
    _check_log(tr, plog, rec["pg"], top, "never policy")
    _check_log(tr, vlog, [rec["vg"]], top, "never value")
    row = tr.stats()[0]
    assert row[_lib.STAT_PCLIP_STEPS] == 0
    assert row[_lib.STAT_PCLIP_SCALE_MIN] == 1 and row[_lib.STAT_VCLIP_SCALE] == 1
    tr.close()


# -------------------------------------------------------- 5. off again ----
def test_off_again(ctx):
    from dependence_free_rl_amd import POLICY, VALUE, XhError
    kw = dict(SHAPES["b8"], kind="adam")
    a = _run_a(ctx, **kw)
    tr, chain, _, _, _ = _clipped_run(ctx, a, "before off", iters=1, **kw)
    tr.set_grad_clip(POLICY, 0)
    tr.set_grad_clip(VALUE, 0)
    for which in (POLICY, VALUE):
        with pytest.raises(XhError, match="status 4"):
            tr.grad_clip_log(which)
    rec2 = _iteration(tr)
    _chain_iteration(chain, tr, rec2, None, None, "after off")
    # on again: no log until the next learn()
    tr.set_grad_clip(POLICY, 1.0)
    with pytest.raises(XhError, match="status 4"):
        tr.grad_clip_log(POLICY)
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(XhError, match="status 1"):
            tr.set_grad_clip(POLICY, bad)
    tr.close()


# --------------------------------------------------- 6. other learners ----
def test_actor_critic_clipped(ctx):
    kw = dict(algo="ac", B=8, N=16, T=8, widths=(64, 32), kind="momentum")
    a = _run_a(ctx, **kw)
    tr, _, rec, plog, vlog = _clipped_run(ctx, a, "ac", **kw)
    assert plog.shape == (tr.epochs, 2) == (1, 2) and vlog.shape == (1, 2)
    tr.close()


def test_klppo_clipped(ctx):
    from dependence_free_rl_amd.trainer import BUF_KL
    kw = dict(algo="klppo", B=64, N=16, T=4, widths=(128, 128), kind="adam")
    tr0 = _trainer(ctx, **kw)
    a = _iteration(tr0)
    kl_a = tr0.buffer(BUF_KL)
    tr0.close()
    a["pnorms"] = [_host_norm(g) for g in a["pg"]]
    a["vnorm"] = _host_norm(a["vg"])
    # the policy alone is clipped here, so the values, the advantages and the
    # first epoch (its gradient, its mean KL and the beta it sets) are run A's
    from dependence_free_rl_amd import POLICY
    tr = _trainer(ctx, **kw)
    pmax = float(np.float32(0.5 * a["pnorms"][0]))
    tr.set_grad_clip(POLICY, pmax)
    chain = Chain(ctx, tr)
    rec = _iteration(tr)
    plog = tr.grad_clip_log(POLICY)
    assert plog.shape == (tr.epochs, 2) and tr.epochs > 1
    _check_log(tr, plog, rec["pg"], pmax, "klppo policy")
    assert plog[0, 1] < 1
    _same_bits(rec["pg"][0], a["pg"][0], "klppo first gradient")
    _same_bits(rec["vg"], a["vg"])
    _same_bits(rec["v"], a["v"])
    _chain_iteration(chain, tr, rec, plog, None, "klppo")
    _same_bits(tr.buffer(BUF_KL)[0], kl_a[0], "klppo epoch 0 beta / KL")
    tr.close()
    # and both nets clipped, two iterations
    tr, _, _, _, _ = _clipped_run(ctx, a, "klppo both", **kw)
    tr.close()


def test_reinforce_clipped(ctx):
    from dependence_free_rl_amd import POLICY, VALUE, XhError
    kw = dict(algo="pg", B=8, D=2, N=8, T=1, widths=(64, 0), kind="adam")
    a = _run_a(ctx, **kw)
    tr, _, rec, plog, vlog = _clipped_run(ctx, a, "pg", **kw)
    assert plog.shape == (1, 2) and vlog is None
    _same_bits(_run_a(ctx, **kw)["pg"], a["pg"])
    with pytest.raises(XhError, match="status 1"):
        tr.set_grad_clip(VALUE, 1.0)
    tr.close()


# ------------------------------------------------ 7. communicator path ----
def test_one_rank_communicator(ctx):
    from dependence_free_rl_amd import Context
    kw = dict(SHAPES["b8"], kind="adam")
    a = _run_a(ctx, **kw)
    rc = Context(device=0, rank=0, world=1, uid=Context.unique_id())
    try:
        out = []
        for c in (ctx, rc):
            tr, _, rec, plog, vlog = _clipped_run(c, a, "comm", **kw)
            tr.set_timing(True)
            tr.iterate(1)
            out.append((rec, plog, vlog, tr.kernel_time("allreduce")[1]))
            tr.close()
        (r0, p0, v0, n0), (r1, p1, v1, n1) = out
        assert n0 == 0 and n1 == 1 + tr.epochs, (n0, n1)
        for key in ("pg", "vg", "p", "v"):
            _same_bits(r0[key], r1[key], key)
        np.testing.assert_array_equal(p0.view(np.uint64), p1.view(np.uint64))
        np.testing.assert_array_equal(v0.view(np.uint64), v1.view(np.uint64))
    finally:
        rc.close()


# ------------------------------------------------------- 8. statistics ----
def test_statistics_rows(ctx):
    from dependence_free_rl_amd import POLICY, VALUE, _lib
    from test_gpu_stats import EPS, _fsum
    kw = dict(SHAPES["b8"], kind="adam")
    a = _run_a(ctx, **kw)
    tr = _trainer(ctx, **kw)
    tr.set_stats(8)
    new = [_lib.STAT_PCLIP_STEPS, _lib.STAT_PCLIP_SCALE_MIN,
           _lib.STAT_VCLIP_SCALE]
    # iteration 0 is run A's: its value step and first epoch are clipped at
    # half of A's norms; the later steps as they come
    tr.set_grad_clip(POLICY, float(np.float32(0.5 * a["pnorms"][0])))
    tr.set_grad_clip(VALUE, float(np.float32(0.5 * a["vnorm"])))
    for it in range(3):
        rec = _iteration(tr)
        plog, vlog = tr.grad_clip_log(POLICY), tr.grad_clip_log(VALUE)
        row = tr.stats()[it]
        assert row[_lib.STAT_ITER] == it
        assert row[_lib.STAT_PCLIP_STEPS] == int((plog[:, 1] < 1).sum())
        assert row[[_lib.STAT_PCLIP_SCALE_MIN]].view(np.uint64)[0] == \
            plog[:, 1].min(keepdims=True).view(np.uint64)[0]
        assert row[[_lib.STAT_VCLIP_SCALE]].view(np.uint64)[0] == \
            vlog[0, 1:].view(np.uint64)[0]
        if it == 0:
            assert row[_lib.STAT_PCLIP_STEPS] >= 1
            assert row[_lib.STAT_PCLIP_SCALE_MIN] < 1
            assert row[_lib.STAT_VCLIP_SCALE] < 1
        # the gradient statistics stay those of the gradient as reduced
        g0 = rec["pg"][0].astype(np.float64)
        s, mag, n = _fsum(g0 * g0)
        err = abs(row[_lib.STAT_PGRAD_SQ_FIRST] - s)
        print("row %d PGRAD_SQ_FIRST err %.3g bound %.3g"
              % (it, err, (n + 8) * EPS * mag))
        assert err <= (n + 8) * EPS * mag
    # clipping off again: the three entries are NaN, the rest of the row is not
    tr.set_grad_clip(POLICY, 0)
    tr.set_grad_clip(VALUE, 0)
    _iteration(tr)
    row = tr.stats()[3]
    assert np.isnan(row[new]).all()
    assert np.isfinite(row[_lib.STAT_VERR_SUM:_lib.STAT_KL_BETA]).all()
    curve = tr.training_curve()
    np.testing.assert_array_equal(
        curve["policy_clip_fraction"][:3],
        tr.stats()[:3, _lib.STAT_PCLIP_STEPS] / tr.epochs)
    assert np.isnan(curve["policy_clip_fraction"][3])
    assert curve["value_clip_scale"][0] < 1
    assert curve["policy_clip_scale_min"][0] < 1
    # a window forget() consumes: the learner part stays NaN, the new entries
    # included
    tr.rollout()
    tr.forget()
    row = tr.stats()[4]
    assert row[_lib.STAT_ITER] == 4
    assert np.isnan(row[_lib.STAT_VERR_SUM:]).all() and row.size == 21
    tr.close()


# ----------------------------------------------------- 9. launch count ----
PHASES = ("rollout_step", "value", "policy_train", "reduce_sgd", "kl", "stats",
          "allreduce")


def _launches(tr):
    tr.reset_timing()
    tr.learn()
    tr.synchronize()
    return {p: tr.kernel_time(p)[1] for p in PHASES}


def test_launch_count(ctx):
    from dependence_free_rl_amd import POLICY, VALUE
    tr = _trainer(ctx, **dict(SHAPES["b8"], kind="adam"))
    tr.set_timing(True)
    tr.rollout()
    before = _launches(tr)
    tr.set_grad_clip(POLICY, 1e-3)
    tr.set_grad_clip(VALUE, 1e-3)
    tr.rollout()
    on = _launches(tr)
    tr.set_grad_clip(POLICY, 0)
    tr.set_grad_clip(VALUE, 0)
    tr.rollout()
    off = _launches(tr)
    print("launches before", before, "clip on", on, "clip off", off)
    assert off == before
    assert before["reduce_sgd"] == tr.epochs + 1
    extra = sum(on.values()) - sum(off.values())
    assert 0 < extra <= 2 * (tr.epochs + 1), (on, off)
    assert {k: v for k, v in on.items() if k != "reduce_sgd"} == \
        {k: v for k, v in off.items() if k != "reduce_sgd"}
    tr.close()
