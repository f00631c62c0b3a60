"""PPO update diagnostics (xh_trainer_set_update_diag) on the device: the
per-row records of the extra forward (p_new, entropy, KL) and the ring row of
their sums, for both kernel forms (policy_diag_kernel, f32 MFMA;
policy_diag_split_kernel, f16 pairs).

What is held to what:

* a no-op update (lr_policy = 0): p_new against XH_BUF_POLD at the project's
  figure for two forwards of the same math (rtol 2e-6, atol 1e-7,
  tests/test_gpu_scale.py), no row clipped, |LOGR_SUM| <= rows * 2.1e-6, every
  KL record within 2 (2e-6 + B 1e-7) (the first-order term |sum_b (q_b - p_b)|
  under that rule), the entropy record against -sum q log q of XH_BUF_QOLD;
* a moved policy against the CPU oracle's forward on the device trainer's own
  parameters, with the yardstick measured in the same run on the rollout (code
  the diagnostics do not touch): g_logp = max |log POLD - log p_oracle[a]|,
  g_H = max |H(QOLD) - H(p_oracle)|, and for the KL records g_logq = max over
  bins |log QOLD_b - log p_oracle_b| (KL = sum q log q - sum q log p', so its
  error is at most the largest per-bin log-probability error: the per-bin
  form of g_logp); every deviation <= 4 max(g, 2e-6);
* every floating entry of the ring row against math.fsum of the xh_diag.h
  terms restated in numpy on the device's own records, XH_BUF_POLD and
  XH_BUF_ADV: |device - host| <= (n + 8) 2^-52 fsum|terms| (the derived bound
  of tests/test_gpu_stats.py); LEARN, ROWS and CLIPPED equal.

The learning rates of the moved-policy cases were chosen on the CPU with the
oracle's Trainer alone (warm-up iterations at the default rate, then one
learn() at the rate below) so that 33% - 54% of the rows leave [0.8, 1.2] and
at most one row lies within 1e-4 of a clip boundary (the device reproduced
the oracle's fractions: 54%, 42%, 43%, 33%); the device's own fraction is
asserted to stay within 5% - 95%.
"""
import math

import numpy as np
import pytest

from conftest import log_record

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CLIP = 0.2


def _trainer(ctx, algo="ppo", B=8, D=2, widths=(128, 64), N=24, T=3, seed=31,
             x0=4242, **kw):
    from dependence_free_rl_amd import POLICY, VALUE, Trainer, init_policy, init_value
    tr = Trainer(ctx, algo=algo, bins=B, dims=D, num_envs=N, steps=T,
                 widths=widths, rng_state=x0, clip_eps=CLIP, **kw)
    tr.set_params(POLICY, init_policy(D, *widths, seed=seed))
    tr.set_params(VALUE, init_value(B, D, seed=seed + 1))
    return tr


def _fsum(terms):
    t = np.asarray(terms, np.float64).ravel().tolist()
    return math.fsum(t), math.fsum(abs(x) for x in t), len(t)


def _terms(p_new, pold, adv, eps=CLIP):
    """xh_diag.h in numpy: np.float32 for the f32 steps, float64 logs."""
    pn = np.asarray(p_new, np.float32).ravel()
    po_ = np.asarray(pold, np.float32).ravel()
    A = np.asarray(adv, np.float32).ravel()
    hi = np.float32(1.0) + np.float32(eps)
    lo = np.float32(1.0) - np.float32(eps)
    with np.errstate(all="ignore"):
        r = (pn / po_).astype(np.float32)
        above, below = r > hi, r < lo
        c = np.where(above, hi, np.where(below, lo, r)).astype(np.float32)
        x, y = (c * A).astype(np.float32), (r * A).astype(np.float32)
        surr = np.where(y < x, y, x).astype(np.float64)
        pn64, po64 = pn.astype(np.float64), po_.astype(np.float64)
        logr = np.log(pn64) - np.log(po64)
        return {"r32": r, "clipped": (above | below).astype(np.float64),
                "surr": surr, "logr": logr, "logr2": logr * logr,
                "k3": (pn64 / po64 - 1.0) - logr}


def _check_sums(tr, row, learn, what):
    """The ring row against the numpy restatement on the device's records."""
    from dependence_free_rl_amd import _lib as L
    from dependence_free_rl_amd.trainer import BUF_ADV, BUF_POLD
    rec = tr.update_diag_rows()
    t = _terms(rec["p_new"], tr.buffer(BUF_POLD), tr.buffer(BUF_ADV))
    n = tr.T * tr.N
    assert row[L.UPD_LEARN] == learn, what
    assert row[L.UPD_ROWS] == n, what
    assert row[L.UPD_CLIPPED] == t["clipped"].sum(), what
    out = {}
    for idx, name, terms in ((L.UPD_LOGR_SUM, "logr", t["logr"]),
                             (L.UPD_LOGR_SQSUM, "logr2", t["logr2"]),
                             (L.UPD_K3_SUM, "k3", t["k3"]),
                             (L.UPD_SURR_SUM, "surr", t["surr"]),
                             (L.UPD_ENTROPY_SUM, "entropy", rec["entropy"]),
                             (L.UPD_KL_SUM, "kl", rec["kl"])):
        s, mag, cnt = _fsum(terms)
        dev = float(row[idx])
        out[name] = {"device": dev, "host": s, "bound": (cnt + 8) * EPS * mag}
        print(what, name, out[name])
        if math.isnan(s):
            assert math.isnan(dev), (what, name, dev)
        else:
            assert abs(dev - s) <= (cnt + 8) * EPS * mag, (what, name, dev, s, mag)
    return rec, t, out


def _entropy(p):
    """-sum p log p over the last axis in float64, terms 0 where p == 0; and
    the sum of |terms|."""
    p = np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(axis=-1), np.abs(t).sum(axis=-1)


def _kl(q, p):
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    with np.errstate(all="ignore"):
        t = np.where(q > 0, q * (np.log(q) - np.log(p)), 0.0)
    return t.sum(axis=-1)


# ------------------------------------ 1: a no-op update, every kernel form --
NOOP = [
    # kernel form, B, D, widths, N
    ("f32", 8, 2, (128, 64), 24),
    ("f32", 8, 2, (128, 64), 8),      # one group
    ("f32", 16, 2, (64, 64), 12),
    ("f32", 32, 1, (64, 64), 6),
    ("f32", 64, 2, (128, 128), 5),
    ("f32", 128, 3, (128, 128), 3),
    ("split", 64, 2, (128, 128), 13),  # more than one workgroup's 12 waves
    ("split", 32, 1, (64, 64), 6),
]


@pytest.mark.parametrize("form,B,D,widths,N", NOOP)
def test_noop_update_every_kernel_form(ctx, monkeypatch, form, B, D, widths, N):
    from dependence_free_rl_amd import _lib as L
    from dependence_free_rl_amd.trainer import BUF_POLD, BUF_QOLD
    if form == "f32":
        monkeypatch.setenv("XH_ROLLOUT_KERNEL", "4")
    else:
        monkeypatch.delenv("XH_ROLLOUT_KERNEL", raising=False)
    T = 3
    what = "noop %s B%d D%d N%d" % (form, B, D, N)
    tr = _trainer(ctx, "ppo", B, D, widths, N, T, lr_policy=0.0, wd_policy=0.0,
                  record_distrib=True)
    tr.set_update_diag(4)
    tr.rollout()
    tr.learn()
    info = tr.update_diag_info()
    assert info["kernel"] == ("policy_diag_kernel" if form == "f32"
                              else "policy_diag_split_kernel"), info
    assert info["math"] == ("f32_mfma" if form == "f32" else "f16_pair"), info
    assert info["kl_source"] == "qold" and info["history_rows"] == 4
    assert info["every"] == 1
    row = tr.update_diag()[0]
    rec, t, sums = _check_sums(tr, row, 0, what)
    pold, q = tr.buffer(BUF_POLD), tr.buffer(BUF_QOLD).astype(np.float64)
    differing = int((rec["p_new"] != pold).sum())
    # the p_new record: the rollout's p_old to the last place
    np.testing.assert_allclose(rec["p_new"], pold, rtol=2e-6, atol=1e-7,
                               err_msg=what)
    # the ring row
    assert row[L.UPD_CLIPPED] == 0.0, what
    assert abs(row[L.UPD_LOGR_SUM]) <= T * N * 2.1e-6, (what, row[L.UPD_LOGR_SUM])
    # the per-row KL and entropy records
    kl_max = float(np.abs(rec["kl"]).max())
    assert kl_max <= 2 * (2e-6 + B * 1e-7), (what, kl_max)
    h, hmag = _entropy(q)
    with np.errstate(all="ignore"):
        lq = np.where(q > 0, np.abs(np.log(q)), 0.0)
    bound = ((B + 8) * EPS * hmag + 2e-6 * (q * (1 + lq)).sum(axis=-1) +
             B * 1e-7 * (1 + lq.max(axis=-1)))
    herr = np.abs(rec["entropy"] - h)
    assert (herr <= bound).all(), (what, float((herr / bound).max()))
    log_record("update_diag.jsonl", {
        "what": what, "kernel": info["kernel"], "rows": T * N,
        "p_new_rows_differing_from_pold": differing, "kl_abs_max": kl_max,
        "entropy_err_over_bound_max": float((herr / bound).max()),
        "logr_sum": float(row[L.UPD_LOGR_SUM])})
    tr.close()


# ------------------------------------ 2: a moved policy against the oracle --
# algo, B, D, widths, N, warm-up iterations, the learn()'s policy rate
MOVED = [
    ("ppo", 8, 2, (128, 64), 24, 4, 0.05),
    ("ac", 8, 2, (128, 64), 24, 4, 0.02),
    ("klppo", 8, 2, (128, 64), 24, 4, 0.2),
    ("ppo", 64, 2, (128, 128), 6, 6, 0.03),
]


def _oracle_probs(tr, params):
    """The oracle's forward of `params` over the batch's T*N observations
    [bins / 8, item / 8], as [T][N][B] float64."""
    from oracle import pyoracle as po
    from dependence_free_rl_amd.trainer import BUF_BINS, BUF_ITEMS
    T, N, B, D = tr.T, tr.N, tr.B, tr.D
    bins = tr.buffer(BUF_BINS)[:T].astype(np.float32) / 8.0      # [T][N][B][D]
    items = tr.buffer(BUF_ITEMS)[:T, :, :D].astype(np.float32) / 8.0
    obs = np.concatenate(
        [bins, np.broadcast_to(items[:, :, None, :], bins.shape)], axis=-1)
    widths = [tr.cfg.policy_h1, tr.cfg.policy_h2]
    p = po.model_eval(po.perbin_model(2 * D, widths, po.OR_SOFTMAX), params,
                      obs.reshape(T * N, B * 2 * D))
    return p.reshape(T, N, B).astype(np.float64)


def _moved_check(tr, what, pre_params):
    """After the probed learn(): the records against the oracle, with the
    yardsticks from the rollout under pre_params."""
    from dependence_free_rl_amd import POLICY
    from dependence_free_rl_amd.trainer import BUF_ACTION, BUF_POLD, BUF_QOLD
    T, N = tr.T, tr.N
    row = tr.update_diag()[-1]
    rec, t, sums = _check_sums(tr, row, row[0], what)
    a = tr.buffer(BUF_ACTION)
    pold = tr.buffer(BUF_POLD)
    q = tr.buffer(BUF_QOLD).astype(np.float64)
    tt, nn = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    p0 = _oracle_probs(tr, pre_params)
    p1 = _oracle_probs(tr, tr.params(POLICY))
    # the yardsticks: the rollout's own deviation from the oracle
    g_logp = float(np.abs(np.log(pold.astype(np.float64)) -
                          np.log(p0[tt, nn, a])).max())
    g_h = float(np.abs(_entropy(q)[0] - _entropy(p0)[0]).max())
    with np.errstate(all="ignore"):
        g_logq = float(np.where(q > 0, np.abs(np.log(q) - np.log(p0)), 0.0).max())
    d_logp = float(np.abs(np.log(rec["p_new"].astype(np.float64)) -
                          np.log(p1[tt, nn, a])).max())
    d_h = float(np.abs(rec["entropy"] - _entropy(p1)[0]).max())
    d_kl = float(np.abs(rec["kl"] - _kl(q, p1)).max())
    # clip decisions against the oracle's ratio on the same p_old
    r_orc = (p1[tt, nn, a].astype(np.float32) / pold).astype(np.float32)
    hi, lo = np.float32(1) + np.float32(CLIP), np.float32(1) - np.float32(CLIP)
    c_orc = (r_orc > hi) | (r_orc < lo)
    c_dev = t["clipped"].reshape(T, N) > 0
    near = np.abs(np.abs(r_orc.astype(np.float64) - 1.0) - CLIP) < 1e-4
    frac = float(c_dev.mean())
    recd = {"what": what, "kernel": tr.update_diag_info()["kernel"],
            "g_logp": g_logp, "g_H": g_h, "g_logq": g_logq, "d_logp": d_logp,
            "d_H": d_h, "d_KL": d_kl, "clip_fraction": frac,
            "near_boundary_rows": int(near.sum()),
            "clip_mismatches": int((c_orc != c_dev).sum())}
    print(recd)
    log_record("update_diag.jsonl", recd)
    assert 0.05 <= frac <= 0.95, (what, frac)
    assert d_logp <= 4 * max(g_logp, 2e-6), (what, d_logp, g_logp)
    assert d_h <= 4 * max(g_h, 2e-6), (what, d_h, g_h)
    assert d_kl <= 4 * max(g_logq, 2e-6), (what, d_kl, g_logq)
    assert not ((c_orc != c_dev) & ~near).any(), what
    assert near.sum() <= 0.01 * T * N + 1, (what, int(near.sum()))
    return row


@pytest.mark.parametrize("algo,B,D,widths,N,warm,lr", MOVED)
def test_moved_policy_against_the_oracle(ctx, algo, B, D, widths, N, warm, lr):
    from dependence_free_rl_amd import POLICY
    from dependence_free_rl_amd import _lib as L
    what = "moved %s B%d" % (algo, B)
    tr = _trainer(ctx, algo, B, D, widths, N, 3, record_distrib=True)
    tr.iterate(warm)
    tr.set_learning_rate(POLICY, lr)
    tr.set_update_diag(2)
    tr.rollout()
    pre = tr.params(POLICY)
    tr.learn()
    info = tr.update_diag_info()
    assert info["kernel"] == ("policy_diag_split_kernel" if B == 64
                              else "policy_diag_kernel"), info
    assert info["kl_source"] == "qold", info
    row = _moved_check(tr, what, pre)
    assert np.isfinite(row).all(), row
    assert row[L.UPD_K3_SUM] > 0 and row[L.UPD_KL_SUM] > 0, row
    c = tr.update_curve()
    assert c["clip_fraction"][-1] == row[L.UPD_CLIPPED] / row[L.UPD_ROWS]
    assert c["approx_kl"][-1] == -row[L.UPD_LOGR_SUM] / row[L.UPD_ROWS]
    assert c["approx_kl_k2"][-1] == row[L.UPD_LOGR_SQSUM] / (2 * row[L.UPD_ROWS])
    assert c["entropy"][-1] == row[L.UPD_ENTROPY_SUM] / row[L.UPD_ROWS]
    tr.close()


# ------------------------------------------- 3: where the KL comes from -----
def test_kl_is_nan_without_recorded_distributions(ctx):
    """PPO at 8 bins without record_distrib: no distributions exist, the KL
    records and KL_SUM are NaN, every other entry is finite."""
    from dependence_free_rl_amd import POLICY
    from dependence_free_rl_amd import _lib as L
    tr = _trainer(ctx, "ppo", 8, 2, (128, 64), 24, 3)
    tr.iterate(4)
    tr.set_learning_rate(POLICY, 0.05)
    tr.set_update_diag(2)
    tr.iterate(1)
    assert tr.update_diag_info()["kl_source"] is None
    row = tr.update_diag()[0]
    rec, _, _ = _check_sums(tr, row, 0, "ppo B8 no distributions")
    assert np.isnan(rec["kl"]).all() and math.isnan(row[L.UPD_KL_SUM])
    assert np.isfinite(np.delete(row, L.UPD_KL_SUM)).all(), row
    assert math.isnan(tr.update_curve()["kl"][0])
    tr.close()


def test_kl_from_the_epoch0_distributions_at_64_bins(ctx):
    """PPO at 64 bins without record_distrib: the KL reads the distributions
    the rollout left for epoch 0 (valid when the learn() began).  With
    record_distrib the same values sit in XH_BUF_QOLD, so the two trainers'
    records are bit-identical."""
    from dependence_free_rl_amd import POLICY
    from dependence_free_rl_amd import _lib as L
    got = []
    for rd in (False, True):
        tr = _trainer(ctx, "ppo", 64, 2, (128, 128), 6, 3, record_distrib=rd)
        tr.iterate(6)
        tr.set_learning_rate(POLICY, 0.03)
        tr.set_update_diag(2)
        tr.iterate(1)
        info = tr.update_diag_info()
        assert info["kl_source"] == ("qold" if rd else "e0_p"), info
        assert info["kernel"] == "policy_diag_split_kernel", info
        row = tr.update_diag()[0]
        rec, _, _ = _check_sums(tr, row, 0, "ppo B64 record_distrib=%s" % rd)
        assert np.isfinite(row).all() and row[L.UPD_KL_SUM] > 0, row
        got.append((row, rec))
        tr.close()
    np.testing.assert_array_equal(got[0][0], got[1][0])
    for k in ("p_new", "entropy", "kl"):
        np.testing.assert_array_equal(got[0][1][k], got[1][1][k], err_msg=k)


# ------------------------------------------------ 4: changes nothing else ---
PHASES = ("rollout_step", "policy_train", "value", "reduce_sgd", "allreduce",
          "stats", "kl")


@pytest.mark.parametrize("algo,B,D,widths,N", [("ppo", 64, 2, (128, 128), 6),
                                               ("klppo", 8, 2, (128, 64), 24)])
def test_diagnostics_change_nothing_else(ctx, algo, B, D, widths, N):
    from dependence_free_rl_amd import POLICY, VALUE
    from dependence_free_rl_amd import _lib as L
    out = []
    for on in (False, True):
        tr = _trainer(ctx, algo, B, D, widths, N, 3, record_last_step=True)
        tr.set_stats(8)
        tr.set_timing(True)
        if on:
            tr.set_update_diag(8)
        tr.iterate(3)
        bufs = {b: tr.buffer(b).copy() for b in range(18)
                if L.lib.xh_trainer_buffer_bytes(tr.h, b) > 0}
        times = {p: tr.kernel_time(p)[1] for p in PHASES + ("probe",)}
        out.append((tr.params(POLICY), tr.params(VALUE), bufs, tr.stats(), times))
        if on:
            assert tr.update_diag_count() == 3
        tr.close()
    off, on = out
    np.testing.assert_array_equal(off[0].view(np.uint32), on[0].view(np.uint32))
    np.testing.assert_array_equal(off[1].view(np.uint32), on[1].view(np.uint32))
    assert off[2].keys() == on[2].keys() and len(off[2]) >= 15
    for b in off[2]:
        np.testing.assert_array_equal(off[2][b].view(np.uint8),
                                      on[2][b].view(np.uint8), err_msg=str(b))
    np.testing.assert_array_equal(off[3].view(np.uint64), on[3].view(np.uint64))
    for p in PHASES:
        assert off[4][p] == on[4][p], (p, off[4], on[4])
    assert off[4]["probe"] == 0 and on[4]["probe"] == 3 * 3, (off[4], on[4])


# ------------------------------------------------ 5: ring, every, async -----
def test_ring_every_and_async_reads(ctx):
    from dependence_free_rl_amd import XhError
    from dependence_free_rl_amd import _lib as L
    tr = _trainer(ctx, "ppo", 8, 2, (128, 64), 24, 3)
    tr.set_update_diag(4, every=2)
    tr.iterate(7)
    assert tr.update_diag_count() == 4
    rows = tr.update_diag()
    assert rows.shape == (4, L.UPD_COUNT)
    assert rows[:, L.UPD_LEARN].tolist() == [0.0, 2.0, 4.0, 6.0]
    assert (rows[:, L.UPD_ROWS] == 72).all()
    # the same run read after every iteration
    t2 = _trainer(ctx, "ppo", 8, 2, (128, 64), 24, 3)
    t2.set_update_diag(4, every=2)
    seen = []
    for i in range(7):
        t2.iterate(1)
        if i % 2 == 0:
            seen.append(t2.update_diag(t2.update_diag_count() - 1, 1)[0])
    np.testing.assert_array_equal(np.array(seen).view(np.uint64),
                                  rows.view(np.uint64))
    t2.close()
    # two more learns: a fifth row overwrites row 0
    tr.iterate(2)
    assert tr.update_diag_count() == 5
    with pytest.raises(XhError, match="status 1"):  # overwritten
        tr.update_diag(0, 1)
    with pytest.raises(XhError, match="status 1"):  # not written yet
        tr.update_diag(5, 1)
    with pytest.raises(XhError, match="status 1"):
        tr.update_diag(3, 3)
    assert tr.update_diag()[:, L.UPD_LEARN].tolist() == [2.0, 4.0, 6.0, 8.0]
    np.testing.assert_array_equal(tr.update_diag(1, 3).view(np.uint64),
                                  rows[1:].view(np.uint64))
    n = tr.T * tr.N  # a wrong n for the records
    buf = np.zeros(n + 1, np.float32)
    assert L.lib.xh_trainer_get_update_diag_rows(
        tr.h, buf.ctypes.data, None, None, n + 1) == L.XH_ERR_INVALID
    assert L.lib.xh_trainer_get_update_diag_rows(
        tr.h, buf.ctypes.data, None, None, n) == L.XH_OK
    # off, then on again: the counters restart; forget() is no learn()
    tr.set_update_diag(0)
    with pytest.raises(XhError, match="status 4"):  # XH_ERR_STATE
        tr.update_diag_count()
    tr.iterate(1)
    tr.set_update_diag(4, every=2)
    assert tr.update_diag_count() == 0
    tr.rollout()
    tr.forget()
    tr.iterate(1)            # learn 0: probed
    assert tr.update_diag_count() == 1
    tr.rollout()
    tr.forget()
    tr.iterate(1)            # learn 1: not probed
    assert tr.update_diag_count() == 1
    tr.iterate(1)            # learn 2: probed
    assert tr.update_diag()[:, L.UPD_LEARN].tolist() == [0.0, 2.0]
    tr.close()


# ---------------------------------------------------------------- 6: edges --
def test_wide_slot_runs_the_f32_form(ctx):
    """A slot 0 holding a bin below -capacity at 64 bins: the f32 form runs
    (as the f32 rollout and train kernels do), and its records meet the
    moved-policy limits."""
    from dependence_free_rl_amd import POLICY
    tr = _trainer(ctx, "ppo", 64, 2, (128, 128), 6, 3, record_distrib=True)
    tr.iterate(6)
    tr.set_learning_rate(POLICY, 0.03)
    tr.set_update_diag(2)
    bins, items = tr.env_state()
    bins[1, 7, 0] = -20
    bins[4, 0, :] = -128
    tr.set_env_state(0, bins, items)
    tr.rollout()
    pre = tr.params(POLICY)
    tr.learn()
    info = tr.update_diag_info()
    assert info["kernel"] == "policy_diag_kernel" and info["math"] == "f32_mfma", info
    _moved_check(tr, "wide slot 0, B64", pre)
    tr.iterate(1)  # states >= 0 again: back on the f16-pair form
    assert tr.update_diag_info()["kernel"] == "policy_diag_split_kernel"
    tr.close()


def test_refusals_and_state_errors(ctx):
    from dependence_free_rl_amd import Trainer, XhError
    from dependence_free_rl_amd import _lib as L
    pg = Trainer(ctx, algo="pg", bins=8, dims=2, num_envs=8, steps=1,
                 widths=(32, 0))
    with pytest.raises(XhError, match="status 1"):  # XH_ERR_INVALID
        pg.set_update_diag(8)
    pg.close()
    tr = _trainer(ctx, "ppo", 8, 2, (128, 64), 8, 3)
    row = np.zeros(L.UPD_COUNT)
    n = L.C.c_long(-1)
    buf = L.C.create_string_buffer(256)
    # off: every reader is a state error
    assert L.lib.xh_trainer_update_diag_count(tr.h, L.C.byref(n)) == L.XH_ERR_STATE
    assert L.lib.xh_trainer_get_update_diag(tr.h, 0, 1, row.ctypes.data) == L.XH_ERR_STATE
    assert L.lib.xh_trainer_get_update_diag_rows(tr.h, None, None, None, 24) == L.XH_ERR_STATE
    assert L.lib.xh_trainer_update_diag_info(tr.h, buf, 256) == L.XH_ERR_STATE
    for bad in ((-1, 1), (8, 0), (8, -2), ((1 << 20) + 1, 1)):
        with pytest.raises(XhError, match="status 1"):
            tr.set_update_diag(*bad)
    # on, before any learn(): the rows and records are a state error
    tr.set_update_diag(8)
    assert tr.update_diag_count() == 0
    assert tr.update_diag_info()["kernel"] is None
    assert L.lib.xh_trainer_get_update_diag(tr.h, 0, 1, row.ctypes.data) == L.XH_ERR_STATE
    assert L.lib.xh_trainer_get_update_diag(tr.h, 0, 0, None) == L.XH_ERR_STATE
    assert L.lib.xh_trainer_get_update_diag_rows(tr.h, None, None, None, 24) == L.XH_ERR_STATE
    tr.rollout()
    assert L.lib.xh_trainer_get_update_diag(tr.h, 0, 1, row.ctypes.data) == L.XH_ERR_STATE
    tr.learn()
    assert tr.update_diag().shape == (1, L.UPD_COUNT)
    tr.close()


def test_one_rank_communicator_and_two_runs_are_identical(ctx):
    from dependence_free_rl_amd import Context
    rc = Context(device=0, rank=0, world=1, uid=Context.unique_id())
    try:
        out = []
        for c in (ctx, rc, ctx):
            tr = _trainer(c, "ppo", 8, 2, (128, 64), 24, 3, record_distrib=True)
            tr.set_update_diag(4)
            tr.set_timing(True)
            tr.iterate(3)
            out.append((tr.update_diag(), tr.update_diag_rows(),
                        tr.kernel_time("allreduce")[1]))
            tr.close()
        for other in out[1:]:
            np.testing.assert_array_equal(out[0][0].view(np.uint64),
                                          other[0].view(np.uint64))
            for k in ("p_new", "entropy", "kl"):
                np.testing.assert_array_equal(out[0][1][k], other[1][k], err_msg=k)
        # the communicator's run made one more all-reduce per probed learn
        assert out[0][2] == 0 and out[1][2] > 0
    finally:
        rc.close()
