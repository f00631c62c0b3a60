"""Host restatements of the KL-PPO side of the VecEnv chain (include/
xylo_hip.h: XH_LOSS_KL_REGULATED and kl_stats of xh_venv_policy_loss,
xh_venv_kl_beta), np.float32 operation by operation -- numpy rounds every f32
operation once and fuses nothing.  CPU only.

  kl_grad_f32    the KL-regulated gradient in the header's operation order
  row_kl_f64     per row KL(q || p) = sum_k q_k (log q_k - log p_k) in float64,
                 a term with q_k == 0 being 0, and sum_k |term|
  kl_stats_f64   the XH_VKL_* row over the counted rows, and sum |terms|
  beta_rule_f32  kl_beta_kernel's rule: (beta before, d, beta after)
  kl_inputs      a shape's sampling distributions q for the KL tests
"""
import math

import numpy as np

import venv_loss_ref as vr

f32 = np.float32
KL_SUM, ROWS, KL_SQSUM, COUNT = range(4)
BETA_MIN, BETA_MAX = f32(1e-25), f32(0.1)


def kl_grad_f32(p, q, ch, q_old, A, beta, scale=1.0):
    """v = p_k * A; v[ch] = v[ch] - A; reg = (p_k - q_k) * beta; v = v + reg;
    grad = v * scale; zeros where q_old <= 0 or NaN (a skipped row)."""
    p, q = np.ascontiguousarray(p, f32), np.ascontiguousarray(q, f32)
    q_old, A = np.asarray(q_old, f32), np.asarray(A, f32)
    rows = np.arange(len(p))
    with np.errstate(all="ignore"):
        v = p * A[:, None]
        v[rows, ch] = v[rows, ch] - A
        reg = (p - q) * f32(beta)
        v = v + reg
        g = v * f32(scale)
    g[~(q_old > 0)] = 0
    assert g.dtype == f32
    return g


def row_kl_f64(p, q):
    """(KL [n], sum_k |term| [n]) in float64; a term with q_k == 0 is 0 and
    nothing else is masked (p_k == 0 < q_k gives +inf)."""
    p64 = np.asarray(p, f32).astype(np.float64)
    q64 = np.asarray(q, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        term = q64 * (np.log(q64) - np.log(p64))
    term = np.where(q64 == 0, 0.0, term)
    kl = np.array([math.fsum(r) for r in term])
    return kl, np.abs(term).sum(axis=1)


def kl_stats_f64(p, q, q_old):
    """(the XH_VKL_* row, sum |terms|) over the rows with q_old > 0."""
    keep = np.asarray(q_old, f32) > 0
    kl, mag = row_kl_f64(np.asarray(p)[keep], np.asarray(q)[keep])
    out = np.zeros(COUNT)
    out[KL_SUM] = math.fsum(kl)
    out[ROWS] = keep.sum()
    out[KL_SQSUM] = math.fsum(k * k for k in kl)
    return out, math.fsum(mag)


def beta_rule_f32(kl_sum, rows, d_targ, beta):
    """d = (float)(kl_sum / rows); beta halves where |d| < d_targ / 1.5f,
    doubles where |d| > d_targ * 1.5f, then fmaxf(., 1e-25f), fminf(., 0.1f).
    A NaN d compares false twice.  Returns (beta, d, beta after) as f32."""
    with np.errstate(all="ignore"):
        d = f32(np.float64(kl_sum) / np.float64(rows))
        b0 = f32(beta)
        b = b0
        if abs(d) < f32(d_targ) / f32(1.5):
            b = b / f32(2)
        elif abs(d) > f32(d_targ) * f32(1.5):
            b = b * f32(2)
        b = np.fmax(b, BETA_MIN)
        b = np.fmin(b, BETA_MAX)
    return b0, d, f32(b)


def kl_inputs(sel):
    """The sampling distributions q [n][B] f32 of a shape's clipped_inputs:
    the softmax (f32, max shift) of the logits plus a perturbation of standard
    deviation 0.3, with exact zeros: every 7th row has logits pushed 200 below
    the row's maximum in three bins (expf underflows to 0.0f) and every 5th
    row has one entry set to zero outright (q then sums to a little less than
    1, as a recorded row may)."""
    inp = vr.clipped_inputs(*sel)
    n, B = inp["z"].shape
    g = np.random.default_rng(77 * B + n)
    zq = inp["z"] + (g.standard_normal((n, B)) * 0.3).astype(f32)
    for r in range(0, n, 7):
        zq[r, g.choice(B, 3, replace=False)] -= f32(200)
    e = np.exp(zq - zq.max(axis=1, keepdims=True), dtype=f32)
    q = (e / e.sum(axis=1, keepdims=True, dtype=f32)).astype(f32)
    for r in range(0, n, 5):
        q[r, int(g.integers(0, B))] = 0
    assert (q == 0).sum() >= n // 5 and (q >= 0).all()
    return q
