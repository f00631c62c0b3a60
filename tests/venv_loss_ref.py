"""Host restatement of xh_venv_policy_loss (include/xylo_hip.h), np.float32
operation by operation -- numpy rounds every f32 operation once and fuses
nothing -- and the inputs the CPU and GPU tests share.  CPU only.

  grad_f32            both losses on given p (probabilities, or the softmax of
                      the logits), the one-hot Jacobian form for logits, the
                      skipped rows and the scale
  jacobian_full_f32   softmax_layer::backward's full (linear - quadratic)
                      matrix times a backprop row (nn.h:403-414)
  dvalue_f32          square_loss_grad (nn.h:548-550) times value_scale
  stats_f64           the XH_VLOSS_* row in float64, summed with math.fsum
  clipped_inputs      the clipped-loss test inputs of a shape
"""
import math

import numpy as np

f32 = np.float32
U32 = 2.0 ** -24
EPS = 0.2
(ROWS, SKIPPED, LOGR_SUM, LOGR_SQSUM, K3_SUM, CLIPPED, SURR_SUM, ENTROPY_SUM,
 VERR_SUM, VERR_SQSUM, COUNT) = range(11)
# (bins, dims, envs) of the GPU tests, T recorded steps each
CASES = [(8, 2, 19), (32, 1, 70), (64, 2, 40), (128, 3, 5), (16, 3, 9)]
T = 4
RATIOS = (0.5, 0.79, 0.81, 0.95, 1.0, 1.05, 1.19, 1.21, 2.0)


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def clip_bounds(eps):
    """1.0f + eps and 1.0f - eps as the kernel forms them (f32)."""
    return f32(1) + f32(eps), f32(1) - f32(eps)


def d_clipped_f32(p_ch, q_old, A, eps):
    """clipped_gradient's entry at the choice (rl.h:54-74)."""
    hi, lo = clip_bounds(eps)
    with np.errstate(all="ignore"):
        ratio = p_ch / q_old
        clipped = np.where(ratio > hi, hi, np.where(ratio < lo, lo, ratio))
        x, y = clipped * A, ratio * A
        imp = np.where(y < x, y, x) * f32(-1)
        d = imp / p_ch
    assert d.dtype == f32
    return d


def d_clipped_f64(p_ch, q_old, A, eps):
    """The same in float64 (the bounds are the kernel's f32 values)."""
    hi, lo = (float(b) for b in clip_bounds(eps))
    p_ch, q_old, A = (np.asarray(a, np.float64) for a in (p_ch, q_old, A))
    ratio = p_ch / q_old
    clipped = np.clip(ratio, lo, hi)
    return -np.minimum(clipped * A, ratio * A) / p_ch


def grad_f32(p, ch, q_old, A, kind, loss, eps=EPS, scale=1.0):
    """grad [n][B] from p [n][B] f32: kind "probs" | "logits" (p = the softmax
    of the logits), loss "log" | "clipped"."""
    p = np.ascontiguousarray(p, f32)
    q_old, A = np.asarray(q_old, f32), np.asarray(A, f32)
    n, B = p.shape
    rows = np.arange(n)
    hot = np.zeros((n, B), bool)
    hot[rows, ch] = True
    p_ch = p[rows, ch]
    if loss == "log":
        g = p * A[:, None]
        g[rows, ch] = g[rows, ch] - A
    else:
        d = d_clipped_f32(p_ch, q_old, A, eps)[:, None]
        if kind == "probs":
            g = np.where(hot, d, f32(0))
        else:
            quad = p * p_ch[:, None]
            pd = np.where(hot, p, f32(0)) - quad
            with np.errstate(all="ignore"):
                g = pd * d
    with np.errstate(all="ignore"):
        g = g * f32(scale)
    g[~(q_old > 0)] = 0
    assert g.dtype == f32
    return g


def jacobian_full_f32(p, bp):
    """result[j] = sum_k (linear - quadratic)[j][k] bp[k], the sum from 0.0f
    in k order, every operation in f32 (nn.h:403-414) for one row."""
    p, bp = np.asarray(p, f32), np.asarray(bp, f32)
    quad = p[:, None] * p[None, :]
    pd = np.diag(p) - quad
    acc = np.zeros(len(p), f32)
    for k in range(len(p)):
        acc = acc + pd[:, k] * bp[k]
    assert acc.dtype == f32
    return acc


def dvalue_f32(values_new, target_q, value_scale, q_old):
    dv = np.asarray(values_new, f32) - np.asarray(target_q, f32)
    out = dv * f32(value_scale)
    out[~(np.asarray(q_old, f32) > 0)] = 0
    return out, dv


def stats_f64(p, ch, q_old, A, eps, dv=None):
    """(the XH_VLOSS_* row, sum |log ratio|) over the rows with q_old > 0."""
    p = np.ascontiguousarray(p, f32)
    hi, lo = clip_bounds(eps)
    t = {k: [] for k in (LOGR_SUM, LOGR_SQSUM, K3_SUM, CLIPPED, SURR_SUM,
                         ENTROPY_SUM, VERR_SUM, VERR_SQSUM)}
    out = np.zeros(COUNT)
    for i in range(len(p)):
        if not q_old[i] > 0:
            out[SKIPPED] += 1
            continue
        out[ROWS] += 1
        pn, po, a = f32(p[i, ch[i]]), f32(q_old[i]), f32(A[i])
        r = pn / po
        c = hi if r > hi else lo if r < lo else r
        x, y = c * a, r * a
        logr = math.log(float(pn)) - math.log(float(po))
        t[CLIPPED].append(float(r > hi or r < lo))
        t[SURR_SUM].append(float(y if y < x else x))
        t[LOGR_SUM].append(logr)
        t[LOGR_SQSUM].append(logr * logr)
        t[K3_SUM].append((float(pn) / float(po) - 1.0) - logr)
        t[ENTROPY_SUM].extend(-float(v) * math.log(float(v))
                              for v in p[i] if v > 0)
        if dv is not None:
            t[VERR_SUM].append(float(dv[i]))
            t[VERR_SQSUM].append(float(dv[i]) * float(dv[i]))
    for k, v in t.items():
        out[k] = math.fsum(v)
    return out, math.fsum(abs(v) for v in t[LOGR_SUM])


# ---------------------------------------------------------------- inputs --
def clipped_inputs(case, total=None):
    """The clipped-loss inputs of a shape, `total` rows (T * N by default):
    logits z [total][B] f32, probs = f32(softmax64(z)), the taken bins ch (of
    probability below 0.45, so p_old stays a probability), p_old = p_ch /
    ratio with the target ratios of RATIOS and advantages of both signs with
    0.25 <= |A| <= 2, the 18 (ratio, sign) pairs dealt round-robin over a
    seeded permutation of the rows."""
    B, D, N = case
    n = total or T * N
    g = np.random.default_rng(1000 * B + n)
    z = (g.standard_normal((n, B)) * 2.0).astype(f32)
    p64 = softmax64(z)
    ch = g.integers(0, B, n)
    rows = np.arange(n)
    ch = np.where(p64[rows, ch] > 0.45, p64.argmin(axis=1), ch).astype(np.int32)
    combo = np.zeros(n, int)
    combo[g.permutation(n)] = (rows + int(g.integers(0, 18))) % 18
    ratio = np.array(RATIOS)[combo % 9]
    sign = np.where(combo >= 9, -1.0, 1.0)
    p_old = (p64[rows, ch] / ratio).astype(f32)
    adv = (sign * g.uniform(0.25, 2.0, n)).astype(f32)
    return {"z": z, "probs": p64.astype(f32), "p64": p64, "ch": ch,
            "p_old": p_old, "adv": adv, "ratio": ratio}


def regimes(p_ch, q_old, A, eps=EPS):
    """0 .. 5 per row: (below, inside, above the clip range) x (A > 0, A < 0)."""
    hi, lo = (float(b) for b in clip_bounds(eps))
    r = np.asarray(p_ch, np.float64) / np.asarray(q_old, np.float64)
    return np.where(r < lo, 0, np.where(r > hi, 2, 1)) * 2 + (np.asarray(A) < 0)


def excluded_rows(p_ch, q_old, A, eps=EPS):
    """The rows a float64 comparison of the clipped loss must leave out: the
    ratio within 1e-5 of a clip boundary (f32 and float64 may take different
    branches), or the min's two arguments different but nearly tied."""
    hi, lo = (float(b) for b in clip_bounds(eps))
    p_ch, q_old, A = (np.asarray(a, np.float64) for a in (p_ch, q_old, A))
    r = p_ch / q_old
    edge = (np.abs(r - hi) < 1e-5) | (np.abs(r - lo) < 1e-5)
    c = np.clip(r, lo, hi)
    x, y = c * A, r * A
    tie = (c != r) & (np.abs(x - y) <= 1e-5 * np.maximum(np.abs(x), np.abs(y)))
    return edge | tie
