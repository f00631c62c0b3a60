"""Host restatement of xh_venv_policy_loss_ex's two terms (include/
xylo_hip.h), np.float32 operation by operation -- numpy rounds every f32
operation once and fuses nothing -- their float64 forms, and the inputs the CPU
and GPU tests share.  CPU only.

  row_sum_f32         S = sum_k p_k log p_k as the kernel adds it: 16 bins per
                      lane in bin order (all 8 at 8 bins), the lanes' sums by
                      the xor butterfly (partners 1, 2, 4)
  entropy_grad_f32    e [n][B] and S [n] of a batch of rows, both kinds
  entropy_grad_f64    the same gradient in float64, with H [n]
  neg_entropy_f64     -c H(softmax(z)) / -c H(p), what the gradients are of
  entropy_bound       the bound of |f32 - float64| (derived below)
  vclip_f32           the clipped value loss's dvalue, zero, e1, e2
  vclip_f64           the piecewise gradient of 0.5 max((v - tg)^2, (vc - tg)^2)
  vclip_inputs        binary-fraction value inputs with every regime
  ext_stats_f64       the XH_VEXT_* row

The logarithm is numpy's f32 log here and logf on the device: both within one
ulp, not the same bits, so the device's entropy term is compared with float64
within entropy_bound and not with entropy_grad_f32 bit for bit.

The bound.  With u = 2^-24, l_k = log p_k, H = -S >= 0, every f32 operation
within (1 + u): l_k carries |l_k| u (logf within an ulp -- counted as one
rounding), t_k = p_k l_k one more, the sum of B terms of one sign B - 1
roundings on S, so |dS| <= (B + 1) u H.  d = l_k - S: |dd| <= |l_k| u + (B +
1) u H + (|l_k| + H) u; e = p_k d and e c two more roundings of (|l_k| + H).
To first order |de| <= (4 |l_k| + (B + 4) H) u c p_k; counting three roundings
on t_k instead gives (5 |l_k| + (B + 5) H) u c p_k, and (B + 8) u c p_k (|l_k|
+ H) covers both.  For probabilities d = l_k + 1 and e = d c: |de| <=
(|l_k| + 2 (|l_k| + 1)) u c <= 4 u c (|l_k| + 1) to first order (3 of the 4).
"""
import math

import numpy as np

f32 = np.float32
U32 = 2.0 ** -24
ROWS, ENTROPY_SUM, VCLIP_ROWS, VLOSS_SUM, COUNT = range(5)
VCLIP = 0.25
# the value-clip regimes: (inside, boundary, zeroed, kept, tie) x (dl > 0, < 0)
INSIDE, BOUNDARY, ZEROED, KEPT, TIE = range(5)


def lanes(B):
    """(bins per lane, lanes per row) of the kernels' layout."""
    bpl = min(16, B)
    return bpl, B // bpl


def row_sum_f32(p):
    """(S [n] f32, l [n][B] f32): l_k = log(p_k), t_k = p_k * l_k, the lane's
    t_k with p_k > 0 added from 0.0f in bin order, the lanes' sums by the xor
    butterfly.  Every lane ends with the same bits; lane 0's are returned."""
    p = np.ascontiguousarray(p, f32)
    n, B = p.shape
    bpl, lpe = lanes(B)
    with np.errstate(all="ignore"):
        l = np.log(p)
        t = p * l
    assert l.dtype == f32 and t.dtype == f32
    pl, tl = p.reshape(n, lpe, bpl), t.reshape(n, lpe, bpl)
    s = np.zeros((n, lpe), f32)
    for k in range(bpl):
        with np.errstate(all="ignore"):
            s = np.where(pl[:, :, k] > 0, s + tl[:, :, k], s)
    o = 1
    while o < lpe:
        s = s + s[:, np.arange(lpe) ^ o]
        o *= 2
    assert s.dtype == f32
    assert all((s[:, i].view(np.uint32) == s[:, 0].view(np.uint32)).all()
               for i in range(lpe))
    return s[:, 0].copy(), l


def entropy_grad_f32(p, c, kind):
    """(e [n][B], S [n]) f32.  "logits": d = l_k - S; e = p_k * d; e = e * c.
    "probs": d = l_k + 1.0f; e = d * c.  e = 0 where p_k == 0, by a select."""
    p = np.ascontiguousarray(p, f32)
    S, l = row_sum_f32(p)
    c = f32(c)
    with np.errstate(all="ignore"):
        if kind == "logits":
            d = l - S[:, None]
            e = p * d
            e = e * c
        else:
            d = l + f32(1)
            e = d * c
    e = np.where(p > 0, e, f32(0))
    assert e.dtype == f32
    return e, S


def entropy_grad_f64(p, c, kind):
    """(e64 [n][B], H [n]) on p as given, in float64: "logits" c p_k (log p_k
    + H), the gradient of -c H(softmax(z)) in z; "probs" c (log p_k + 1), the
    unconstrained partial of -c H(p).  0 where p_k == 0."""
    p = np.asarray(p).astype(np.float64)
    with np.errstate(all="ignore"):
        l = np.log(p)
    t = np.where(p > 0, p * np.where(p > 0, l, 0.0), 0.0)
    H = -np.array([math.fsum(r) for r in t])
    with np.errstate(all="ignore"):
        if kind == "logits":
            e = float(c) * p * (l + H[:, None])
        else:
            e = float(c) * (l + 1.0)
    return np.where(p > 0, e, 0.0), H


def neg_entropy_f64(x, c, kind):
    """-c H of one row in float64: of softmax(x) under "logits", of x itself
    (no constraint) under "probs".  0 log 0 = 0."""
    x = np.asarray(x, np.float64)
    if kind == "logits":
        e = np.exp(x - x.max())
        x = e / e.sum()
    return float(c) * math.fsum(v * math.log(v) for v in x if v > 0)


def entropy_bound(p, c, kind):
    """[n][B]: (B + 8) u c p_k (|log p_k| + H) for logits, 4 u c (|log p_k| +
    1) for probabilities; 0 where p_k == 0 (the entry is exactly 0)."""
    p = np.asarray(p).astype(np.float64)
    B = p.shape[1]
    _, H = entropy_grad_f64(p, 1.0, kind)
    with np.errstate(all="ignore"):
        al = np.abs(np.log(p))
    al = np.where(p > 0, al, 0.0)
    if kind == "logits":
        out = (B + 8) * U32 * float(c) * p * (al + H[:, None])
    else:
        out = 4 * U32 * float(c) * (al + 1.0)
    return np.where(p > 0, out, 0.0)


# ------------------------------------------------------ clipped value loss --
def vclip_f32(vn, tg, vo, vclip, value_scale, q_old=None):
    """(dvalue, zero, e1, e2), every operation in f32 in the header's order;
    dvalue is 0 on a skipped row (q_old <= 0 or NaN) too."""
    vn, tg, vo = (np.asarray(a, f32) for a in (vn, tg, vo))
    vc_ = f32(vclip)
    with np.errstate(all="ignore"):
        dl = vn - vo
        hit = (dl > vc_) | (dl < -vc_)
        vc = vo + np.where(dl > vc_, vc_, -vc_)
        e1 = vn - tg
        e2 = vc - tg
        s1, s2 = e1 * e1, e2 * e2
        zero = hit & (s2 > s1)
        out = np.where(zero, f32(0), e1 * f32(value_scale))
    if q_old is not None:
        out = np.where(np.asarray(q_old, f32) > 0, out, f32(0))
    assert out.dtype == f32 and e1.dtype == f32 and e2.dtype == f32
    return out, zero, e1, e2


def vclip_f64(vn, tg, vo, vclip):
    """d/dv of 0.5 max((v - tg)^2, (v_clip - tg)^2), v_clip = vo + clamp(v -
    vo, -vclip, vclip), in float64: v - tg, but 0 where the clip is hit (v_clip
    constant in v) and the clipped square is strictly the larger."""
    vn, tg, vo = (np.asarray(a, np.float64) for a in (vn, tg, vo))
    vc = vo + np.clip(vn - vo, -float(vclip), float(vclip))
    a, b = (vn - tg) ** 2, (vc - tg) ** 2
    return np.where((vc != vn) & (b > a), 0.0, vn - tg)


def vclip_inputs(n, seed=0):
    """Values of n rows, all multiples of 1/64 below 16 in magnitude, for
    vclip = 0.25 -- every operation of vclip_f32 on them is exact.  The ten
    (regime, sign) pairs are dealt round-robin over a seeded permutation of the
    rows.  With s = the sign of dl = vn - vo, m >= 0 a multiple of 1/64:
      INSIDE    |dl| < 0.25, tg free
      BOUNDARY  |dl| == 0.25, tg free (not a hit: kept)
      ZEROED    |dl| > 0.25, tg = vn + s m beyond vn: |vc - tg| > |vn - tg|
      KEPT      |dl| > 0.25, tg = vc - s m before vc: |vc - tg| < |vn - tg|
      TIE       |dl| - 0.25 an even number of 64ths, tg midway between vc and
                vn: the two squares are equal (kept)
    Returns {"vn", "tg", "vo"} f32 [n] and "regime" [n] = 2 * regime + (dl <
    0)."""
    g = np.random.default_rng(9000 + 31 * n + seed)
    combo = np.zeros(n, int)
    combo[g.permutation(n)] = (np.arange(n) + int(g.integers(0, 10))) % 10
    reg, neg = combo // 2, combo % 2
    s = np.where(neg == 1, -1, 1)
    vo = g.integers(-256, 257, n)                      # in 64ths
    over = g.integers(1, 65, n)                        # |dl| - 16, outside
    over = np.where(reg == TIE, 2 * ((over + 1) // 2), over)
    mag = np.where(reg == INSIDE, g.integers(0, 16, n),
                   np.where(reg == BOUNDARY, 16, 16 + over))
    mag = np.where((reg == INSIDE) & (mag == 0) & (neg == 1), 1, mag)
    vn = vo + s * mag
    vc = vo + s * 16
    m = g.integers(0, 129, n)
    tg = g.integers(-256, 257, n)
    tg = np.where(reg == ZEROED, vn + s * m, tg)
    tg = np.where(reg == KEPT, vc - s * m, tg)
    tg = np.where(reg == TIE, (vc + vn) // 2, tg)
    out = {k: (v / 64.0).astype(f32) for k, v in
           (("vn", vn), ("tg", tg), ("vo", vo))}
    out["regime"] = combo
    return out


def ext_stats_f64(p, q_old, ent_on, vn=None, tg=None, vo=None, vclip=VCLIP):
    """The XH_VEXT_* row over the rows with q_old > 0: ENTROPY_SUM the fsum of
    the float64 entropies of p (0 without the bonus), VCLIP_ROWS and VLOSS_SUM
    from vclip_f32's zero, e1 and e2 (0 without the value head; vo None: no
    clipping)."""
    keep = np.asarray(q_old, f32) > 0
    out = np.zeros(COUNT)
    out[ROWS] = keep.sum()
    if ent_on:
        _, H = entropy_grad_f64(np.asarray(p)[keep], 1.0, "probs")
        out[ENTROPY_SUM] = math.fsum(H)
    if vn is not None:
        if vo is None:
            e1 = np.asarray(vn, f32) - np.asarray(tg, f32)
            zero, e2 = np.zeros(len(e1), bool), e1
        else:
            _, zero, e1, e2 = vclip_f32(vn, tg, vo, vclip, 1.0)
        out[VCLIP_ROWS] = (zero & keep).sum()
        sq = np.where(zero, e2.astype(np.float64) ** 2,
                      e1.astype(np.float64) ** 2)
        out[VLOSS_SUM] = math.fsum(sq[keep])
    return out
