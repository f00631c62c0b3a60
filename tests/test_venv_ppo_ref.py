"""Pins tests/venv_ppo_ref.py, the host restatement of xh_venv_policy_loss_
ex's entropy bonus and clipped value loss, against things that are not the
kernel restated: central differences of -c H, the row-sum identity, float64,
and the piecewise gradient of 0.5 max(...).  CPU only."""
import functools

import numpy as np
import pytest

import venv_loss_ref as vr
import venv_ppo_ref as pr

f32 = np.float32
SETS = [(c, None) for c in vr.CASES] + [(vr.CASES[0], 600), (vr.CASES[4], 72)]
SET_IDS = ["B%d-n%s" % (c[0], n or vr.T * c[2]) for c, n in SETS]
COEFS = (0.01, 0.37)


@functools.lru_cache(maxsize=None)
def _probs(sel):
    """f32 probabilities of a shape, [n][B]: the f32 softmax of clipped_inputs'
    logits, every 7th row with three bins at -inf (exact zeros, as a masked
    row has) and every 11th row with one legal bin only (p = 1, 0, ...)."""
    z = vr.clipped_inputs(*sel)["z"].copy()
    n, B = z.shape
    g = np.random.default_rng(5 * B + n)
    for r in range(0, n, 7):
        z[r, g.choice(B, 3, replace=False)] = -np.inf
    for r in range(3, n, 11):
        keep = int(g.integers(0, B))
        z[r, np.arange(B) != keep] = -np.inf
        z[r, keep] = 0
    e = np.exp(z - z.max(axis=1, keepdims=True), dtype=f32)
    p = (e / e.sum(axis=1, keepdims=True, dtype=f32)).astype(f32)
    assert (p == 0).any() and (p == 1).any() and np.isfinite(p).all()
    p.setflags(write=False)
    return p


# --------------------------------------------------------------- entropy --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("B", [8, 16])
def test_float64_gradient_against_central_differences(B, kind):
    """d/dx of -c H(softmax(x)) (logits) and of -c H(x) (probabilities,
    unconstrained) by central differences with step 1e-6, within 1e-7 c max(1,
    max |g|): the truncation (h^2 f''' / 6, about 1e-10 here) and the
    roundoff (1e-16 / h) are orders of magnitude below that."""
    g = np.random.default_rng(B)
    h = 1e-6
    worst = 0.0
    for c in COEFS:
        for _ in range(4):
            if kind == "logits":
                x = g.standard_normal(B) * 2.0
                p = vr.softmax64(x)
            else:
                x = g.uniform(0.05, 1.0, B)   # not normalised: no constraint
                p = x
            want, _ = pr.entropy_grad_f64(p[None, :], c, kind)
            fd = np.zeros(B)
            for k in range(B):
                d = np.zeros(B)
                d[k] = h
                fd[k] = (pr.neg_entropy_f64(x + d, c, kind) -
                         pr.neg_entropy_f64(x - d, c, kind)) / (2 * h)
            tol = 1e-7 * c * max(1.0, np.abs(want).max())
            worst = max(worst, np.abs(fd - want[0]).max() / tol)
            assert np.all(np.abs(fd - want[0]) <= tol)
    print("B=%d %s: max |fd - g64| / tol = %.3g" % (B, kind, worst))


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_logits_form_sums_to_zero_and_meets_its_bound(sel):
    """On every shape, rows with exact zeros included: the f32 restatement is
    within (B + 8) 2^-24 c p_k (|log p_k| + H) of float64, entries at p_k == 0
    are exact zeros, a one-bin row is all zeros, and each row of the logits
    form sums to 0 within the sum of its entries' bounds."""
    p = _probs(sel)
    B = p.shape[1]
    for c in COEFS:
        e, S = pr.entropy_grad_f32(p, c, "logits")
        e64, H = pr.entropy_grad_f64(p, c, "logits")
        bound = pr.entropy_bound(p, c, "logits")
        err = np.abs(e.astype(np.float64) - e64)
        ratio = (err / np.where(bound > 0, bound, 1.0)).max()
        print("B=%d c=%g: max |e - e64| / bound = %.4f; max |S + H| / ((B+1) u"
              " H) = %.4f" % (B, c, ratio, (np.abs(S + H) / np.where(
                  H > 0, (B + 1) * pr.U32 * H, 1.0)).max()))
        assert np.all(err <= bound)
        assert not e[p == 0].any()
        one = (p == 1).any(axis=1)
        assert one.any() and not e[one].any()
        assert np.all(np.abs(S + H) <= (B + 1) * pr.U32 * H)
        assert np.all(np.abs(e.astype(np.float64).sum(axis=1)) <=
                      bound.sum(axis=1))
        assert np.all(np.abs(e64.sum(axis=1)) <= 1e-6 * c)


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_probs_form_meets_its_bound(sel):
    """|e - e64| <= 4 2^-24 c (|log p_k| + 1); entries at p_k == 0 are 0."""
    p = _probs(sel)
    for c in COEFS:
        e, _ = pr.entropy_grad_f32(p, c, "probs")
        e64, _ = pr.entropy_grad_f64(p, c, "probs")
        bound = pr.entropy_bound(p, c, "probs")
        err = np.abs(e.astype(np.float64) - e64)
        print("B=%d c=%g: max |e - e64| / bound = %.4f"
              % (p.shape[1], c, (err / np.where(bound > 0, bound, 1.0)).max()))
        assert np.all(err <= bound)
        assert not e[p == 0].any()


def test_row_sum_order_is_the_lanes_then_the_butterfly():
    """row_sum_f32 on 128 bins equals the order written out by hand: eight
    lanes of 16 bins each, added in bin order, then ((0+1)+(2+3)) +
    ((4+5)+(6+7)) -- the xor butterfly's tree as lane 0 sees it."""
    p = _probs((vr.CASES[3], None))
    S, l = pr.row_sum_f32(p)
    with np.errstate(invalid="ignore"):
        t = p * l   # NaN where p_k == 0: never added
    for r in (0, 1, 5, 7):
        lane = []
        for i in range(8):
            s = f32(0)
            for k in range(16):
                if p[r, 16 * i + k] > 0:
                    s = f32(s + t[r, 16 * i + k])
            lane.append(s)
        a = [f32(lane[0] + lane[1]), f32(lane[2] + lane[3]),
             f32(lane[4] + lane[5]), f32(lane[6] + lane[7])]
        want = f32(f32(a[0] + a[1]) + f32(a[2] + a[3]))
        assert want.view(np.uint32) == S[r].view(np.uint32)


# ------------------------------------------------------------ value clip --
def _classify(vn, tg, vo):
    """2 * regime + (dl < 0) from the values alone, in float64."""
    vn, tg, vo = (np.asarray(a, np.float64) for a in (vn, tg, vo))
    dl = vn - vo
    vc = vo + np.clip(dl, -pr.VCLIP, pr.VCLIP)
    s1, s2 = (vn - tg) ** 2, (vc - tg) ** 2
    reg = np.where(np.abs(dl) < pr.VCLIP, pr.INSIDE,
                   np.where(np.abs(dl) == pr.VCLIP, pr.BOUNDARY,
                            np.where(s2 > s1, pr.ZEROED,
                                     np.where(s2 < s1, pr.KEPT, pr.TIE))))
    return 2 * reg + (dl < 0)


@pytest.mark.parametrize("sel", SETS, ids=SET_IDS)
def test_value_clip_is_the_piecewise_gradient(sel):
    """Every shape's rows hold each regime in both signs; on these binary
    fractions every f32 operation is exact, and the f32 restatement equals
    the float64 gradient of 0.5 max((v - tg)^2, (v_clip - tg)^2) exactly, at
    value_scale 1 and 0.5."""
    case, n = sel
    n = n or vr.T * case[2]
    inp = pr.vclip_inputs(n)
    vn, tg, vo = inp["vn"], inp["tg"], inp["vo"]
    got = _classify(vn, tg, vo)
    np.testing.assert_array_equal(got, inp["regime"])
    assert sorted(set(got.tolist())) == list(range(10))
    for a in (vn, tg, vo):
        assert np.all(a * 64 == np.round(a * 64)) and np.abs(a).max() < 16
    want = pr.vclip_f64(vn, tg, vo, pr.VCLIP)
    for scale in (1.0, 0.5):
        dval, zero, e1, e2 = pr.vclip_f32(vn, tg, vo, pr.VCLIP, scale)
        np.testing.assert_array_equal(dval.astype(np.float64), want * scale)
        np.testing.assert_array_equal(zero, got // 2 == pr.ZEROED)
    assert np.array_equal(e1.astype(np.float64),
                          vn.astype(np.float64) - tg.astype(np.float64))
    # a kept row keeps the plain gradient, a zeroed one an exact zero
    plain, _ = vr.dvalue_f32(vn, tg, 1.0, np.ones(n, f32))
    dval, zero, _, _ = pr.vclip_f32(vn, tg, vo, pr.VCLIP, 1.0)
    assert np.array_equal(dval[~zero], plain[~zero]) and not dval[zero].any()
    # ... and a NaN is not masked
    nan = pr.vclip_f32([np.nan, 1.0], [0.0, 0.0], [0.0, np.nan], pr.VCLIP,
                       1.0)[0]
    assert np.isnan(nan[0]) and nan[1] == 1.0


def test_ext_stats_reference():
    inp = pr.vclip_inputs(76)
    q_old = np.ones(76, f32)
    q_old[5] = 0
    p = _probs((vr.CASES[0], None))
    st = pr.ext_stats_f64(p, q_old, True, inp["vn"], inp["tg"], inp["vo"])
    assert st[pr.ROWS] == 75 and 0 < st[pr.VCLIP_ROWS] < 75
    assert st[pr.ENTROPY_SUM] > 0 and st[pr.VLOSS_SUM] * 4096 % 1 == 0
    off = pr.ext_stats_f64(p, q_old, False)
    assert off.tolist() == [75, 0, 0, 0]
