"""Logit tables for VecEnv learners (xh_venv_table_*, venv_table_kernels.hip)
on the GPU against tests/venv_table_ref.py: the table's observations, the act
on a table against the act on the reference's gathered rows (bit for bit, all
of the act's records), the act through a PolicyNet, the gather, the exact
entry sum of the gradient, the table backward within the per-row path's
budget, and the refusals of out-of-domain states."""
import json

import numpy as np
import pytest

import venv_net_ref as nref
import venv_table_ref as tr
from conftest import assert_grad_units, grad_units
from venv_items_ref import DEFAULT_ITEMS

pytestmark = pytest.mark.gpu

CAP57 = ([(3, 1), (2, 2), (1, 4)], (5, 7))
# 16 items at capacity 8 in three dims: 11664 entries, past the sum kernel's
# LDS form (4096)
BIG = ([(1 + k % 8, 1 + k // 8, 1) for k in range(16)], (8, 8, 8))
# (B, D, N, set): 5 envs at 8 bins leave a partial wave, 37 span workgroups
SHAPES = [(8, 1, 5, None), (16, 3, 37, None), (64, 2, 37, None),
          (128, 3, 3, None), (8, 2, 37, CAP57)]
SUM_SHAPES = SHAPES + [(8, 3, 5, BIG)]
_ids = lambda s: "B%dD%dN%d%s" % (s[0], s[1], s[2],  # noqa: E731
                                  "" if s[3] is None else "set")


def _domain(D, iset):
    if iset is None:
        return tr.Domain(DEFAULT_ITEMS[D], 8, D)
    return tr.Domain(iset[0], iset[1], D)


def _venv(ctx, B, D, N, iset, seed=11, **kw):
    from dependence_free_rl_amd import VecEnv
    if iset is None:
        return VecEnv(ctx, N, bins=B, dims=D, rng_state=seed, **kw)
    return VecEnv(ctx, N, bins=B, dims=D, rng_state=seed, items=iset[0],
                  capacity=iset[1], **kw)


def _table(m, B, seed=0):
    """A random-valued table [R * B] (the padding too: it is never read)."""
    rng = np.random.default_rng(seed)
    return (2.0 * rng.standard_normal(m.rows(B) * B)).astype(np.float32)


def _state(v):
    from dependence_free_rl_amd._lib import VENV_BINS, VENV_ITEMS
    return v.get(VENV_BINS), v.get(VENV_ITEMS)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), what)


def _same_venvs(a, b, ep):
    """Every buffer and record of two venvs, bit for bit."""
    from dependence_free_rl_amd import _lib
    for which in (_lib.VENV_ACTIONS, _lib.VENV_PCHOICE, _lib.VENV_REWARD,
                  _lib.VENV_DONE, _lib.VENV_BINS, _lib.VENV_ITEMS,
                  _lib.VENV_RNG, _lib.VENV_OBS):
        _same(a.get(which), b.get(which), "buffer %d" % which)
    ra, rb = a.record(), b.record()
    assert sorted(ra) == sorted(rb)
    for k in ra:
        _same(ra[k], rb[k], "record " + k)
    if ep:
        a.episode_row()
        b.episode_row()
        _same(a.episode_stats(), b.episode_stats(), "episode rows")
        for x, y in zip(a.episode_state(), b.episode_state()):
            _same(x, y, "episode state")
    return ra


# ---- 1. the observations -----------------------------------------------------
@pytest.mark.parametrize("shape", SUM_SHAPES, ids=_ids)
def test_table_obs_is_the_references(ctx, shape):
    B, D, N, iset = shape
    m = _domain(D, iset)
    v = _venv(ctx, B, D, N, iset)
    info = v.table_info()
    assert (info["entries"], info["states"], info["items"], info["rows"]) == \
        (m.E, m.S, m.K, m.rows(B))
    assert np.array_equal(info["side"], m.side)
    _same(v.table_obs(), m.table_obs(B), "table obs")
    v.close()


# ---- 2. act_table against act on the gathered rows ---------------------------
@pytest.mark.parametrize("flags", range(8),
                         ids=lambda f: "mask%d_ep%d_rd%d" % (f & 1, f >> 1 & 1,
                                                              f >> 2 & 1))
@pytest.mark.parametrize("mode", ["sample", "argmax"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_act_table_is_act_on_the_gathered_rows(ctx, shape, mode, flags):
    B, D, N, iset = shape
    mask, ep, rd = bool(flags & 1), bool(flags & 2), bool(flags & 4)
    m = _domain(D, iset)
    table = _table(m, B, seed=B + D)
    steps = 40
    a, b = (_venv(ctx, B, D, N, iset) for _ in range(2))
    for v in (a, b):
        v.set_record(steps, states=True, distrib=rd)
        v.set_action_mask(mask)
        if ep:
            v.set_episode_stats(4)
    tptr = a._scratch("t", table.nbytes)
    a._upload(tptr, table)
    for _ in range(steps):
        bins, items = _state(b)
        rows, live = m.gather(table, bins, items)
        assert live.all()
        a.act_table(tptr, mode=mode, write_obs=True)
        b.act(rows, kind="logits", mode=mode, write_obs=True, fetch=False)
    a.synchronize()
    b.synchronize()
    rec = _same_venvs(a, b, ep)
    assert rec["action"].shape == (steps, N)
    assert sorted(rec) == sorted(["action", "pchoice", "reward", "done",
                                  "bins", "items"] + ["distrib"] * rd +
                                 ["legal"] * mask)
    if B == 8:
        assert rec["done"].any()  # envs were reset on the way
    if mode == "sample":
        assert len(np.unique(rec["action"])) > 1
    a.close()
    b.close()


def test_act_table_argument_rules(ctx):
    from dependence_free_rl_amd import XhError
    m = _domain(2, None)
    table = _table(m, 8)
    v = _venv(ctx, 8, 2, 5, None, policy_draws=0)
    with pytest.raises(XhError, match="policy_draws 0"):
        v.act_table(table)
    v.act_table(table, mode="argmax")
    v.set_record(1)
    v.act_table(table, mode="argmax")
    with pytest.raises(XhError, match="slots are full"):
        v.act_table(table, mode="argmax")
    with pytest.raises(ValueError, match="162 entries"):
        v.act_table(table[:100], mode="argmax")
    v.close()


# ---- 3. act_table with a PolicyNet -------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_act_table_with_a_policy_net(ctx, shape):
    from dependence_free_rl_amd import PolicyNet
    B, D, N, iset = shape
    widths = (64, 32)
    pol = PolicyNet(ctx, B, D, widths)
    pol.params = nref.make_params("policy", B, D, widths, 500 + B + D)
    a, b = (_venv(ctx, B, D, N, iset, seed=23) for _ in range(2))
    for v in (a, b):
        v.set_record(8)
    table = pol.forward(a.table_obs())
    assert table.shape == (a.table_info()["rows"], B)
    for _ in range(8):
        a.act_table(table)
        b.act(pol.forward(b.observe()), kind="logits", fetch=False)
    a.observe()
    b.observe()
    _same_venvs(a, b, False)
    a.close()
    b.close()
    pol.close()


# ---- a recorded window shared by the gather and the sum ----------------------
def _window(ctx, shape, steps=3):
    """A venv after `steps` recorded first-fit steps (states that differ from
    the fresh one), its domain, a table, and the STATE view's bins / items
    [(steps + 1) N] with slot P the present state."""
    B, D, N, iset = shape
    m = _domain(D, iset)
    v = _venv(ctx, B, D, N, iset, seed=31, policy_draws=0)
    v.set_record(steps)
    for _ in range(steps):
        v.act_heuristic("firstfit")
    rec = v.record()
    bins, items = _state(v)
    bins = np.concatenate([rec["bins"].reshape(-1, B, D), bins])
    items = np.concatenate([rec["items"].reshape(-1, 4), items])
    return v, m, _table(m, B, seed=3), bins, items


def _rows(total, N, seed):
    """A shuffled index list with a repeat that includes slot P's rows."""
    rng = np.random.default_rng(seed)
    r = rng.permutation(total).astype(np.int32)
    r = np.concatenate([r, r[:3], [total - 1, total - N]]).astype(np.int32)
    return r


# ---- 4. the gather -----------------------------------------------------------
@pytest.mark.parametrize("shape", SUM_SHAPES, ids=_ids)
def test_table_logits_is_the_references_gather(ctx, shape):
    from dependence_free_rl_amd import XhError
    B, D, N, iset = shape
    v, m, table, bins, items = _window(ctx, shape)
    total = bins.shape[0]
    want, live = m.gather(table, bins, items)
    assert live.all()
    _same(v.table_logits(table), want, "all rows")
    _same(v.table_logits(table, first=N + 1, count=N), want[N + 1:2 * N + 1],
          "a run of rows")
    r = _rows(total, N, 7)
    _same(v.table_logits(table, rows=r), want[r], "an index list")
    _same(v.table_logits(table, rows=r, first=2, count=5), want[r[2:7]],
          "part of an index list")
    v.synchronize()
    # a bad index: its row is left untouched, the others are written
    bad = r.copy()
    bad[1], bad[4] = total, -1
    out = v._scratch("out", bad.size * B * 4)
    fill = np.full((bad.size, B), 7.5, np.float32)
    v._upload(out, fill)
    v.table_logits(table, rows=bad, out=out)
    got = v._download(out, np.float32, (bad.size, B))
    exp = want[np.clip(bad, 0, total - 1)]
    exp[[1, 4]] = 7.5
    _same(got, exp, "with bad indices")
    with pytest.raises(XhError, match="row index"):
        v.synchronize()
    v.synchronize()
    v.close()


# ---- 5. the entry sum --------------------------------------------------------
def _dout(n, B, seed):
    """Magnitudes over 2^+-20, exact zeros (as at masked bins)."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, B)) * np.ldexp(1.0, rng.integers(-20, 21,
                                                                 (n, B)))
    d[rng.random((n, B)) < 0.3] = 0.0
    return d.astype(np.float32)


@pytest.mark.parametrize("shape", SUM_SHAPES, ids=_ids)
def test_table_grad_is_the_exact_entry_sum(ctx, shape):
    from dependence_free_rl_amd import XhError
    B, D, N, iset = shape
    v, m, _, bins, items = _window(ctx, shape)
    total, width = bins.shape[0], m.rows(B) * B
    e, live = m.row_entries(bins, items)
    assert live.all()
    # fresh bins are all at capacity: many (row, bin) pairs share an entry
    assert np.bincount(e.reshape(-1)).max() >= B
    r = _rows(total, N, 9)
    d1, d2 = _dout(r.size, B, 1), _dout(total, B, 2)
    g1 = tr.entry_sum(d1, e[r], live[r], m.E, width)
    g2 = tr.entry_sum(d2, e, live, m.E, width)
    _same(v.table_grad(d1, rows=r), g1, "an index list")
    _same(v.table_grad(d1, rows=r), g1, "again")
    _same(v.table_grad(d2), g2, "all rows")
    # accumulate: one f32 add per entry onto what is there
    v.table_grad(d1, rows=r)
    _same(v.table_grad(d2, accumulate=True), g1 + g2, "accumulate")
    # one row, one value; all zeros
    one = np.zeros((1, B), np.float32)
    one[0, B - 1] = -3.25
    _same(v.table_grad(one, first=total - 1, count=1),
          tr.entry_sum(one, e[-1:], live[-1:], m.E, width), "one row")
    assert not v.table_grad(np.zeros((total, B), np.float32)).any()
    v.synchronize()
    # a NaN (an infinity) in dout leaves g untouched and raises the flag
    g = v._scratch("g", width * 4)
    for poison in (np.nan, -np.inf):
        v._upload(g, np.full(width, 2.5, np.float32))
        d = d2.copy()
        d[total // 2, B // 2] = poison
        v.table_grad(d, out=g)
        assert np.all(v._download(g, np.float32, (width,)) == 2.5)
        with pytest.raises(XhError, match="NaN / infinity in dout"):
            v.synchronize()
    v.close()


# ---- 6. the table backward ---------------------------------------------------
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=_ids)
def test_table_backward_meets_the_per_row_budget(ctx, shape):
    from dependence_free_rl_amd import PolicyNet
    B, D, N, iset = shape
    widths = (64, 32)
    v, m, _, bins, items = _window(ctx, shape)
    total, R = bins.shape[0], m.rows(B)
    p = nref.make_params("policy", B, D, widths, 900 + B)
    obs = v.record_obs()
    assert obs.shape == (total, B, 2 * D)
    dout = nref.make_dout("policy", total, B, 77)
    want, mag = nref.gradient("policy", p, obs, dout, B, D, widths)
    pol = PolicyNet(ctx, B, D, widths)
    pol.params = p
    pol.backward(obs, dout)
    per_row = pol.grad
    G = v.table_grad(dout)
    pol.backward(v.table_obs(), G.reshape(R, B))
    table = pol.grad
    what = "table bwd %s" % _ids(shape)
    assert_grad_units(per_row, want, mag, what=what + " (per row)")
    assert_grad_units(table, want, mag, what=what)
    u_tab, _, _ = grad_units(table, want, mag)
    u_row, _, _ = grad_units(per_row, want, mag)
    line = {"what": what,
            "table_units": [float(np.median(u_tab)),
                            float(np.percentile(u_tab, 99)),
                            float(u_tab.max())],
            "per_row_units": [float(np.median(u_row)),
                              float(np.percentile(u_row, 99)),
                              float(u_row.max())]}
    print(json.dumps(line))
    pol.close()
    v.close()


# ---- 7. refusals ---------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sample", "argmax"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=_ids)
def test_states_outside_the_domain_are_refused(ctx, shape, mode):
    from dependence_free_rl_amd import XhError
    from dependence_free_rl_amd._lib import VENV_BINS, VENV_DONE, VENV_ITEMS
    B, D, N, iset = shape
    items, cap = (DEFAULT_ITEMS[D], 8) if iset is None else iset
    kept, old = list(items[:-1]) + [(2, 2)], items[-1]  # the last shape goes
    m = tr.Domain(kept, cap, D)
    table = _table(m, B, seed=5)
    a, b = (_venv(ctx, B, D, N, iset, seed=41) for _ in range(2))
    for v in (a, b):
        v.set_record(2)
        v.act_heuristic("firstfit")
        bins, its = _state(v)
        bins[1, B - 1, D - 1] = -1       # env 1: a bin below zero
        its[:, :D] = kept[0]             # every item one of the new set's,
        its[N - 1, :D] = kept[-1]
        its[2, :D] = old                 # but env 2's: a shape it lacks
        v.set(VENV_BINS, bins)
        v.set(VENV_ITEMS, its)
        v.set_item_set(kept)
        v.set(VENV_DONE, np.ones(N, np.uint8))
    before = {w: a.get(w) for w in (VENV_BINS, VENV_ITEMS)}
    rows, live = m.gather(table, bins, its)
    assert (~live).nonzero()[0].tolist() == [1, 2]
    rows[~live] = np.nan                 # the per-row act refuses a NaN row
    a.act_table(table, mode=mode, write_obs=False)
    b.act(rows, kind="logits", mode=mode, fetch=False)
    with pytest.raises(XhError, match="outside the table's domain"):
        a.synchronize()
    with pytest.raises(XhError, match="policy row was refused"):
        b.synchronize()
    for w in before:  # untouched
        _same(a.get(w)[1:3], before[w][1:3], "refused envs, buffer %d" % w)
    assert a.get(VENV_DONE)[1:3].tolist() == [0, 0]
    a.observe()
    b.observe()
    _same_venvs(a, b, False)
    # the recorded rows of those envs are skipped by the gather and the sum
    total = 3 * N
    sb = np.concatenate([a.record()["bins"].reshape(-1, B, D),
                         _state(a)[0]])
    si = np.concatenate([a.record()["items"].reshape(-1, 4), _state(a)[1]])
    e, live = m.row_entries(sb, si)
    # (slot 0 was recorded under the old set: its rows with the old shape too)
    dead = (~live).nonzero()[0]
    assert {N + 1, N + 2, 2 * N + 1, 2 * N + 2} <= set(dead.tolist())
    assert np.array_equal(dead[dead >= N], [N + 1, N + 2, 2 * N + 1, 2 * N + 2])
    out = a._scratch("out", total * B * 4)
    a._upload(out, np.full((total, B), -9.0, np.float32))
    a.table_logits(table, out=out)
    want, _ = m.gather(table, sb, si, out=np.full((total, B), -9.0,
                                                  np.float32))
    _same(a._download(out, np.float32, (total, B)), want, "gather")
    with pytest.raises(XhError, match="outside the table's domain"):
        a.synchronize()
    d = _dout(total, B, 4)
    _same(a.table_grad(d), tr.entry_sum(d, e, live, m.E, m.rows(B) * B),
          "entry sum")
    with pytest.raises(XhError, match="outside the table's domain"):
        a.synchronize()
    a.close()
    b.close()
