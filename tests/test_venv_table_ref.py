"""Pins tests/venv_table_ref.py, the numpy restatement of a venv's logit
table: its observation rows are venv_items_ref's observation formula entry by
entry, its index is a bijection onto [0, E) (first-equal-shape for a set with
a duplicate), and its int64 entry sum is the exact sum in Python integers.
CPU only."""
from fractions import Fraction

import numpy as np
import pytest

import venv_table_ref as tr
from venv_items_ref import DEFAULT_ITEMS, ItemsRef

# (items, capacity, D); weights do not enter the domain
SETS = {
    "default1": (DEFAULT_ITEMS[1], 8, 1),
    "default2": (DEFAULT_ITEMS[2], 8, 2),
    "default3": (DEFAULT_ITEMS[3], 8, 3),
    "cap57": ([(3, 1), (2, 2), (1, 4)], (5, 7), 2),
    # item 1 repeats item 0 (and would carry weight 0 in a curriculum)
    "duplicate": ([(2, 1), (2, 1), (1, 3)], (4, 4), 2),
    # 16 items x 3 * 11 * 31 = 16368 and x 5 * 5 * 41 = 16400 entries
    "under": ([(1, k % 11, 1 + k) for k in range(16)], (2, 10, 30), 3),
    "over": ([(1, 1, 1 + k) for k in range(16)], (4, 4, 40), 3),
}


def test_set_sizes():
    E = {n: tr.Domain(*s).E for n, s in SETS.items()}
    assert E == {"default1": 18, "default2": 162, "default3": 1458,
                 "cap57": 144, "duplicate": 75, "under": 16368, "over": 16400}
    assert E["under"] < tr.MAX_ENTRIES < E["over"]
    assert tr.Domain(*SETS["default2"]).rows(64) == 3
    assert tr.Domain(*SETS["default3"]).rows(128) == 12


@pytest.mark.parametrize("name", sorted(SETS))
def test_index_is_a_bijection(name):
    items, cap, D = SETS[name]
    m = tr.Domain(items, cap, D)
    seen = np.zeros(m.E, np.int64)
    first = [m.item_index(m.shapes[k]) for k in range(m.K)]
    # every (first-occurrence item, state) -> an entry, each exactly once
    grids = np.stack(np.meshgrid(*[np.arange(s) for s in m.side],
                                 indexing="ij"), -1).reshape(-1, D)
    for k in range(m.K):
        e = m.entry(grids, m.shapes[k])
        assert e.min() >= 0 and e.max() < m.E
        assert np.array_equal(e, first[k] * m.S + np.arange(m.S))
        if first[k] == k:
            seen[e] += 1
    distinct = [k for k in range(m.K) if first[k] == k]
    assert np.array_equal(np.nonzero(seen)[0],
                          np.concatenate([k * m.S + np.arange(m.S)
                                          for k in distinct]))
    assert seen.max() == 1
    # the enumeration is the inverse
    for e in range(0, m.E, 1 if m.E < 2000 else 7):
        k, b = m.decode(e)
        assert m.entry(b, m.shapes[k]) == first[k] * m.S + e % m.S
        assert k * m.S + m.state_index(b) == e
    if name != "duplicate":
        assert first == list(range(m.K))


def test_outside_the_domain():
    m = tr.Domain(*SETS["cap57"])
    assert m.entry(np.array([5, 7]), (3, 1)) == 0 * 48 + 5 * 8 + 7
    assert m.entry(np.array([0, 0]), (1, 4)) == 2 * 48
    for b in ((-1, 0), (0, -1), (6, 0), (0, 8)):
        assert m.entry(np.array(b), (3, 1)) == -1
    assert m.entry(np.array([1, 1]), (4, 2)) == -1  # not one of the shapes
    e, live = m.row_entries(np.array([[[1, 1], [2, 2]], [[1, 1], [-1, 2]]]),
                            np.array([[2, 2, 0, 0], [2, 2, 0, 0]]))
    assert live.tolist() == [True, False]
    assert e[0].tolist() == [48 + 9, 48 + 18]


@pytest.mark.parametrize("name", ["default1", "default2", "default3", "cap57",
                                  "duplicate"])
def test_observation_rows_are_the_venvs(name):
    items, cap, D = SETS[name]
    m = tr.Domain(items, cap, D)
    B = 8
    obs = m.table_obs(B)
    assert obs.shape == (m.rows(B), B, 2 * D) and obs.dtype == np.float32
    flat = obs.reshape(-1, 2 * D)
    assert not flat[m.E:].any()
    ref = ItemsRef(B, D, 1, 7, items, capacity=cap)
    for e in range(m.E):
        k, b = m.decode(e)
        ref.envs[0].bins[0] = b
        ref.envs[0].item = m.shapes[k].astype(np.int32)
        assert np.array_equal(ref.obs()[0, 0].view(np.uint32),
                              flat[e].view(np.uint32)), e


def _exact_sum(dout, entries, E):
    """The reference's G from Python integers and fractions."""
    m = float(np.abs(dout).max())
    s = tr.quant_shift(dout.size, m)
    acc = [0] * E
    for g, e in zip(dout.reshape(-1), entries.reshape(-1)):
        x = Fraction(float(g)) * Fraction(2) ** s
        q = round(x)  # Python rounds halves to even
        assert abs(q) <= 2 ** (62 - tr.quant_log2(dout.size))
        acc[e] += q
    assert all(abs(a) < 2 ** 62 for a in acc)
    out = np.zeros(E, np.float32)
    for e, a in enumerate(acc):
        out[e] = np.float32(np.ldexp(float(a), -s))  # int -> double: to even
    return out, s


def test_entry_sum_is_the_exact_integer_sum():
    rng = np.random.default_rng(5)
    n, B, E = 37, 8, 20
    mag = np.ldexp(1.0, rng.integers(-20, 21, (n, B)))
    dout = (rng.standard_normal((n, B)) * mag).astype(np.float32)
    dout[rng.random((n, B)) < 0.3] = 0.0
    entries = rng.integers(0, 4, (n, B))  # many duplicates
    live = np.ones(n, bool)
    live[5] = False
    G = tr.entry_sum(dout, entries, live, E, 24)
    ex, s = _exact_sum(np.where(live[:, None], dout, 0).astype(np.float32),
                       entries, E)
    # the skipped row's floats still count towards m and n
    assert s == tr.quant_shift(dout.size, float(np.abs(dout).max()))
    assert np.array_equal(G[:E].view(np.uint32), ex.view(np.uint32))
    assert not G[E:].any() and G.shape == (24,)
    # close to the float64 sum: the stated bound
    f64 = np.zeros(E)
    np.add.at(f64, entries[live].reshape(-1),
              dout[live].astype(np.float64).reshape(-1))
    cnt = np.bincount(entries[live].reshape(-1), minlength=E)
    bound = cnt * 2.0 ** (-s - 1) + np.abs(f64) * (2.0 ** -24 + 2.0 ** -52)
    assert np.all(np.abs(G[:E] - f64) <= bound)


def test_entry_sum_edges():
    z = np.zeros((3, 8), np.float32)
    e = np.zeros((3, 8), np.int64)
    live = np.ones(3, bool)
    assert not tr.entry_sum(z, e, live, 4, 8).any()
    z[1, 2] = np.nan
    assert tr.entry_sum(z, e, live, 4, 8) is None
    z[1, 2] = np.inf
    assert tr.entry_sum(z, e, live, 4, 8) is None
    # ex: 2^(ex-1) <= m < 2^ex, denormals included
    assert tr.quant_exponent(1.0) == 1 and tr.quant_exponent(0.75) == 0
    assert tr.quant_exponent(np.float32(2.0 ** -149)) == -148
    assert tr.quant_exponent(np.float32(3.0e38)) == 128
    assert [tr.quant_log2(n) for n in (1, 2, 3, 4, 5, 1024, 1025)] == \
        [0, 1, 2, 2, 3, 10, 11]
