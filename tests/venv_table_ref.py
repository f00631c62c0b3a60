"""Host restatement of a venv's logit table (xh_venv_table_*,
include/xylo_hip.h; csrc/xh_venv_table.h) in numpy: the domain's index and its
inverse enumeration, the table's observations, the gather of a row's logits
and the exact int64 entry sum of the table gradient.  Written from the
header's text, not from the C++ (tests/test_venv_table_cpu.py compares the
two).  CPU only."""
import math

import numpy as np

MAX_ENTRIES = 16384


class Domain:
    """items [K][D] ints, capacity [D] (or one int)."""

    def __init__(self, items, capacity, D):
        self.D = D
        self.shapes = np.asarray(items, np.int64).reshape(-1, D)
        self.K = len(self.shapes)
        self.cap = np.broadcast_to(np.asarray(capacity, np.int64), (D,)).copy()
        self.side = self.cap + 1
        self.S = int(np.prod(self.side))
        self.E = self.K * self.S

    def rows(self, B):
        return (self.E + B - 1) // B

    def item_index(self, item):
        """The first shape equal to the item, -1 where there is none."""
        item = np.asarray(item, np.int64).reshape(-1)[:self.D]
        for k in range(self.K):
            if np.array_equal(self.shapes[k], item):
                return k
        return -1

    def state_index(self, b):
        """s of bins [..][D]; -1 where a value is outside [0, capacity]."""
        b = np.asarray(b, np.int64)
        ok = ((b >= 0) & (b <= self.cap)).all(-1)
        s = np.zeros(b.shape[:-1], np.int64)
        for d in range(self.D):
            s = s * self.side[d] + np.where(ok, b[..., d], 0)
        return np.where(ok, s, -1)

    def entry(self, bins, item):
        """e of bins [..][D] under one item [D]; -1 outside the domain."""
        k = self.item_index(item)
        s = self.state_index(bins)
        if k < 0:
            return np.full(s.shape, -1, np.int64)
        return np.where(s >= 0, k * self.S + s, -1)

    def decode(self, e):
        """(k, b [D]) of entry e < E."""
        k, s = divmod(int(e), self.S)
        b = np.zeros(self.D, np.int64)
        for d in range(self.D - 1, -1, -1):
            s, b[d] = divmod(s, int(self.side[d]))
        return k, b

    def table_obs(self, B):
        """[R][B][2D] float32: per-bin row e is entry e's observation, the
        formula of venv_items_ref.ItemsRef.obs; zeros from E on."""
        R = self.rows(B)
        out = np.zeros((R * B, 2 * self.D), np.float32)
        capf = self.cap.astype(np.float32)
        for e in range(self.E):
            k, b = self.decode(e)
            out[e, :self.D] = b.astype(np.float32) / capf
            out[e, self.D:] = self.shapes[k].astype(np.float32) / capf
        return out.reshape(R, B, 2 * self.D)

    def row_entries(self, bins, items):
        """bins int [n][B][D], items int [n][>=D] -> (e int64 [n][B], live bool
        [n]): a row is live when every bin and the item are inside."""
        bins = np.asarray(bins, np.int64)
        n = bins.shape[0]
        e = np.zeros(bins.shape[:2], np.int64)
        for j in range(n):
            e[j] = self.entry(bins[j], np.asarray(items[j])[:self.D])
        return e, (e >= 0).all(1)

    def gather(self, table, bins, items, out=None):
        """[n][B] float32 logits; rows that are not live keep `out`'s."""
        table = np.asarray(table, np.float32).reshape(-1)
        e, live = self.row_entries(bins, items)
        res = np.zeros(e.shape, np.float32) if out is None else out.copy()
        res[live] = table[e[live]]
        return res, live


# ---- the fixed-point entry sum ------------------------------------------
def quant_log2(n):
    """The least L with 2^L >= n."""
    L = 0
    while (1 << L) < n:
        L += 1
    return L


def quant_exponent(m):
    """ex with 2^(ex-1) <= m < 2^ex, m > 0 finite."""
    return math.frexp(float(m))[1]


def quant_shift(n, m):
    return 62 - quant_log2(n) - quant_exponent(m)


def quantise(g, s):
    """llrint((double)g * 2^s) as int64: the product exact, np.rint to nearest
    even."""
    return np.rint(np.ldexp(np.asarray(g, np.float32).astype(np.float64),
                            s)).astype(np.int64)


def dequantise(total, s):
    """(float)((double)sum * 2^-s): int64 -> double and double -> float both to
    nearest even (numpy's conversions)."""
    return np.ldexp(np.asarray(total, np.int64).astype(np.float64),
                    -s).astype(np.float32)


def entry_sum(dout, entries, live, E, total):
    """G float32 [total] of dout [n][B] under entries [n][B] / live [n]: m over
    ALL of dout's floats, n = dout.size addends.  None where dout holds a NaN
    or an infinity (g is left untouched)."""
    dout = np.asarray(dout, np.float32)
    if not np.isfinite(dout).all():
        return None
    G = np.zeros(total, np.float32)
    m = float(np.abs(dout).max()) if dout.size else 0.0
    if m == 0.0:
        return G
    s = quant_shift(dout.size, m)
    acc = np.zeros(E, np.int64)
    q = quantise(dout, s)
    np.add.at(acc, entries[live].reshape(-1), q[live].reshape(-1))
    G[:E] = dequantise(acc, s)
    return G
