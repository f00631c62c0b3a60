"""Cases and host-built windows of the record-reading value net
(ValueNet.forward_record / backward_record, xh_net_*_record): the reference of
tests/test_venv_value_ref.py and tests/test_gpu_venv_value.py.  CPU only.

A case's window is the restatement's run (venv_heur_ref.HeurRef) of N = 24
envs from seeded near-full bins (preset_bins) through T = 5 steps of the
random agent, so that episodes end inside it; its two views are
venv_learn_ref.state_rows / next_rows, turned into the float32 observations
record_obs writes ((float)v / (float)capacity[d]).  The net's values and
gradients are venv_net_ref.forward / gradient("value", ...).

Few-row gradient cases are conditioned as venv_net_ref.py explains: a case
takes the first seed (base, base + 100000, ...) on which numpy's own float32
gradient is within conftest's default budgets of the float64 one and, up to
WELL_ROWS rows, whose inputs hold every positive H1 above WELL * its mag --
judged on these restatements alone, never on the kernels.

Why the H1 condition stops at WELL_ROWS = 9 rows.  An H1 value z that nearly
cancels carries a relative error of a few u mag / z into its row's term of
the 32 entries of its column of dW1; that term is about 1 / rows of the
entry's mag, so the entry moves by a few (mag / z) / rows units: thousands of
units at one row and hundreds at nine for z = WELL * mag -- there the luck of
one rounding decides the 99th percentile (two or three such features cover 1 %
of the entries at Fin = 96), in any float32 evaluation, and the float32
condition alone, met by numpy's order of summation, says nothing about
another order.  At 120 rows the same term is diluted to tens of units, and the
condition could not be met at any seed anyway: 120 x 64 values of H1, each
within (0, WELL mag) with a probability of about 0.7 % at Fin = 768."""
import functools

import numpy as np

import long_window_ref as lw
import venv_heur_ref as hr
import venv_learn_ref as lr
import venv_net_ref as nr

WIDTHS = (64, 32)
N, T = 24, 5
STATE_ROWS, NEXT_ROWS = (T + 1) * N, T * N
# (B, D): Fin = 2BD from 16 to 768, one chunk and many, every dims
SHAPES = ((8, 1), (8, 2), (16, 3), (64, 2), (128, 3))
# (B, D, builtin): ITEMS[D] of venv_net_ref (non-default items and
# capacities), plus one venv on the builtin instance
WINDOWS = tuple((B, D, False) for B, D in SHAPES) + ((8, 2, True),)
COUNTS = (1, 9, 120)


def window_seed(B, D, builtin):
    return 500 + 10 * B + D + (7 if builtin else 0)


def item_set(D, builtin):
    """(items, capacity) of the venv; (None, None): the builtin instance."""
    return (None, None) if builtin else nr.ITEMS[D]


def _obs_f32(rows64, B, D, cap):
    """state_rows / next_rows give v / 8 exactly; record_obs's bits are
    float32(v) / float32(cap[d])."""
    v = np.rint(np.asarray(rows64).reshape(-1, B, 2 * D) * lw.CAP)
    capf = np.asarray(cap, np.float32)
    capf = np.concatenate([capf, capf])
    out = v.astype(np.float32) / capf
    assert out.dtype == np.float32
    return out


@functools.lru_cache(maxsize=None)
def window(B, D, builtin=False):
    """The restatement's window, computed once and shared (read-only): preset
    int8 [N][B][D], record (bins / items / action / done of slots 0 .. T - 1),
    present (bins, items), cap, and the float32 views "state" [(T + 1) N][B][2D]
    and "next" [T N][B][2D] with "ended", the number of ended transitions."""
    items, cap = item_set(D, builtin)
    x0 = window_seed(B, D, builtin)
    ref = hr.HeurRef(B, D, N, x0, items, None, cap, policy_draws=2)
    preset = hr.preset_bins(ref, x0 + 1)
    ref.set_bins(preset)
    rec = {k: [] for k in ("bins", "items", "action", "done")}
    for _ in range(T):
        rec["bins"].append(ref.bins())
        rec["items"].append(ref.items())
        r = ref.act_heuristic("random")
        rec["action"].append(r["action"])
        rec["done"].append(r["done"])
    rec = {k: np.stack(v) for k, v in rec.items()}
    present = (ref.bins(), ref.items())
    capv = np.asarray(ref.cap, np.int32)
    return {"preset": preset, "record": rec, "present": present, "cap": capv,
            "x0": x0,
            "state": _obs_f32(lr.state_rows(rec, *present), B, D, capv),
            "next": _obs_f32(lr.next_rows(rec, present), B, D, capv),
            "ended": int((rec["done"] != 0).sum())}


def make_params(B, D, seed):
    return nr.make_params("value", B, D, WIDTHS, seed)


# ---- the gradient cases ---------------------------------------------------
def grad_view(count):
    """120 rows are the whole NEXT view (ended rows among them), shuffled; the
    smaller counts come from the STATE view."""
    return "next" if count == NEXT_ROWS else "state"


def grad_inputs(B, D, count, seed):
    """(params, rows int32 [count], dout [count]): a shuffled index list into
    the view and venv_net_ref's loss gradients with their exact-zero rows."""
    view = grad_view(count)
    total = NEXT_ROWS if view == "next" else STATE_ROWS
    rng = np.random.default_rng(seed + 3)
    rows = rng.permutation(total)[:count].astype(np.int32)
    return (make_params(B, D, seed), rows,
            nr.make_dout("value", count, B, seed + 2))


WELL_ROWS = 9


def well_conditioned(params, obs, B, D):
    """venv_net_ref.well_conditioned for the value net's layer 0: every
    positive H1 pre-activation is at least WELL * its mag."""
    p = np.asarray(params, np.float64)
    x = np.asarray(obs, np.float64).reshape(-1, B * 2 * D)
    A, b = nr.split(p, [B * 2 * D, WIDTHS[0], WIDTHS[1], 1])[0]
    z = x @ A.T + b
    m = np.abs(x) @ np.abs(A).T + np.abs(b)
    return bool(np.all((z <= 0) | (z >= nr.WELL * m)))


def conditioned(params, obs, dout, B, D):
    """The condition a gradient case's seed has to meet."""
    if len(dout) <= WELL_ROWS and not well_conditioned(params, obs, B, D):
        return False
    return float32_in_budget(params, obs, dout, B, D)


def float32_in_budget(params, obs, dout, B, D):
    """numpy's float32 gradient within conftest's default budgets (median 1,
    p99 100 units, at most 1 % + 1 entries over 1024) of the float64 one."""
    g, mag = nr.gradient("value", params, obs, dout, B, D, WIDTHS)
    g32, _ = nr.gradient("value", params, obs, dout, B, D, WIDTHS, np.float32)
    nz = mag > 0
    u = np.abs(g32[nz].astype(np.float64) - g[nz]) / (nr.U32 * mag[nz])
    return bool(np.median(u) <= 1.0 and np.percentile(u, 99) <= 100.0 and
                (u > 1024).sum() <= 0.01 * u.size + 1)


@functools.lru_cache(maxsize=None)
def grad_cases():
    """(B, D, count, seed) of every GPU gradient test input."""
    out = []
    for B, D in SHAPES:
        w = window(B, D)
        for count in COUNTS:
            seed = 9000 + 100 * count + 10 * B + D
            while True:  # every count here is a few-row case (<= FEW_ROWS)
                p, rows, dout = grad_inputs(B, D, count, seed)
                if conditioned(p, w[grad_view(count)][rows], dout, B, D):
                    break
                seed += 100000
            out.append((B, D, count, seed))
    assert all(c <= nr.FEW_ROWS for c in COUNTS)
    return tuple(out)


# the grid-cap and accumulation test's inputs: the whole STATE view, three
# tiles of 64 rows, shuffled; conditioned like the few-row cases
GRID_SHAPES = ((8, 2), (64, 2), (128, 3))


@functools.lru_cache(maxsize=None)
def grid_cases():
    out = []
    for B, D in GRID_SHAPES:
        w = window(B, D)
        seed = 700 + 10 * B + D
        while True:
            p, rows, dout = grad_inputs(B, D, STATE_ROWS, seed)
            if conditioned(p, w["state"][rows], dout, B, D):
                break
            seed += 100000
        out.append((B, D, STATE_ROWS, seed))
    return tuple(out)


def forward_bound(B, D, mag):
    """(2BD + 64 + 32 + 11) u mag: venv_net_ref.forward_bound with the first
    chain's 2BD terms; it holds for any order of each chain's sum."""
    return (2 * B * D + WIDTHS[0] + WIDTHS[1] + 11) * nr.U32 * np.asarray(mag)
