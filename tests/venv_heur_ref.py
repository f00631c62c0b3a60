"""Host restatement of xh_venv_act_heuristic (the four heuristic agents as an
act of the VecEnv), built on ItemsRef (tests/venv_items_ref.py): the three
score functions in numpy float32 as include/xylo_hip.h states them, the first
maximum (argmax_first) and, for random, Rng.discrete on the constant row.
tests/test_venv_heur_ref.py pins it to the oracle's or_heuristic_eval on the
reference's instance.  CPU only.

Also the fixtures the GPU tests share: the cases, the item sets and the seeded
near-full bins (preset_bins) that make "nothing fits", resets and exact
best-fit ties occur within a few tens of steps."""
import functools

import numpy as np

from venv_act_ref import argmax_first
from venv_items_ref import DEFAULT_ITEMS, DEFAULT_WEIGHTS, ItemsRef

KINDS = ("random", "firstfit", "bestfit", "minwaste")
DETERMINISTIC = KINDS[1:]

# (B, D, N, offset, Ng): tests/test_gpu_venv_items.py's
CASES = [(8, 2, 19, 0, 19), (32, 1, 70, 0, 70), (64, 2, 40, 0, 40),
         (128, 3, 5, 0, 5), (16, 3, 9, 6, 21)]
SHARDED_2D = (16, 2, 9, 6, 21)
X0 = 4242
STEPS = 24

ITEMS5 = [(3, 1), (2, 2), (1, 4), (5, 7), (1, 1)]
WEIGHTS5 = [2.0, 0.0, 1.0, 0.5, 3.25]  # item 1 is never drawn
CAP57 = (5, 7)
ITEMS16 = [(1 + k % 7, 1 + (3 * k) % 5) for k in range(16)]
WEIGHTS16 = [1.0 + (5 * k) % 7 for k in range(16)]
CAP75 = (7, 5)
ITEMS3D = [(6, 1, 3), (2, 8, 1), (1, 1, 1)]
WEIGHTS3D = [1.0, 2.0, 3.0]
CAP683 = (6, 8, 3)
ITEMS_ZERO = [(3, 0), (0, 2), (2, 2)]  # zero entries: best-fit's +0 terms
WEIGHTS_ZERO = [1.0, 1.0, 2.0]
CAP64 = (6, 4)

# name -> (case, items, weights, capacity); items None: the builtin instance
SETUPS = {}
for _c in CASES:
    SETUPS["default-B%d-D%d" % _c[:2]] = (_c, None, None, None)
SETUPS["K5-cap57-B8"] = (CASES[0], ITEMS5, WEIGHTS5, CAP57)
SETUPS["K5-cap57-sharded"] = (SHARDED_2D, ITEMS5, WEIGHTS5, CAP57)
SETUPS["K16-cap75-B64"] = (CASES[2], ITEMS16, WEIGHTS16, CAP75)
SETUPS["K3-cap683-B128"] = (CASES[3], ITEMS3D, WEIGHTS3D, CAP683)
SETUPS["zero-cap64-sharded"] = (SHARDED_2D, ITEMS_ZERO, WEIGHTS_ZERO, CAP64)


def scores(kind, bins, item, cap):
    """float32 [B]: the heuristic's score of every bin (bins int [B][D], item
    int [D], cap int [D])."""
    bins = np.asarray(bins, np.int32)
    item = np.asarray(item, np.int32)
    D = bins.shape[1]
    fits = (bins >= item).all(axis=1)
    if kind == "firstfit":
        return np.where(fits, np.float32(1.0), np.float32(0.0))
    if kind == "bestfit":
        s = np.zeros(len(bins), np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            for d in range(D):
                if item[d] == 0:
                    term = np.zeros(len(bins), np.float32)
                else:
                    term = np.float32(item[d]) / bins[:, d].astype(np.float32)
                s = term if d == 0 else (s + term).astype(np.float32)
        assert s.dtype == np.float32
        return np.where(fits, s, np.float32(-1.0))
    if kind == "minwaste":
        r = bins - item
        is_half = r == (np.asarray(cap, np.int32) // 2)
        half = is_half.sum(axis=1)
        zero = (~is_half & (r == 0)).sum(axis=1)
        sc = np.where((half == 1) & (zero == D - 1), np.float32(0.0),
                      np.float32(1.0))
        return np.where(fits, sc, np.float32(-1.0))
    raise ValueError(kind)


class HeurRef(ItemsRef):
    """ItemsRef with act_heuristic; policy_draws 2 for random, else 0 unless
    given."""

    def __init__(self, B, D, N, x0, items=None, weights=None, capacity=None,
                 policy_draws=2, n_global=None, offset=0):
        if items is None:
            items, weights, capacity = DEFAULT_ITEMS[D], DEFAULT_WEIGHTS, 8
        super().__init__(B, D, N, x0, items, weights, capacity,
                         policy_draws=policy_draws, n_global=n_global,
                         offset=offset)

    def set_bins(self, bins):
        """xh_venv_set(XH_VENV_BINS)."""
        bins = np.asarray(bins).reshape(self.N, self.B, self.D)
        for e, env in enumerate(self.envs):
            env.bins[:] = bins[e]

    def scores(self, kind, e):
        return scores(kind, self.envs[e].bins, self.envs[e].item, self.cap)

    def act_heuristic(self, kind, masked=False):
        """One xh_venv_act_heuristic call.  masked changes random alone."""
        if kind == "random":
            rows = np.full((self.N, self.B), np.float32(1.0 / self.B),
                           np.float32)
            return self.act(rows, "sample", masked=masked)
        sc = np.stack([self.scores(kind, e) for e in range(self.N)])
        out = self.act(sc, "argmax")
        out["pchoice"][:] = np.float32(1.0)
        return out


def preset_bins(ref, seed):
    """int8 [N][B][D]: seeded near-full states for ref's envs as they stand.
    Most bins hold 0 or 1 per dim and a few hold between half and all of the
    capacity.  By env index e:
      e % 4 == 1  every bin empty: nothing fits, whatever the item;
      e % 4 == 3  bin 0 holds the item plus half of dim 0's capacity where
                  that is within it: first-fit takes it, min-waste scores it 0;
      e % 2 == 0  where two dims i < j of the item can be doubled within the
                  capacity, two bins hold the item with entry i doubled and
                  with entry j doubled, and no bin holds the item exactly:
                  different contents that best-fit scores alike in f32 (item
                  (2,2): bins (4,2) and (2,4), 2/4 + 2/2 and 2/2 + 2/4), and
                  only an exact fit would score higher."""
    g = np.random.default_rng(seed)
    B, D, N, cap = ref.B, ref.D, ref.N, ref.cap
    bins = g.integers(0, 2, (N, B, D))
    for e in range(N):
        it = ref.envs[e].item
        if e % 4 == 1:
            bins[e] = 0
        else:
            for b in g.choice(B, max(2, min(5, B // 4)), replace=False):
                bins[e, b] = [g.integers(cap[d] // 2, cap[d] + 1)
                              for d in range(D)]
        if e % 4 == 3 and it[0] + cap[0] // 2 <= cap[0]:
            bins[e, 0] = it
            bins[e, 0, 0] += cap[0] // 2
        dbl = [d for d in range(D) if it[d] > 0 and 2 * it[d] <= cap[d]]
        if e % 2 == 0 and len(dbl) >= 2:
            exact = (bins[e] == it).all(axis=1)
            bins[e, exact, dbl[0]] += 1
            lo, hi = sorted(g.choice(B, 2, replace=False))
            x, y = it.copy(), it.copy()
            x[dbl[0]] *= 2
            y[dbl[1]] *= 2
            bins[e, lo], bins[e, hi] = (x, y) if g.random() < 0.5 else (y, x)
    return bins.astype(np.int8)


def make_ref(name, kind, x0=X0):
    """(ref, preset): the restatement of SETUPS[name] for `kind`, its bins
    preset (the preset depends on the setup alone, not on the kind)."""
    case, items, weights, capacity = SETUPS[name]
    B, D, N, offset, Ng = case
    ref = HeurRef(B, D, N, x0, items, weights, capacity,
                  policy_draws=2 if kind == "random" else 0, n_global=Ng,
                  offset=offset)
    preset = preset_bins(ref, sum(map(ord, name)))
    ref.set_bins(preset)
    return ref, preset


def _state(ref):
    return {"bins": ref.bins(), "item": ref.items(), "rng": ref.streams(),
            "obs": ref.obs(), "legal": ref.legal()}


def _diag(ref):
    """What a step's states hold, for the fixture conditions: per env, whether
    nothing fits; whether best-fit's maximum is shared by two fitting bins of
    different contents; whether that maximum is no multiple of 1/8; and the
    three deterministic picks."""
    nofit = np.zeros(ref.N, bool)
    tie = np.zeros(ref.N, bool)
    odd = np.zeros(ref.N, bool)
    picks = np.zeros((ref.N, 3), np.int32)
    for e, env in enumerate(ref.envs):
        fits = (env.bins >= env.item).all(axis=1)
        nofit[e] = not fits.any()
        for i, kind in enumerate(DETERMINISTIC):
            picks[e, i] = argmax_first(ref.scores(kind, e))
        if fits.any():
            sc = ref.scores("bestfit", e)
            top = np.flatnonzero(fits & (sc == sc.max()))
            tie[e] = len({tuple(env.bins[b]) for b in top}) > 1
            odd[e] = float(sc.max()) * 8.0 != np.floor(float(sc.max()) * 8.0)
    return {"nofit": nofit, "tie": tie, "odd": odd, "picks": picks}


@functools.lru_cache(maxsize=None)
def trajectory(name, kind, masked=False, steps=STEPS):
    """The restatement's run of SETUPS[name] under `kind`, computed once and
    shared (treat it as read-only): "preset" int8 [N][B][D], "first" (the state
    after the preset) and "steps", a list of dicts with action / pchoice /
    reward / done, the state after the step (bins / item / rng / obs / legal)
    and "diag" of the state before it."""
    ref, preset = make_ref(name, kind)
    out = {"preset": preset, "first": _state(ref), "steps": []}
    for _ in range(steps):
        diag = _diag(ref)
        r = ref.act_heuristic(kind, masked=masked)
        r.update(_state(ref))
        r["diag"] = diag
        out["steps"].append(r)
    return out
