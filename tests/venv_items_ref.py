"""Host restatement of a VecEnv on a general item set (xh_item_set): K shapes
drawn by the K-way threshold rule, a capacity per dim.  Built only from the
oracle's primitives (oracle.pyoracle: Rng.canonical, Rng.discrete, or_argmax,
minstd_jump), with the structure of venv_act_ref.ActRef: ONE engine seeded at
state x0, Ng envs constructed in order, every step visits every env in env
order.  tests/test_venv_items_ref.py pins it to the oracle's own env where
the oracle can express the case (two items, one capacity).  CPU only."""
import numpy as np

from oracle import pyoracle as po
from venv_act_ref import argmax_first

# make_env's two items (xh_host.h), by dims
DEFAULT_ITEMS = {1: [(4,), (1,)], 2: [(4, 2), (1, 2)],
                 3: [(4, 2, 2), (1, 2, 1)]}
DEFAULT_WEIGHTS = [0.4, 0.6]


def thresholds(weights):
    """c_k of include/xylo_hip.h, in double: W the sequential sum, c_k =
    c_(k-1) + w_k / W, and 1.0 from the last item of positive weight on."""
    w = [float(x) for x in weights]
    W = 0.0
    for x in w:
        W = W + x
    acc, c = 0.0, []
    for x in w:
        acc = acc + x / W
        c.append(acc)
    last = max(k for k, x in enumerate(w) if x > 0.0)
    for k in range(last, len(w)):
        c[k] = 1.0
    return np.array(c, np.float64)


def pick_item(c, u):
    """The first k with u < c_k."""
    for k, ck in enumerate(c):
        if u < ck:
            return k
    raise AssertionError("u = %r is not below c[-1] = %r" % (u, c[-1]))


class _Env:
    def __init__(self, B, D):
        self.bins = np.zeros((B, D), np.int32)
        self.item = np.zeros(D, np.int32)


class ItemsRef:
    """Ng agents on one engine; the envs [offset, offset + N) are kept."""

    def __init__(self, B, D, N, x0, items, weights=None, capacity=None,
                 policy_draws=2, n_global=None, offset=0):
        self.B, self.D, self.N = B, D, N
        self.Ng, self.offset, self.pd = n_global or N, offset, policy_draws
        self.k = policy_draws + 2
        self.cap = np.broadcast_to(
            np.asarray(8 if capacity is None else capacity, np.int32), (D,))
        self.set_item_set(items, weights)
        self.rng = po.Rng(x0)
        self.envs = []
        for g in range(self.Ng):  # constructed one after another
            e = _Env(B, D)
            self._reset(e)
            if offset <= g < offset + N:
                self.envs.append(e)

    def set_item_set(self, items, weights=None):
        """From the next draw on; held items stay, no stream position moves."""
        self.shapes = np.asarray(items, np.int32).reshape(-1, self.D)
        K = len(self.shapes)
        self.c = thresholds(np.ones(K) if weights is None else weights)

    # ---- bp::environment on the set --------------------------------------
    def _draw(self, env):
        env.item = self.shapes[pick_item(self.c, self.rng.canonical())].copy()

    def _reset(self, env):
        env.bins[:] = self.cap
        self._draw(env)

    def _apply(self, env, choice):
        """environment::apply: a new item unless the chosen bin went
        negative."""
        env.bins[choice] -= env.item
        if not (env.bins[choice] < 0).any():
            self._draw(env)

    # ---- what the device holds between two calls -------------------------
    def bins(self):
        return np.stack([e.bins for e in self.envs]).astype(np.int8)

    def items(self):
        return np.stack([e.item for e in self.envs]).astype(np.int8)

    def obs(self):
        """observation::to_vector: float(x) / float(capacity[d]), f32."""
        capf = self.cap.astype(np.float32)
        out = np.zeros((self.N, self.B, 2 * self.D), np.float32)
        for n, e in enumerate(self.envs):
            out[n, :, :self.D] = e.bins.astype(np.float32) / capf
            out[n, :, self.D:] = e.item.astype(np.float32) / capf
        return out

    def legal(self):
        """eff(e) bool [N][B]: the bins that take the item; all where none."""
        out = np.zeros((self.N, self.B), bool)
        for n, e in enumerate(self.envs):
            fits = (e.bins >= e.item).all(axis=1)
            out[n] = fits if fits.any() else True
        return out

    def streams(self):
        """The engine state at each kept env's turn of the next step
        (XH_VENV_RNG); valid for envs no call has refused."""
        return np.array([po.minstd_jump(self.rng.state,
                                        self.k * (self.offset + e))
                         for e in range(self.N)], np.uint32)

    def draws(self):
        """u of each kept env's next pick (SAMPLE), without consuming it."""
        return np.array([po.Rng(int(x)).canonical() for x in self.streams()])

    def _skip(self, n):
        self.rng.x.value = po.minstd_jump(self.rng.state, n)

    def _visit(self, pick):
        N = self.N
        out = {"action": np.zeros(N, np.int32),
               "pchoice": np.zeros(N, np.float32),
               "reward": np.zeros(N, np.float32),
               "done": np.zeros(N, np.uint8)}
        for g in range(self.Ng):
            e = g - self.offset
            if not 0 <= e < N:
                self._skip(self.k)  # the other envs' react + item draws
                continue
            r = pick(e)
            if r is None:           # refused: untouched, the others go on
                continue
            env = self.envs[e]
            out["action"][e], out["pchoice"][e] = r
            self._apply(env, r[0])
            over = bool((env.bins < 0).any())
            out["reward"][e], out["done"][e] = (0.0 if over else 1.0), over
            if over:
                self._reset(env)
        return out

    def act(self, rows, mode="sample", refuse=(), masked=False):
        """rows [N][B] float32 probabilities (values, for argmax); masked:
        entries outside eff(e) are 0 first (set_action_mask, probs)."""
        rows = np.ascontiguousarray(rows, np.float32).copy()
        if masked:
            rows[~self.legal()] = 0.0

        def pick(e):
            if e in refuse:
                self._skip(self.k)
                return None
            if mode == "sample":
                assert self.pd == 2
                c = self.rng.discrete(rows[e])
            else:
                self._skip(self.pd)
                c = argmax_first(rows[e])
            return c, rows[e, c]
        return self._visit(pick)

    def step(self, actions):
        """xh_venv_step: the caller's actions, the policy's draws skipped."""
        def pick(e):
            self._skip(self.pd)
            return int(actions[e]), 0.0
        return self._visit(pick)

    # ---- environment::apply / reset on the env's own stream --------------
    # With Ng = 1 the env's stream is the engine; the restatement has no
    # other way to say "where the env's stream stands".
    def apply(self, action):
        """xh_venv_apply of the one env: no reset; returns game_over."""
        assert self.Ng == 1 and self.N == 1
        self._apply(self.envs[0], int(action))
        return bool((self.envs[0].bins < 0).any())

    def reset(self):
        assert self.Ng == 1 and self.N == 1
        self._reset(self.envs[0])


def run(ref, rows, masked=False):
    """Drive `ref` through act(rows[s]) for every s.  Returns bins
    [S+1][N][B][D] / item [S+1][N][D] int8, obs [S+1][N][B][2D], rng
    [S+1][N], legal [S+1][N][B], u [S][N], action / pchoice / reward / done
    [S][N], x_end."""
    S = len(rows)
    out = {k: [] for k in ("bins", "item", "obs", "rng", "legal", "u",
                           "action", "pchoice", "reward", "done")}
    for s in range(S + 1):
        out["bins"].append(ref.bins())
        out["item"].append(ref.items())
        out["obs"].append(ref.obs())
        out["rng"].append(ref.streams())
        out["legal"].append(ref.legal())
        if s == S:
            break
        out["u"].append(ref.draws())
        r = ref.act(rows[s], masked=masked)
        for k in ("action", "pchoice", "reward", "done"):
            out[k].append(r[k])
    out = {k: np.stack(v) for k, v in out.items()}
    out["x_end"] = ref.rng.state
    return out
