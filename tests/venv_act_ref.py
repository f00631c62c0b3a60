"""Host reference of xh_venv_act, built only from the oracle's primitives
(oracle.pyoracle: Rng.discrete / canonical, Env.apply / reset / obs, or_argmax,
minstd_jump): ONE engine seeded at state x0, Ng envs constructed in order,
every step visits every env in env order -- pick from the row the caller
supplies (policy_gradient_policy::react, policy_gradient.h:343-350), apply,
reset on game over (agent::step, rl.h:325-349).  CPU only.

Also the row generators the GPU tests share (mixed_rows, boundary_rows)."""
import numpy as np

from oracle import pyoracle as po


def argmax_first(row):
    row = np.ascontiguousarray(row, np.float32)
    return int(po.lib().or_argmax(po._ptr(row), len(row)))


class ActRef:
    """Ng agents on one engine; the envs [offset, offset + N) are kept."""

    def __init__(self, B, D, N, x0, policy_draws=2, n_global=None, offset=0):
        self.B, self.D, self.N = B, D, N
        self.Ng, self.offset, self.pd = n_global or N, offset, policy_draws
        self.k = policy_draws + 2
        self.cfg = po.env_cfg(B, D)
        self.rng = po.Rng(x0)
        self.envs = []
        for g in range(self.Ng):  # constructed one after another
            e = po.Env(self.cfg, self.rng)
            if offset <= g < offset + N:
                self.envs.append(e)

    # ---- what the device holds between two calls -----------------------
    def bins(self):
        return np.stack([e.bins for e in self.envs]).astype(np.int8)

    def items(self):
        return np.stack([e.item[:self.D] for e in self.envs]).astype(np.int8)

    def obs(self):
        return np.stack([e.obs() for e in self.envs]).reshape(
            self.N, self.B, 2 * self.D)

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
            env.apply(r[0])
            over = bool((env.bins < 0).any())
            out["reward"][e], out["done"][e] = (0.0 if over else 1.0), over
            if over:
                env.reset()
        return out

    def act(self, rows, mode="sample", refuse=()):
        """rows [N][B] float32 probabilities (values, for argmax).  An env in
        `refuse` is left untouched; the engine passes over its k draws."""
        rows = np.ascontiguousarray(rows, np.float32)

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


def run(B, D, N, x0, rows, mode="sample", policy_draws=2, n_global=None,
        offset=0):
    """rows [S][N][B].  Returns bins [S+1][N][B][D] / item [S+1][N][D] int8,
    obs [S+1][N][B][2D], rng [S+1][N], u [S][N] (the draws SAMPLE uses),
    action / pchoice / reward / done [S][N], x_end (the engine after step S)."""
    ref = ActRef(B, D, N, x0, policy_draws, n_global, offset)
    S = len(rows)
    out = {k: [] for k in ("bins", "item", "obs", "rng", "u", "action",
                           "pchoice", "reward", "done")}
    for s in range(S + 1):
        out["bins"].append(ref.bins())
        out["item"].append(ref.items())
        out["obs"].append(ref.obs())
        out["rng"].append(ref.streams())
        if s == S:
            break
        out["u"].append(ref.draws() if policy_draws == 2 else np.zeros(N))
        r = ref.act(rows[s], mode)
        for k in ("action", "pchoice", "reward", "done"):
            out[k].append(r[k])
    out = {k: np.stack(v) for k, v in out.items()}
    out["x_end"] = ref.rng.state
    return out


# ------------------------------------------------------------ row makers --
def mixed_rows(seed, S, N, B):
    """[S][N][B] float32: unnormalised positive rows, rows with zero entries,
    one-hot rows, and -- for every fourth env, at every step -- a row peaked
    at bin 0, so that env overflows its bin and is reset."""
    g = np.random.default_rng(seed)
    rows = np.zeros((S, N, B), np.float32)
    for s in range(S):
        for e in range(N):
            kind = 3 if e % 4 == 0 else int(g.integers(0, 3))
            if kind == 0:    # unnormalised, positive
                r = g.random(B) * 5.0 + 1e-3
            elif kind == 1:  # zero entries
                r = g.random(B) * (g.random(B) < 0.5)
                r[int(g.integers(0, B))] += 0.25
            elif kind == 2:  # one-hot
                r = np.zeros(B)
                r[int(g.integers(0, B))] = 1.0
            else:            # peaked at bin 0
                r = np.full(B, 0.03 / (B - 1))
                r[0] = 0.97
            rows[s, e] = r
    return rows


# the boundary test's venv: BOUNDARY_N envs on the engine at BOUNDARY_X0
BOUNDARY_N, BOUNDARY_X0 = 64, 20261


def boundary_rows(u, B):
    """The row whose second cumulative boundary is u up to rounding, and its
    neighbour with p1 moved one ulp to the other side of u: p0 = f32(u), p1 =
    f32(u - p0), p2 = f32(1 - p0 - p1), p3 = f32(1 - p0 - p1 - p2), the rest
    zero.  None when f32 rounding makes an entry negative (p0 above u) or
    one ulp of p1 does not cross u."""
    from sampling_ties import cumulative
    f = np.float32
    p0 = f(u)
    p1 = f(u - float(p0))
    p2 = f(1.0 - float(p0) - float(p1))
    p3 = f(1.0 - float(p0) - float(p1) - float(p2))
    if not (p0 > 0 and p1 > 0 and p2 > 0 and p3 >= 0):
        return None
    a = np.zeros(B, f)
    a[:4] = (p0, p1, p2, p3)
    ca = cumulative(a)[1]
    if ca == u:
        return None
    n = a.copy()
    n[1] = np.nextafter(p1, f(np.inf) if ca < u else f(0))
    cn = cumulative(n)[1]
    if not (n[1] > 0 and (ca - u) * (cn - u) < 0):
        return None
    return a, n
