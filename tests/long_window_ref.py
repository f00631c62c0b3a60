"""Host references for the learner's value / advantage chain over a rollout
window of any length T (tests only, plain numpy, no device, no oracle).

Arrays are step-major as the device buffers are: done / action / v_term /
targets / adv [T][N], v_state [T+1][N], bins [T+1][N][B][D], items
[T+1][N][>=D].  test_long_window_ref.py pins every function here against the
CPU oracle before a GPU test relies on it.

Two kinds of reference:

* the `_f32` functions restate a kernel's expression in numpy.float32
  operations, one rounding per operation, which is what the device does under
  `#pragma clang fp contract(off)` (value_kernels.hip): the kernels are held
  to them bit for bit;
* the `_f64` functions are the reference learner's own statement in float64
  from float32 inputs: the kernels are held to them within a stated bound.
"""
import math

import numpy as np

F32 = np.float32
U32 = 2.0 ** -24  # unit roundoff of float32
CAP = 8           # bin capacity (bin_packing.h:48): observations are x / 8


# ------------------------------------------------------------- targets ----
def td_targets_f32(done, v_state0, v_term, gamma):
    """value_targets_kernel: reward = done ? 0 : 1, vn = done ? v_term[t,e]
    : v_state0[t+1,e], target = reward + gamma * vn, in float32 operations.
    Entries of v_term where done == 0 are never used."""
    d = np.asarray(done) != 0
    v0 = np.asarray(v_state0, F32)
    vt = np.asarray(v_term, F32)
    T = d.shape[0]
    assert v0.shape[0] == T + 1 and vt.shape == d.shape
    reward = np.where(d, F32(0), F32(1)).astype(F32)
    vn = np.where(d, vt, v0[1:]).astype(F32)
    prod = F32(gamma) * vn
    out = reward + prod
    assert prod.dtype == F32 and out.dtype == F32
    return out


# ----------------------------------------------------------------- GAE ----
def gae_f32(done, v_state, gamma, lam):
    """gae_kernel's documented arithmetic with no chunking: lg = f32(lam) *
    f32(gamma); per env, t = T-1 .. 0: vn = done ? 0 : V_{t+1}, delta =
    (reward + gamma * vn) - V_t, A = done ? delta : delta + lg * A; every
    operation rounded to float32."""
    d = np.asarray(done) != 0
    v = np.asarray(v_state, F32)
    T, N = d.shape
    assert v.shape == (T + 1, N)
    g = F32(gamma)
    lg = F32(lam) * F32(gamma)
    assert type(lg) is F32
    adv = np.zeros((T, N), F32)
    A = np.zeros(N, F32)
    one, zero = F32(1), F32(0)
    for t in range(T - 1, -1, -1):
        reward = np.where(d[t], zero, one).astype(F32)
        vn = np.where(d[t], zero, v[t + 1]).astype(F32)
        delta = (reward + g * vn) - v[t]
        A = np.where(d[t], delta, delta + lg * A)
        assert A.dtype == F32
        adv[t] = A
    return adv


def gae_f64_forward(done, v_state, gamma, lam):
    """calculate_advantage as the reference states it (policy_gradient.h:
    220-281): V(terminal end row) = 0, delta_i = r_i + gamma V'_i - V_i, and
    the forward sum A_t = sum_i delta_i (lam gamma)^(i-t) over the rest of
    step t's segment (up to its terminal step, or the window's last step), in
    float64 from the float32 inputs.  gamma and lam gamma are the float32
    constants the reference holds (`const float lg = lambda * gamma`), taken
    exactly, so the result measures the arithmetic and not the constants.

    Returns (A, S): S_t = sum_i (lam gamma)^(i-t) (|r_i| + gamma |V'_i| +
    |V_i|), the magnitude the rounding errors of a float32 evaluation scale
    with."""
    d = np.asarray(done) != 0
    v = np.asarray(v_state, F32).astype(np.float64)
    T, N = d.shape
    assert v.shape == (T + 1, N)
    g = float(F32(gamma))
    lg = float(F32(lam) * F32(gamma))
    reward = np.where(d, 0.0, 1.0)
    vn = np.where(d, 0.0, v[1:])
    delta = reward + g * vn - v[:T]
    mag = np.abs(reward) + g * np.abs(vn) + np.abs(v[:T])
    A = np.zeros((T, N), np.float64)
    S = np.zeros((T, N), np.float64)
    for t in range(T):
        live = np.ones(N, bool)  # env's segment from t still running at i
        coef = 1.0
        for i in range(t, T):
            A[t] += np.where(live, delta[i] * coef, 0.0)
            S[t] += np.where(live, mag[i] * coef, 0.0)
            live &= ~d[i]
            if not live.any():
                break
            coef *= lg
    return A, S


def adv_normalize_f64(A, count):
    """(A - mean) / (sqrt(var) + 1e-8) with the population mean and variance
    over `count` rows in float64 (exact sums), rounded once to float32."""
    a = np.asarray(A, F32).astype(np.float64)
    flat = a.ravel().tolist()
    mean = math.fsum(flat) / count
    var = math.fsum((x - mean) * (x - mean) for x in flat) / count
    return ((a - mean) / (math.sqrt(max(var, 0.0)) + 1e-8)).astype(F32)


# ------------------------------------------------------ terminal views ----
def terminal_views(bins, items, action, done):
    """The states E_t the value net sees for the ended transitions: the
    state after the env applied the action and before it reset (agent::step,
    rl.h:336-343; oracle.c agent_step's `curr`).  From the device buffers:
    slot t's bins with the chosen bin reduced by slot t's item, shown with
    slot t's item -- the overflowing apply returns before it draws
    (bin_packing.h:53-64; or_env_apply), so the item of slot t + 1 (drawn by
    the reset) is not in it.  test_long_window_ref.py confirms this against
    the oracle's own end rows.

    Returns (t, e, bins_E [n][B][D], items_E [n][D]), transitions in env-major
    order (e ascending, then t)."""
    d = np.asarray(done) != 0
    T, N = d.shape
    b = np.asarray(bins).astype(np.int64)
    D = b.shape[3]
    it = np.asarray(items).astype(np.int64)[:, :, :D]
    e, t = np.nonzero(d.T)
    a = np.asarray(action).astype(np.int64)[t, e]
    eb = b[t, e].copy()
    ei = it[t, e].copy()
    eb[np.arange(len(t)), a] -= ei
    return t, e, eb, ei


def obs_f64(bins, items):
    """observation::to_vector (bin_packing.h:31-40; or_obs): per bin
    [bin / cap, item / cap]; bins [rows][B][D], items [rows][>=D] ->
    [rows][B * 2D] float64 (eighths: exact)."""
    b = np.asarray(bins).astype(np.float64)
    rows, B, D = b.shape
    it = np.asarray(items).astype(np.float64)[:, :D]
    out = np.empty((rows, B, 2 * D), np.float64)
    out[:, :, :D] = b / CAP
    out[:, :, D:] = it[:, None, :] / CAP
    return out.reshape(rows, B * 2 * D)


# ----------------------------------------------------------- value net ----
def value_f64(params, obs, widths=(64, 32)):
    """The value MLP (B * 2D -> 64 -> 32 -> 1, full layers with relu between,
    ppo_training.cc:19-26) in float64; params in model::parameters() order:
    per layer A (out x in, row-major) then b (out)."""
    x = np.asarray(obs, np.float64)
    p = np.asarray(params, F32).astype(np.float64)
    sizes = [x.shape[1]] + list(widths) + [1]
    off = 0
    for k, (fi, fo) in enumerate(zip(sizes[:-1], sizes[1:])):
        W = p[off:off + fo * fi].reshape(fo, fi)
        off += fo * fi
        bias = p[off:off + fo]
        off += fo
        x = x @ W.T + bias
        if k < len(sizes) - 2:
            x = np.maximum(x, 0.0)
    assert off == p.size, (off, p.size)
    return x[:, 0]


def value_params(B, D, widths=(64, 32), seed=4):
    """Value-net parameters for these tests: weights N(0, sqrt(2 / fan_in)),
    biases N(0, 0.1).  The library's default initialisation (N(0, 0.01), zero
    biases) gives |V| of about 1e-4, under which the parity tolerance 1e-4
    max(1, |V|) cannot tell one state's value from another's; with these V is
    of order 1 and differs from state to state by far more than the
    tolerance (assert_values_differ)."""
    rng = np.random.default_rng(seed)
    sizes = [B * 2 * D] + list(widths) + [1]
    parts = []
    for fi, fo in zip(sizes[:-1], sizes[1:]):
        parts.append(rng.normal(0.0, np.sqrt(2.0 / fi), fo * fi))
        parts.append(rng.normal(0.0, 0.1, fo))
    return np.concatenate(parts).astype(F32)


def assert_values_differ(v, tol, what=""):
    """A condition on the inputs: a value landing on its neighbour's place
    would be caught, i.e. most neighbours in `v` differ by more than 10 times
    the tolerance."""
    v = np.asarray(v, np.float64).ravel()
    if v.size < 2:
        return
    gap = np.abs(v - np.roll(v, 1)) / np.maximum(1.0, np.abs(v))
    assert (gap > 10 * tol).mean() >= 0.5, (what, float(np.median(gap)))


# ------------------------------------------------------------- density ----
def density(done):
    """(share of terminal transitions, episodes ended per env [N])."""
    d = np.asarray(done) != 0
    return float(d.mean()), d.sum(axis=0)


def assert_dense(done, what="", every_env=True):
    """A window stays terminal-dense: at least 15% of the transitions end an
    episode and, from T = 9 on, every env ends at least two (an episode
    under forced action 0 lasts 3 to 5 steps, so at T = 9 that depends on the
    seed: every_env=False, for batches of hundreds of envs, asks it of most
    envs and one episode of all)."""
    share, per_env = density(done)
    assert share >= 0.15, (what, "terminal share", share)
    if np.asarray(done).shape[0] >= 9:
        if every_env:
            assert per_env.min() >= 2, (what, "episodes per env", per_env.min())
        else:
            assert per_env.min() >= 1 and (per_env >= 2).mean() >= 0.5, (
                what, "episodes per env", np.bincount(per_env))
    return share, per_env


def ulp_distance_f32(x, y):
    """|x - y| in float32 units in the last place (finite inputs)."""
    def key(a):
        i = np.ascontiguousarray(a, F32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(x) - key(y))
