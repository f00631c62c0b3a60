"""Host references for the learner's side of a window xh_venv_act recorded
(xh_venv_record_obs / xh_venv_record_ends / xh_venv_advantages): tests only,
plain numpy, no device.

The `_f32` functions restate the device's expressions (venv_gae_kernel,
venv_learn_kernels.hip) in numpy.float32 operations, one rounding per
operation; they are long_window_ref's gae_f32 / td_targets_f32 with the
reward an argument instead of `done ? 0 : 1` (test_venv_learn_ref.py holds
them to those bit for bit).  Arrays are step-major: reward / done / v_term /
adv [T][N], values [T+1][N]."""
import math

import numpy as np

import long_window_ref as lw

F32 = np.float32


# ---------------------------------------------------------- advantages ----
def gae_reward_f32(done, reward, values, gamma, lam):
    """lg = f32(lam) * f32(gamma); per env, t = T-1 .. 0: vn = done ? 0 :
    V_{t+1}, delta = (r + gamma * vn) - V_t, A = done ? delta : delta + lg *
    A; every operation rounded to float32."""
    d = np.asarray(done) != 0
    r = np.asarray(reward, F32)
    v = np.asarray(values, F32)
    T, N = d.shape
    assert v.shape == (T + 1, N) and r.shape == (T, N)
    g = F32(gamma)
    lg = F32(lam) * F32(gamma)
    assert type(lg) is F32
    adv = np.zeros((T, N), F32)
    A = np.zeros(N, F32)
    zero = F32(0)
    for t in range(T - 1, -1, -1):
        vn = np.where(d[t], zero, v[t + 1]).astype(F32)
        delta = (r[t] + g * vn) - v[t]
        A = np.where(d[t], delta, delta + lg * A)
        assert A.dtype == F32
        adv[t] = A
    return adv


def td_targets_reward_f32(done, reward, values, v_term, gamma):
    """target = r + gamma * (done ? v_term[t,e] : V_{t+1}), in float32
    operations; v_term None is a zero array."""
    d = np.asarray(done) != 0
    r = np.asarray(reward, F32)
    v = np.asarray(values, F32)
    T = d.shape[0]
    vt = np.zeros(d.shape, F32) if v_term is None else np.asarray(v_term, F32)
    assert v.shape[0] == T + 1 and vt.shape == d.shape == r.shape
    vn = np.where(d, vt, v[1:]).astype(F32)
    prod = F32(gamma) * vn
    out = r + prod
    assert prod.dtype == F32 and out.dtype == F32
    return out


def lambda_return_f32(adv, values):
    """A_t (un-normalised) + V(S_t): one float32 addition."""
    a = np.asarray(adv, F32)
    v = np.asarray(values, F32)
    out = a + v[:a.shape[0]]
    assert out.dtype == F32
    return out


def gae_reward_f64_forward(done, reward, values, gamma, lam):
    """long_window_ref.gae_f64_forward with the reward read: the reference's
    forward sum A_t = sum_i delta_i (lam gamma)^(i-t) over the rest of step
    t's segment, in float64 from the float32 inputs, with the float32
    constants gamma and lam gamma taken exactly.  Returns (A, S), S_t = sum_i
    (lam gamma)^(i-t) (|r_i| + gamma |V'_i| + |V_i|)."""
    d = np.asarray(done) != 0
    v = np.asarray(values, F32).astype(np.float64)
    r = np.asarray(reward, F32).astype(np.float64)
    T, N = d.shape
    assert v.shape == (T + 1, N) and r.shape == (T, N)
    g = float(F32(gamma))
    lg = float(F32(lam) * F32(gamma))
    vn = np.where(d, 0.0, v[1:])
    delta = r + g * vn - v[:T]
    mag = np.abs(r) + g * np.abs(vn) + np.abs(v[:T])
    # last step of the segment step t lies in: its terminal step, or T - 1
    end = np.zeros((T, N), np.int64)
    nxt = np.full(N, T - 1)
    for t in range(T - 1, -1, -1):
        nxt = np.where(d[t], t, nxt)
        end[t] = nxt
    coef = np.cumprod(np.concatenate([[1.0], np.full(max(T - 1, 0), lg)]))
    A = np.zeros((T, N), np.float64)
    S = np.zeros((T, N), np.float64)
    steps = np.arange(T)[:, None]
    for t in range(T):  # one forward sum per start step, every env at once
        hi = int(end[t].max()) + 1
        live = steps[t:hi] <= end[t][None, :]
        c = coef[:hi - t, None]
        A[t] = np.where(live, delta[t:hi] * c, 0.0).sum(axis=0)
        S[t] = np.where(live, mag[t:hi] * c, 0.0).sum(axis=0)
    return A, S


def stats_f64(adv, done):
    """[sum A, sum A^2, rows, ended rows] with exact sums (math.fsum) of the
    float32 advantages and of their exact squares."""
    a = np.asarray(adv, F32).astype(np.float64).ravel().tolist()
    return np.array([math.fsum(a), math.fsum(x * x for x in a), len(a),
                     int((np.asarray(done) != 0).sum())], np.float64)


def edge_done(T, N, seed):
    """done [T][N] uint8 with terminals on and beside every multiple of 8,
    counted from the window's start and from its end (the scan's chunks of 8
    start at step T - 1).  Env 0 never ends, env 1 ends on every step, envs 2
    .. 7 end on the steps t with t % 8 == 0 / 7 / 1 and (T - 1 - t) % 8 == 0 /
    7 / 1, env 8 on all of those, the rest on seeded random steps (one in
    four)."""
    g = np.random.default_rng(seed)
    t = np.arange(T)
    d = np.zeros((T, N), np.uint8)
    pats = [t % 8 == 0, t % 8 == 7, t % 8 == 1, (T - 1 - t) % 8 == 0,
            (T - 1 - t) % 8 == 7, (T - 1 - t) % 8 == 1]
    for e in range(N):
        if e == 0:
            continue
        if e == 1:
            d[:, e] = 1
        elif e < 8:
            d[:, e] = pats[e - 2]
        elif e == 8:
            d[:, e] = np.logical_or.reduce(pats)
        else:
            d[:, e] = g.random(T) < 0.25
    return d


# -------------------------------------------------------- observations ----
def state_rows(record, present_bins, present_items):
    """The STATE view: obs_f64 of slots 0 .. P (slot P the present state),
    [(P+1) N][B 2D]."""
    bins = np.concatenate([record["bins"], present_bins[None]])
    D = bins.shape[3]
    items = np.concatenate([record["items"][:, :, :D],
                            present_items[None][:, :, :D]])
    P1, N, B, _ = bins.shape
    return lw.obs_f64(bins.reshape(P1 * N, B, D), items.reshape(P1 * N, D))


def next_rows(record, present_state):
    """The NEXT view from numpy arrays: for transition q = t N + e the
    following slot's observation (slot P = present_state, a (bins [N][B][D],
    items [N][>=D]) pair) where done[q] == 0, and where the row ended the
    terminal view E_t: slot t's bins with bins[action] -= item, shown with
    slot t's item.  [P N][B 2D] float64."""
    pb, pi = present_state
    bins = np.asarray(record["bins"]).astype(np.int64)
    P, N, B, D = bins.shape
    items = np.asarray(record["items"]).astype(np.int64)[:, :, :D]
    done = np.asarray(record["done"]) != 0
    action = np.asarray(record["action"]).astype(np.int64)
    nb = np.concatenate([bins[1:], np.asarray(pb).astype(np.int64)[None]])
    ni = np.concatenate([items[1:],
                         np.asarray(pi).astype(np.int64)[None][:, :, :D]])
    for t in range(P):
        for e in range(N):
            if done[t, e]:
                eb = bins[t, e].copy()
                eb[action[t, e]] -= items[t, e]
                nb[t, e] = eb
                ni[t, e] = items[t, e]
    return lw.obs_f64(nb.reshape(P * N, B, D), ni.reshape(P * N, D))
