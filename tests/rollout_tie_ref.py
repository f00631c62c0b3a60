"""Host reference of a trainer rollout window whose draws are PLACED next to the
boundaries of discrete_distribution's cumulative table, for the samplers' exact
path (the sequential restatement a sampler runs when a cumulative entry lies
within 1e-9 of the draw: sample_discrete / sample_step128_x / pack_step_groups).

Three parts, CPU only:

streams_for   the minstd states whose next canonical draw lies within `tol` of a
              target, on the side asked for.  A draw is u = ((x1 - 1) + (x2 - 1) R)
              / R^2 with x2 = 16807 x1 mod (2^31 - 1): the x2 around c R + 1 give
              draws 1 / R = 4.7e-10 apart, and the state two steps before x2 is
              x2 16807^-2.  Plain Python integers and floats restating
              canonical() of xh_device.h (tests/test_rollout_tie_ref.py holds it
              to the oracle's Rng.canonical bit for bit).
replay        a window on GIVEN distributions q[T][N][B] from given start states
              and per-env stream states: the pick is the oracle's Rng.discrete
              (libstdc++'s sequential result) on the row, p_old the row's entry,
              the transition the oracle's Env.apply / reset.  A trainer env owns
              its stream for the window: 4 draws per step, and after the window
              the state jumps over the other envs' 4 T (Ng - 1) draws
              (jump_mul, xylo_hip.cpp).
build / build_single   the arrangements of the GPU test
              (tests/test_gpu_rollout_ties.py): which env's draw goes next to
              which boundary of its own step-0 distribution."""
import math

import numpy as np

from sampling_ties import cumulative

from oracle import pyoracle as po

M = 2147483647          # minstd modulus
A = 16807               # minstd_rand0 multiplier
R = 2147483646.0        # the engine's range, max - min + 1
R2 = float(2147483646 ** 2)  # the double nearest R * R
A_INV2 = pow(A, -2, M)  # two steps back
TOL = 8e-10             # engineered draws: inside the samplers' 1e-9 by a margin
NEAR = 1e-9             # the samplers' threshold
CONTROL_MIN, CONTROL_MAX = 2e-9, 1e-6  # the controls: just outside the branch
FAR = 1e-4              # a wave neighbour that must not ask


def canonical(x):
    """(u, state after): std::generate_canonical<double, 53>(minstd_rand0) as
    xh_device.h's canonical() states it, the clamp below 1 included."""
    x1 = x * A % M
    x2 = x1 * A % M
    s = float(x1 - 1)
    s = s + float(x2 - 1) * R
    u = s / R2
    if u >= 1.0:
        u = math.nextafter(1.0, 0.0)
    return u, x2


def draw(x):
    return canonical(int(x))[0]


def _states_around(c, reach):
    """(|u - c|, u, state) of the draws whose second engine output lies within
    `reach` of c R + 1."""
    mid = int(c * R) + 1
    out = []
    for x2 in range(max(1, mid - reach), min(M - 1, mid + reach) + 1):
        x = x2 * A_INV2 % M
        u, end = canonical(x)
        assert end == x2
        out.append((abs(u - c), u, x))
    return out


def streams_for(c, side, tol=TOL):
    """The minstd states whose next canonical draw u has 0 < |u - c| < tol, with
    u < c (side "below") or u > c ("above"); the nearest first."""
    assert side in ("below", "above")
    reach = int(tol * R) + 3
    got = [(g, x) for g, u, x in _states_around(c, reach)
           if 0.0 < g < tol and (u < c) == (side == "below")]
    return [x for g, x in sorted(got)]


def boundaries(row):
    """libstdc++'s cumulative table of an f32 row (sampling_ties.cumulative)."""
    return cumulative(np.asarray(row, np.float32))


def pick_of(cp, u):
    """lower_bound(u) in the cumulative table."""
    return int(np.searchsorted(cp, u, side="left"))


def min_gap(cp, u):
    return float(np.abs(np.asarray(cp) - u).min())


def far_stream(cp, seed, lo=FAR, hi=None):
    """A stream state derived from `seed` whose next draw lies more than `lo`
    (and, if given, less than `hi`) from every boundary of cp."""
    x = int(seed) % M or 1
    for _ in range(100000):
        x = x * 48271 % M  # any walk over the states will do
        g = min_gap(cp, draw(x))
        if g > lo and (hi is None or g < hi):
            return x
    raise AssertionError("no stream found")


def control_stream(cp, k):
    """A state whose draw is between CONTROL_MIN and CONTROL_MAX from boundary k
    and from every other boundary at least CONTROL_MIN: just outside the
    branch."""
    for g, u, x in sorted(_states_around(float(cp[k]), 64)):
        if CONTROL_MIN < g < CONTROL_MAX and min_gap(cp, u) > CONTROL_MIN:
            return x
    return None


# ------------------------------------------------------------ arrangements --
def _target(cp, k, side):
    """The stream for boundary k of cp from `side`; the forced last entry 1.0 is
    reachable from below only: the largest draw there is, for both sides."""
    B = len(cp)
    if k == B - 1:
        xs = streams_for(1.0, "below")
        return max(xs, key=draw) if xs else None
    xs = streams_for(float(cp[k]), side)
    return xs[0] if xs else None


def _plan(N):
    return {"streams": np.zeros(N, np.uint32), "k": np.full(N, -1, np.int32),
            "side": np.zeros(N, np.int8),          # -1 below, +1 above, 0 none
            "engineered": np.zeros(N, bool), "control": np.zeros(N, bool),
            "u": np.zeros(N), "gap": np.zeros(N), "pick": np.zeros(N, np.int32),
            "missing": []}


def _finish(plan, q0):
    for e in range(len(q0)):
        cp = boundaries(q0[e])
        u = draw(plan["streams"][e])
        plan["u"][e], plan["gap"][e] = u, min_gap(cp, u)
        plan["pick"][e] = pick_of(cp, u)
    return plan


def no_draw_there(cp, k, side):
    """Whether the draws leave no room on that side of boundary k: below a
    boundary within NEAR of 0, above one within NEAR of 1 (rows with exact
    zeros at either end)."""
    return cp[k] < NEAR if side < 0 else cp[k] > 1.0 - NEAR


def build(q0):
    """The full arrangement on step-0 distributions q0 [N >= 2B + 2][B]: env 2k
    next to boundary k of its own row from below, env 2k + 1 from above (k = 0
    .. B - 1; both from below at the forced last entry), envs 2B and 2B + 1
    controls; what a trainer's env count adds beyond 2B + 2 free-runs far from
    every boundary.  plan["missing"] lists the envs no stream was found for
    (they free-run too)."""
    q0 = np.asarray(q0, np.float32)
    N, B = q0.shape
    assert N >= 2 * B + 2
    plan = _plan(N)
    for e in range(N):
        cp = boundaries(q0[e])
        if e < 2 * B:
            k, side = e // 2, ("below", "above")[e % 2]
            x = _target(cp, k, side)
            plan["k"][e], plan["side"][e] = k, (-1 if e % 2 == 0 or k == B - 1 else 1)
            plan["engineered"][e] = x is not None
        elif e < 2 * B + 2:
            k = (B // 2 - 1, B // 4)[e - 2 * B]
            x = control_stream(cp, k)
            plan["k"][e], plan["control"][e] = k, x is not None
        else:
            x = far_stream(cp, 104729 * (e + 1))
        if x is None:
            plan["missing"].append(e)
            x = far_stream(cp, 15485863 * (e + 1))
        plan["streams"][e] = x
    return _finish(plan, q0)


def build_single(q0, G, targets=None):
    """One env per wave of G envs next to a boundary, the others more than FAR
    from all of theirs: wave w's asking env is w * G + w % G, its boundary and
    side walk over the row (`targets`: the boundaries to use, default all but
    the last)."""
    q0 = np.asarray(q0, np.float32)
    N, B = q0.shape
    plan = _plan(N)
    ks = list(range(B - 1)) if targets is None else list(targets)
    for e in range(N):
        cp = boundaries(q0[e])
        w = e // G
        if e == w * G + w % G:
            k = ks[(w * 5) % len(ks)]
            side = ("below", "above")[w % 2]
            x = _target(cp, k, side)
            plan["k"][e], plan["side"][e] = k, (-1 if w % 2 == 0 else 1)
            plan["engineered"][e] = x is not None
            if x is None:
                plan["missing"].append(e)
                x = far_stream(cp, 15485863 * (e + 1))
        else:
            x = far_stream(cp, 7919 * (e + 1))
        plan["streams"][e] = x
    return _finish(plan, q0)


# ------------------------------------------------------------------ replay --
def _env(cfg, rng, bins, item):
    """An oracle Env in a given state on a given engine (nothing drawn)."""
    env = po.Env.__new__(po.Env)
    env.cfg, env.rng = cfg, rng
    env.bins = np.ascontiguousarray(bins, np.int32).reshape(cfg.B, cfg.D).copy()
    env.item = np.zeros(3, np.int32)
    env.item[:cfg.D] = np.asarray(item, np.int32).ravel()[:cfg.D]
    return env


def replay(B, D, bins0, item0, streams, q, n_global=None):
    """The window of T = len(q) steps on the distributions q [T][N][B] (float32,
    as a device recorded them) from the states bins0 [N][B][D], item0 [N][>= D]
    and the stream states streams [N].  Returns action [T][N] int32, pold
    [T][N] float32 (q at the pick, its bits), done [T][N] uint8, bins
    [T + 1][N][B][D] / items [T + 1][N][D] int8 (slot 0 = the start), u [T][N]
    (the picks' draws) and rng [N] uint32, the stream states after the
    window."""
    q = np.ascontiguousarray(q, np.float32)
    T, N, _ = q.shape
    Ng = n_global or N
    cfg = po.env_cfg(B, D)
    out = {"action": np.zeros((T, N), np.int32), "pold": np.zeros((T, N), np.float32),
           "done": np.zeros((T, N), np.uint8), "u": np.zeros((T, N)),
           "bins": np.zeros((T + 1, N, B, D), np.int8),
           "items": np.zeros((T + 1, N, D), np.int8), "rng": np.zeros(N, np.uint32)}
    for e in range(N):
        rng = po.Rng(int(streams[e]))
        env = _env(cfg, rng, bins0[e], item0[e])
        out["bins"][0, e], out["items"][0, e] = env.bins, env.item[:D]
        for t in range(T):
            out["u"][t, e] = po.Rng(rng.state).canonical()
            c = rng.discrete(q[t, e])
            out["action"][t, e], out["pold"][t, e] = c, q[t, e, c]
            env.apply(c)
            over = bool((env.bins < 0).any())
            out["done"][t, e] = over
            if over:
                env.reset()
            out["bins"][t + 1, e], out["items"][t + 1, e] = env.bins, env.item[:D]
        assert rng.state == po.minstd_jump(int(streams[e]), 4 * T)  # 4 draws a step
        out["rng"][e] = po.minstd_jump(rng.state, 4 * T * (Ng - 1))
    return out
