"""GPU tests of the VecEnv's episode statistics (xh_venv_set_episode_stats):
the counting inside the step / act / apply launches, the row kernel and its
ring, the per-env state and the state rules -- against tests/venv_episode_ref.py
(pinned on the CPU by tests/test_venv_episode_ref.py).  Every assertion on a
row or a per-env array is exact equality.

Where no env is refused the done / live history is ActRef's (tests/venv_act_
ref.py), computed before the device runs; where a call refuses an env (its
stream then stays behind ActRef's) or applies a masked subset, the history is
the call's own XH_VENV_DONE with the live set the test chose.

Shapes: N = 70 envs as in tests/test_gpu_venv_mask.py, which fills the last
wave at no shape; the sampling case runs over every B in {8, 16, 32, 64, 128}
x D in {1, 2, 3}, the others at (8, 1), (64, 2) and (128, 3); the reduction
case takes N = 1030 (five row-kernel workgroups, the last one of 6 envs)."""
import ctypes
import functools

import numpy as np
import pytest

import venv_episode_ref as er
from venv_act_ref import ActRef, mixed_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
N, X0 = 70, 4242
SHAPES = [(B, D) for B in (8, 16, 32, 64, 128) for D in (1, 2, 3)]
SHAPE_IDS = ["B%d-D%d" % s for s in SHAPES]
FEW = [(8, 1), (64, 2), (128, 3)]
FEW_IDS = ["B%d-D%d" % s for s in FEW]


def _venv(ctx, B, D, n=N, x0=X0):
    from dependence_free_rl_amd import VecEnv
    return VecEnv(ctx, num_envs=n, bins=B, dims=D, rng_state=x0)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _same_rows(got, want, what):
    """Exact equality of rows, a NaN equal to a NaN."""
    assert got.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got, want, equal_nan=True), \
        "%s\n%s\n%s" % (what, got, want)


def _check(env, rows, running, first, what):
    _same_rows(env.episode_stats(0, len(rows)), rows, what + ": rows")
    r, f = env.episode_state()
    _same(r, running, what + ": running")
    _same(f, first, what + ": first")
    _same(env.first_episode_lengths(), first[first >= 0], what + ": firsts")


def _drain(env, word):
    """Synchronise; True where the call reports (and clears) an error whose
    message holds `word`."""
    from dependence_free_rl_amd import XhError, _lib
    try:
        env.synchronize()
    except XhError as e:
        assert "status %d" % _lib.XH_ERR_INVALID in str(e) and word in str(e)
        return True
    return False


def _facts(done, live, points):
    """What the history holds, from the reference alone: an env with two or
    more episodes inside one row's span, an env with no finished episode, an
    episode that begins in one span and ends in a later one."""
    S, n = done.shape
    span = lambda c: sum(1 for p in points if p <= c)  # noqa: E731
    two = none = cross = False
    for e in range(n):
        ends, start, seen = [], None, {}
        for c in range(S):
            if not live[c, e]:
                continue
            start = c if start is None else start
            if done[c, e]:
                ends.append(c)
                seen[span(c)] = seen.get(span(c), 0) + 1
                cross |= span(start) != span(c)
                start = None
        two |= any(k >= 2 for k in seen.values())
        none |= not ends
    return {"two": two, "none": none, "cross": cross}


def _run_act(env, rows, points, kind="probs", mode="sample"):
    pts = list(points)
    for s in range(len(rows) + 1):
        while pts and pts[0] == s:
            env.episode_row()
            pts.pop(0)
        if s < len(rows):
            env.act(rows[s], kind=kind, mode=mode, fetch=False)
    env.synchronize()


# --------------------------------------------------------------------- 1 --
S_ACT, POINTS_ACT = 24, [3, 4, 11, 24]


@functools.lru_cache(maxsize=None)
def _ref_act(B, D):
    rows = mixed_rows(11 * B + D, S_ACT, N, B)
    done, live = er.act_history(ActRef(B, D, N, X0), rows)
    want = er.rows_of_history(done, live, POINTS_ACT)[:3]
    return rows, done, live, want


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_act_sampling(ctx, shape):
    """24 sampled steps of mixed_rows (every fourth env overflows bin 0 again
    and again), rows after 3, 4, 11 and 24 calls: the rows and both per-env
    arrays are the restatement's on ActRef's history, with the trajectory
    record off and on, and at 64 bins also with the distribution record (the
    RD instantiation)."""
    B, D = shape
    rows, done, live, want = _ref_act(B, D)
    facts = _facts(done, live, POINTS_ACT)
    assert facts["two"] and facts["cross"]
    if B >= 16:
        assert facts["none"]                   # an env that never finishes
    arms = ["off", "record"] + (["distrib"] if shape == (64, 2) else [])
    for arm in arms:
        env = _venv(ctx, B, D)
        if arm != "off":
            env.set_record(S_ACT, states=(arm == "distrib"),
                           distrib=(arm == "distrib"))
        env.set_episode_stats(8)
        _run_act(env, rows, POINTS_ACT)
        _check(env, *want, what=arm)
        assert env.episode_count() == len(POINTS_ACT)
        if arm != "off":
            _same(env.record()["done"].astype(bool), done, "the history")
        env.close()


def test_episode_curve(ctx):
    """The derived series: means and deviations from the sums, returns =
    lengths - 1, NaN where a row has no episode."""
    B, D = 8, 2
    rows, done, live, want = _ref_act(B, D)
    env = _venv(ctx, B, D)
    env.set_episode_stats(8)
    _run_act(env, rows, [0] + POINTS_ACT)
    c = env.episode_curve()
    r = want[0]
    assert c["episodes"].tolist() == [0.0] + r[:, er.EPISODES].tolist()
    assert np.isnan(c["len_mean"][0]) and np.isnan(c["return_mean"][0])
    assert np.isnan(c["first_len_mean"][0])
    k = 3                                      # the row after 11 calls
    lens = [n for e in range(N) for n in _lengths_in(done, live, e, 4, 11)]
    assert c["episodes"][k] == len(lens) > 0
    assert c["len_mean"][k] == np.mean(lens)
    assert c["return_mean"][k] == np.mean(lens) - 1.0
    assert abs(c["len_std"][k] - np.std(lens)) < 1e-9
    assert c["len_min"][k] == min(lens) and c["return_max"][k] == max(lens) - 1
    first = want[2]
    assert c["envs_finished"][-1] == (first >= 0).sum()
    assert c["first_len_mean"][-1] == first[first >= 0].mean()
    assert abs(c["first_len_std"][-1] - first[first >= 0].std()) < 1e-9
    env.close()


def _lengths_in(done, live, e, lo, hi):
    """The lengths of env e's episodes that end at calls [lo, hi)."""
    out, n = [], 0
    for c in range(hi):
        if live[c, e]:
            n += 1
            if done[c, e]:
                if c >= lo:
                    out.append(n)
                n = 0
    return out


# --------------------------------------------------------------------- 2 --
@functools.lru_cache(maxsize=None)
def _ref_masked(B, D):
    S = 40 if B == 8 else 12
    points = [1, 17, S] if B == 8 else [1, 5, S]
    g = np.random.default_rng(500 + B)
    rows = (g.random((S, N, B)) + 0.05).astype(f32)
    done, live = er.act_history(ActRef(B, D, N, X0), rows, masked=True)
    return rows, points, done, live, er.rows_of_history(done, live, points)[:3]


@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_act_masked(ctx, shape):
    """With the action mask on an episode lasts until nothing fits: at 8 bins
    40 steps hold ends, and episodes that outlive a row's span; at 64 and 128
    bins 12 steps hold none.  The first row, after one step, shows no episode
    and NaN min / max."""
    B, D = shape
    rows, points, done, live, want = _ref_masked(B, D)
    r = want[0]
    assert r[0, er.EPISODES] == 0 and r[0, er.CALLS] == 1
    assert np.isnan(r[0, er.LEN_MIN]) and np.isnan(r[0, er.LEN_MAX])
    assert r[0, er.RUNNING_SUM] == N and r[0, er.RUNNING_MAX] == 1
    if B == 8:
        assert _facts(done, live, points)["cross"]
        assert r[1:, er.EPISODES].sum() > 0 and r[2, er.LEN_MAX] > 16
    else:
        assert done.sum() == 0 and r[2, er.RUNNING_SUM] == 12 * N
    env = _venv(ctx, B, D)
    env.set_action_mask(True)
    env.set_episode_stats(4)
    _run_act(env, rows, points)
    _check(env, *want, what="masked")
    env.close()


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_act_with_refused_rows(ctx, shape):
    """A NaN row (env 9 at step 2, env 4 at step 5) and a zero-sum row (env 9
    at step 3): those envs take no step there and their counts do not move;
    the other envs' verdicts are ActRef's."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    S, points = 10, [4, 10]
    rows = mixed_rows(21 * B + D, S, N, B)
    refuse = {2: {9}, 3: {9}, 5: {4}}
    rows[2, 9, B - 1] = np.nan
    rows[3, 9] = 0
    rows[5, 4, 0] = np.nan
    ref_done, _ = er.act_history(ActRef(B, D, N, X0), rows, refuse=refuse)
    env = _venv(ctx, B, D)
    env.set_episode_stats(4)
    ref, want_rows, pts = er.EpisodeRef(N), [], list(points)
    for s in range(S):
        before = env.episode_state()
        env.act(rows[s], fetch=False)
        assert _drain(env, "refused") == (s in refuse)
        live = np.ones(N, bool)
        live[list(refuse.get(s, ()))] = False
        done = env.get(_lib.VENV_DONE).astype(bool)
        assert not done[~live].any()
        ref.call(live, done)
        after = env.episode_state()
        for e in refuse.get(s, ()):
            assert after[0][e] == before[0][e] and after[1][e] == before[1][e]
        if pts and pts[0] == s + 1:
            env.episode_row()
            want_rows.append(ref.row())
            pts.pop(0)
        keep = np.ones(N, bool)                 # never refused so far
        keep[[e for t in refuse if t <= s for e in refuse[t]]] = False
        _same(done[keep], ref_done[s][keep], "ActRef's verdicts %d" % s)
    assert want_rows[1][er.CALLS] == 6
    _check(env, np.array(want_rows), ref.running, ref.first, "refused rows")
    env.close()


# --------------------------------------------------------------------- 4 --
@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_step_with_an_out_of_range_action(ctx, shape):
    """xh_venv_step on the caller's actions (bin 0 for every third env, so
    episodes end); at step 3 env 5's action is B, written past the host-side
    check: the env is not counted and the call reports it."""
    from dependence_free_rl_amd import _lib
    from test_gpu_venv_loss import Dev
    B, D = shape
    S, bad_s, bad_e = 9, 3, 5
    g = np.random.default_rng(40 + B)
    dev = Dev(ctx)
    env = _venv(ctx, B, D)
    env.set_episode_stats(4)
    ref, want_rows = er.EpisodeRef(N), []
    for s in range(S):
        a = g.integers(0, B, N).astype(np.int32)
        a[::3] = 0
        live = np.ones(N, bool)
        env.set_actions(a)
        if s == bad_s:
            a[bad_e] = B
            live[bad_e] = False
            dev.put(a, ptr=env.device_ptr(_lib.VENV_ACTIONS))
        before = env.episode_state()
        env.step(fetch=False)
        assert _drain(env, "outside") == (s == bad_s)
        done = env.get(_lib.VENV_DONE).astype(bool)
        assert not done[~live].any()
        ref.call(live, done)
        if s == bad_s:
            after = env.episode_state()
            assert after[0][bad_e] == before[0][bad_e]
            assert after[1][bad_e] == before[1][bad_e]
        if s in (bad_s, S - 1):
            env.episode_row()
            want_rows.append(ref.row())
    want = np.array(want_rows)
    assert want[:, er.EPISODES].sum() > 0
    _check(env, want, ref.running, ref.first, "step")
    dev.ptrs = []                              # the venv's own buffer
    env.close()


# --------------------------------------------------------------------- 5 --
@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_apply_reset_and_set(ctx, shape):
    """xh_venv_apply counts its masked envs alone and ends the episode where
    it reports game over, so the reset that follows changes no count;
    reset(mask) zeroes running lengths without counting an episode;
    set(VENV_BINS) zeroes every running length, set(VENV_ITEMS) and
    set(VENV_RNG) none."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    S = 14
    g = np.random.default_rng(70 + B)
    env = _venv(ctx, B, D)
    env.set_episode_stats(4)
    ref = er.EpisodeRef(N)
    ends = 0
    for s in range(S):
        a = g.integers(0, B, N).astype(np.int32)
        a[::2] = 0                             # these envs overflow bin 0
        mask = g.random(N) < 0.6
        env.set_actions(a)
        done = env.apply(mask).astype(bool)
        assert not done[~mask].any()
        ref.call(mask, done)
        ends += int(done.sum())
        if done.any():
            state = env.episode_state()
            assert (state[0][done] == 0).all()
            env.reset(done)                    # the caller's reset
            ref.restart(done)
            _same(env.episode_state()[0], state[0], "reset after game over")
    assert ends > 0 and (ref.running > 0).any()
    env.episode_row()
    rows = [ref.row()]
    assert rows[0][er.EPISODES] == ends and rows[0][er.CALLS] == S
    _check(env, np.array(rows), ref.running, ref.first, "apply")
    # reset(mask): the abandoned episodes are not counted
    sel = (np.arange(N) % 3 == 0) & (ref.running > 0)
    assert sel.any() and (ref.running[~sel] > 0).any()
    env.reset(sel)
    ref.restart(sel)
    env.episode_row()
    rows.append(ref.row())
    assert rows[1][er.EPISODES] == 0 and rows[1][er.CALLS] == 0
    _check(env, np.array(rows), ref.running, ref.first, "reset(mask)")
    # ITEMS and RNG change no count, BINS zeroes every running length
    env.set(_lib.VENV_ITEMS, env.get(_lib.VENV_ITEMS))
    env.set(_lib.VENV_RNG, env.get(_lib.VENV_RNG))
    _same(env.episode_state()[0], ref.running, "after ITEMS / RNG")
    assert ref.running.any()
    env.set(_lib.VENV_BINS, env.get(_lib.VENV_BINS))
    ref.restart()
    env.episode_row()
    rows.append(ref.row())
    assert rows[2][er.RUNNING_SUM] == 0
    assert rows[2][er.ENVS_FINISHED] == rows[0][er.ENVS_FINISHED] > 0
    _check(env, np.array(rows), ref.running, ref.first, "set(BINS)")
    env.close()


# --------------------------------------------------------------------- 6 --
BUFS = ("VENV_ACTIONS", "VENV_REWARD", "VENV_DONE", "VENV_BINS", "VENV_ITEMS",
        "VENV_RNG", "VENV_OBS", "VENV_MASK", "VENV_POLICY", "VENV_PCHOICE")


@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_statistics_perturb_nothing(ctx, shape):
    """Two venvs from one seed, statistics on in one: after the same act
    (recorded, with states and distributions), step, apply and reset calls
    every XH_VENV_* buffer and every record array is byte-identical.  With
    statistics off, the row call is XH_ERR_STATE and the arrays have 0
    bytes."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    lib = _lib.lib
    T = 6
    rows = mixed_rows(33 * B + D, T, N, B)
    g = np.random.default_rng(90 + B)
    acts = g.integers(0, B, (4, N)).astype(np.int32)
    acts[:, ::2] = 0
    masks = g.random((4, N)) < 0.5
    a, b = _venv(ctx, B, D), _venv(ctx, B, D)
    a.set_episode_stats(4)
    n = ctypes.c_long()
    assert lib.xh_venv_episode_row(b.h) == _lib.XH_ERR_STATE
    assert lib.xh_venv_episode_count(b.h, ctypes.byref(n)) == \
        _lib.XH_ERR_STATE
    assert lib.xh_venv_get_episode_rows(b.h, 0, 0, None) == _lib.XH_ERR_STATE
    for which in (_lib.VEPS_RUNNING, _lib.VEPS_FIRST):
        assert lib.xh_venv_episode_bytes(b.h, which) == 0
        assert lib.xh_venv_episode_ptr(b.h, which) is None
        assert lib.xh_venv_episode_bytes(a.h, which) == 4 * N
        assert lib.xh_venv_episode_ptr(a.h, which)
    for which in (-1, _lib.VEPS_COUNT):
        assert lib.xh_venv_episode_bytes(a.h, which) == 0
        assert lib.xh_venv_episode_ptr(a.h, which) is None
    for env in (a, b):
        env.set_record(T, states=True, distrib=True)
        for t in range(T):
            env.act(rows[t], write_obs=True, fetch=False)
        env.set_actions(acts[0])
        env.step(write_obs=True, fetch=False)
        env.set_actions(acts[1])
        env.step(fetch=False)
        env.set_actions(acts[2])
        env.apply(masks[0])
        env.reset(masks[1])
        env.set_actions(acts[3])
        env.apply()
        env.synchronize()
    a.episode_row()
    for name in BUFS:
        which = getattr(_lib, name)
        _same(a.get(which), b.get(which), name)
    ra, rb = a.record(), b.record()
    assert sorted(ra) == sorted(rb) and len(ra) == 7
    for k in rb:
        _same(ra[k], rb[k], "record %s" % k)
    row = a.episode_stats()[0]
    assert row[er.CALLS] == T + 4 and row[er.EPISODES] > 0
    # switched off again: everything is gone
    a.set_episode_stats(0)
    assert lib.xh_venv_episode_row(a.h) == _lib.XH_ERR_STATE
    assert lib.xh_venv_episode_bytes(a.h, _lib.VEPS_RUNNING) == 0
    a.close()
    b.close()


# --------------------------------------------------------------------- 7 --
def test_ring(ctx):
    """history_rows = 3 and five rows: the last three are right, an
    overwritten row and an unwritten one are XH_ERR_INVALID, the count is 5;
    the row launch is one timed bracket; switching on again restarts rows and
    lengths, and first_len goes back to -1."""
    from dependence_free_rl_amd import _lib
    B, D = 8, 2
    lib = _lib.lib
    rows, done, live, _ = _ref_act(B, D)
    points = [2, 6, 9, 15, 24]
    want, running, first, _ = er.rows_of_history(done, live, points)
    assert (want[2:, er.EPISODES] > 0).all()
    env = _venv(ctx, B, D)
    assert lib.xh_venv_set_episode_stats(env.h, -1) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_set_episode_stats(env.h, (1 << 20) + 1) == \
        _lib.XH_ERR_INVALID
    env.set_episode_stats(3)
    _run_act(env, rows, points)
    assert env.episode_count() == 5
    _same_rows(env.episode_stats(), want[2:], "the ring's rows")
    _same_rows(env.episode_stats(first=3, count=2), want[3:], "rows 3, 4")
    _same_rows(env.episode_stats(count=1), want[4:], "the last row")
    buf = np.zeros((3, er.COUNT))
    for first_row, count in ((1, 1), (0, 3), (1, 3), (5, 1), (3, 3), (-1, 1)):
        assert lib.xh_venv_get_episode_rows(
            env.h, first_row, count, buf.ctypes.data) == _lib.XH_ERR_INVALID
    assert lib.xh_venv_get_episode_rows(env.h, 1, 1, buf.ctypes.data)
    assert b"overwritten" in lib.xh_last_error()
    r, f = env.episode_state()
    _same(r, running, "running")
    _same(f, first, "first")
    assert (f >= 0).any()
    # wrong sizes and values of the per-env arrays
    assert lib.xh_venv_episode_get(env.h, 0, r.ctypes.data, 4 * N - 4) == \
        _lib.XH_ERR_INVALID
    assert lib.xh_venv_episode_get(env.h, 2, r.ctypes.data, 4 * N) == \
        _lib.XH_ERR_INVALID
    neg = np.full(N, -2, np.int32)
    assert lib.xh_venv_episode_set(env.h, 1, neg.ctypes.data, 4 * N) == \
        _lib.XH_ERR_INVALID
    # the row launch under xh_venv_set_timing
    env.set_timing(True)
    env.episode_row()
    ms, launches = env.kernel_time()
    env.set_timing(False)
    assert launches == 1 and ms > 0
    assert env.episode_count() == 6
    # switched on again
    env.set_episode_stats(2)
    assert env.episode_count() == 0
    assert env.episode_stats().shape == (0, er.COUNT)
    r, f = env.episode_state()
    assert not r.any() and (f == -1).all()
    assert lib.xh_venv_get_episode_rows(env.h, 0, 1, buf.ctypes.data) == \
        _lib.XH_ERR_INVALID
    env.episode_row()
    row = env.episode_stats()
    zero = np.zeros(er.COUNT)
    zero[[er.LEN_MIN, er.LEN_MAX]] = np.nan
    _same_rows(row, zero[None], "the fresh ring's first row")
    n = ctypes.c_long(-1)
    assert lib.xh_venv_episode_count(env.h, ctypes.byref(n)) == 0
    assert n.value == 1
    env.close()


# --------------------------------------------------------------------- 8 --
N_BIG, S_BIG, POINTS_BIG = 1030, 10, [4, 10]


@functools.lru_cache(maxsize=None)
def _ref_big():
    g = np.random.default_rng(8)
    actions = g.integers(0, 2, (S_BIG, N_BIG)).astype(np.int32)
    done, live = er.step_history(ActRef(8, 1, N_BIG, X0), actions)
    return actions, done, er.rows_of_history(done, live, POINTS_BIG)[:3]


def test_multi_workgroup_reduction(ctx):
    """N = 1030 at 8 bins, 1-D: five row-kernel workgroups of 256 envs, the
    last one of 6; 10 steps through xh_venv_step onto bins 0 and 1, so
    episodes end in every workgroup's range."""
    actions, done, want = _ref_big()
    blocks = {e // 256 for e in np.flatnonzero(done.any(axis=0))}
    assert len(blocks) >= 3 and 4 in blocks
    assert want[0][:, er.EPISODES].min() > 0
    env = _venv(ctx, 8, 1, n=N_BIG)
    env.set_episode_stats(2)
    pts = list(POINTS_BIG)
    for s in range(S_BIG):
        env.set_actions(actions[s])
        env.step(fetch=False)
        if pts and pts[0] == s + 1:
            env.episode_row()
            pts.pop(0)
    env.synchronize()
    _check(env, *want, what="1030 envs")
    env.close()


# --------------------------------------------------------------------- 9 --
@pytest.mark.parametrize("shape", FEW, ids=FEW_IDS)
def test_resume(ctx, shape):
    """Run A takes s1 + s2 calls with a row at s1 and one at the end.  Run B
    takes s1 calls and a row; its BINS / ITEMS / RNG and episode_state() go
    into a fresh venv with statistics on, which takes the other s2 calls and
    a row.  The final rows agree in every entry but ROW, and so do the
    per-env arrays."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    s1, s2 = 9, 15
    rows = _ref_act(B, D)[0]
    assert len(rows) == s1 + s2
    a = _venv(ctx, B, D)
    a.set_episode_stats(4)
    _run_act(a, rows, [s1, s1 + s2])
    b = _venv(ctx, B, D)
    b.set_episode_stats(4)
    _run_act(b, rows[:s1], [s1])
    _same_rows(b.episode_stats(), a.episode_stats(0, 1), "the row at s1")
    running, first = b.episode_state()
    assert running.any() and (first >= 0).any()
    c = _venv(ctx, B, D, x0=X0 + 1)            # a fresh venv, another seed
    c.set_episode_stats(4)
    for which in (_lib.VENV_BINS, _lib.VENV_ITEMS, _lib.VENV_RNG):
        c.set(which, b.get(which))
    c.set_episode_state(running, first)
    _run_act(c, rows[s1:], [s2])
    ra, rc = a.episode_stats(1, 1)[0], c.episode_stats(0, 1)[0]
    assert ra[er.ROW] == 1 and rc[er.ROW] == 0
    keep = np.arange(er.COUNT) != er.ROW
    _same_rows(rc[keep], ra[keep], "the final row")
    assert ra[er.EPISODES] > 0 and ra[er.CALLS] == s2
    for x, y, what in zip(c.episode_state(), a.episode_state(),
                          ("running", "first")):
        _same(x, y, what)
    for env in (a, b, c):
        env.close()
