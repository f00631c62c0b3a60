"""GPU tests of the VecEnv on general item sets (xh_item_set: K shapes drawn by
the K-way threshold rule, a capacity per dim; xh_venv_create_ex /
xh_venv_set_item_set), against the host restatement tests/venv_items_ref.py
(pinned to the oracle by tests/test_venv_items_ref.py) and, for the default
set, against the builtin kernels of the same library.

Shapes: test_gpu_venv_act's -- 8 bins 2-D N = 19 (a partial wave), 32 bins 1-D
N = 70, 64 bins 2-D N = 40 (a partial last wave), 128 bins 3-D N = 5 (eight
lanes per env) and a sharded case at an offset inside a larger job."""
import functools

import numpy as np
import pytest

import venv_episode_ref as er
import venv_learn_ref as vl
from venv_act_ref import BOUNDARY_N, BOUNDARY_X0, ActRef, mixed_rows
from venv_act_ref import run as act_run
from venv_items_ref import DEFAULT_ITEMS, DEFAULT_WEIGHTS, ItemsRef, run

pytestmark = pytest.mark.gpu

# (B, D, N, offset, Ng)
CASES = [(8, 2, 19, 0, 19), (32, 1, 70, 0, 70), (64, 2, 40, 0, 40),
         (128, 3, 5, 0, 5), (16, 3, 9, 6, 21)]
SHARDED_2D = (16, 2, 9, 6, 21)
CASE_ID = lambda c: "B%d-D%d-N%d-o%d-Ng%d" % c  # noqa: E731
X0 = 4242

ITEMS5 = [(3, 1), (2, 2), (1, 4), (5, 7), (1, 1)]
WEIGHTS5 = [2.0, 0.0, 1.0, 0.5, 3.25]  # item 1 is never drawn
CAP57 = (5, 7)
ITEMS16 = [(1 + k % 7, 1 + (3 * k) % 5) for k in range(16)]
WEIGHTS16 = [1.0 + (5 * k) % 7 for k in range(16)]
CAP75 = (7, 5)

# (case, items, weights, capacity)
CUSTOM = [
    (CASES[0], ITEMS5, WEIGHTS5, CAP57),
    (SHARDED_2D, ITEMS5, WEIGHTS5, CAP57),
    (CASES[2], ITEMS16, WEIGHTS16, CAP75),
    (CASES[1], [(64,)], [1.0], (64,)),
    (CASES[3], [(6, 1, 3), (2, 8, 1), (1, 1, 1)], [1.0, 2.0, 3.0], (6, 8, 3)),
]
CUSTOM_IDS = ["K5-cap57-B8", "K5-cap57-sharded", "K16-B64", "K1-cap64-B32",
              "K3-cap683-B128"]


def _venv(ctx, case, x0=X0, **kw):
    from dependence_free_rl_amd import VecEnv
    B, D, N, offset, Ng = case
    return VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=x0,
                  env_offset=offset, num_envs_global=Ng, **kw)


def _ref(case, items, weights, capacity, x0=X0):
    B, D, N, offset, Ng = case
    return ItemsRef(B, D, N, x0, items, weights, capacity, n_global=Ng,
                    offset=offset)


def _raw_set(env, items, weights, capacity):
    """xh_venv_set_item_set with a capacity of the caller's choice (the Python
    method always passes the venv's own); returns the status."""
    import ctypes as C
    from dependence_free_rl_amd import _lib
    from dependence_free_rl_amd.venv import _item_set
    s = _item_set(items, weights, capacity, env.D)
    return _lib.lib.xh_venv_set_item_set(env.h, C.byref(s))


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _buffers(env, acted):
    from dependence_free_rl_amd import _lib
    which = [_lib.VENV_ACTIONS, _lib.VENV_REWARD, _lib.VENV_DONE,
             _lib.VENV_BINS, _lib.VENV_ITEMS, _lib.VENV_RNG, _lib.VENV_OBS,
             _lib.VENV_MASK]
    if acted:
        which += [_lib.VENV_POLICY, _lib.VENV_PCHOICE]
    return {w: env.get(w) for w in which}


# ------------------------------------------- 1. default set == builtin ----
@pytest.mark.parametrize("case", CASES, ids=CASE_ID)
def test_general_kernels_on_the_default_set_are_the_builtin_ones(ctx, case):
    """A venv created with xh_item_set_default's set (the general kernels) and
    one created without a set (the builtin ones), same seed, same calls: 12
    steps of act (sample, obs, the record with distributions), step, and
    masked apply / reset -- every buffer and every record array identical."""
    B, D, N, offset, Ng = case
    S = 12
    rows = mixed_rows(B * 10 + D, S, N, B)
    g = np.random.default_rng(B + D)
    actions = g.integers(0, 2, (S, N)).astype(np.int32)
    masks = (g.random((S, N)) < 0.6).astype(np.uint8)
    envs = [_venv(ctx, case),
            _venv(ctx, case, items=DEFAULT_ITEMS[D], weights=DEFAULT_WEIGHTS,
                  capacity=8)]
    assert envs[1].item_set()["thresholds"].tolist() == [0.4, 1.0]
    for env in envs:
        env.set_record(S, distrib=True)
    acted = False
    for s in range(S):
        for env in envs:
            if s % 3 == 0:
                env.act(rows[s], write_obs=True, fetch=False)
            elif s % 3 == 1:
                env.set_actions(actions[s])
                env.step(write_obs=True, fetch=False)
            else:
                env.set_actions(actions[s])
                over = env.apply(masks[s])
                env.reset(over)
                env.observe()
        acted = True
        a, b = (_buffers(env, acted) for env in envs)
        for w in a:
            _same(b[w], a[w], "buffer %d, step %d" % (w, s))
    ra, rb = (env.record() for env in envs)
    assert sorted(ra) == sorted(rb) and "distrib" in ra and "bins" in ra
    for name in ra:
        _same(rb[name], ra[name], "record " + name)
    assert ra["done"].any()
    for env in envs:
        env.close()


# ------------------------------------------ 2. custom sets == restatement --
@functools.lru_cache(maxsize=None)
def _custom_reference(i):
    """(rows, actions, per-step reference) of CUSTOM[i], computed once: act
    (sample) except every third step, which is xh_venv_step's visit."""
    case, items, weights, capacity = CUSTOM[i]
    B, D, N, offset, Ng = case
    S = 12
    rows = mixed_rows(B * 10 + D + 1, S, N, B)
    actions = np.random.default_rng(i).integers(0, 2, (S, N)).astype(np.int32)
    ref = _ref(case, items, weights, capacity)
    steps = []
    state = lambda: {"bins": ref.bins(), "item": ref.items(),  # noqa: E731
                     "rng": ref.streams(), "obs": ref.obs()}
    first = state()
    for s in range(S):
        r = ref.step(actions[s]) if s % 3 == 2 else ref.act(rows[s])
        r.update(state())
        steps.append(r)
    return rows, actions, first, steps


@pytest.mark.parametrize("i", range(len(CUSTOM)), ids=CUSTOM_IDS)
def test_custom_sets_are_the_restatement_bit_for_bit(ctx, i):
    """bins, items, the stream states, OBS, actions, PCHOICE, reward and done
    after every call, and the record at the end."""
    from dependence_free_rl_amd import _lib
    case, items, weights, capacity = CUSTOM[i]
    B, D, N, offset, Ng = case
    rows, actions, first, steps = _custom_reference(i)
    done = np.stack([r["done"] for r in steps])
    assert done.any() and not done.all(axis=0).all()
    drawn = {tuple(r["item"][e]) for r in steps for e in range(N)}
    zero = [tuple(it) for it, w in zip(items, weights) if w == 0.0]
    assert len(drawn) >= min(len(items) - len(zero), 3)
    assert not drawn & set(zero), "a zero-weight item was drawn"
    env = _venv(ctx, case, items=items, weights=weights, capacity=capacity)
    got = env.item_set()
    np.testing.assert_array_equal(got["items"], np.asarray(items))
    np.testing.assert_array_equal(got["capacity"], np.asarray(capacity))
    env.set_record(len(steps))
    b, it = env.view()
    _same(b, first["bins"], "bins at construction")
    _same(it, first["item"], "items at construction")
    _same(env.get(_lib.VENV_RNG), first["rng"], "streams at construction")
    _same(env.observe(), first["obs"], "obs at construction")
    recorded = []
    for s, want in enumerate(steps):
        if s % 3 == 2:
            env.set_actions(actions[s])
            env.step(write_obs=True, fetch=False)
        else:
            recorded.append(s)
            a, p, _, _ = env.act(rows[s], write_obs=True)
            _same(a, want["action"], "action, step %d" % s)
            _same(p, want["pchoice"], "pchoice, step %d" % s)
        _same(env.get(_lib.VENV_REWARD), want["reward"], "reward, step %d" % s)
        _same(env.get(_lib.VENV_DONE), want["done"], "done, step %d" % s)
        b, it = env.view()
        _same(b, want["bins"], "bins, step %d" % s)
        _same(it, want["item"], "items, step %d" % s)
        _same(env.get(_lib.VENV_RNG), want["rng"], "streams, step %d" % s)
        _same(env.get(_lib.VENV_OBS), want["obs"], "obs, step %d" % s)
    rec = env.record()
    before = [first] + steps
    for name in ("action", "pchoice", "reward", "done"):
        _same(rec[name], np.stack([steps[s][name] for s in recorded]),
              "record " + name)
    _same(rec["bins"], np.stack([before[s]["bins"] for s in recorded]),
          "record bins")
    _same(rec["items"][:, :, :D],
          np.stack([before[s]["item"] for s in recorded]), "record items")
    env.close()


def test_apply_and_reset_on_the_envs_own_stream(ctx):
    """One env (Ng = 1: its stream is the engine): xh_venv_apply / reset on a
    custom set against the restatement."""
    from dependence_free_rl_amd import _lib
    case = (8, 2, 1, 0, 1)
    ref = _ref(case, ITEMS5, WEIGHTS5, CAP57)
    env = _venv(ctx, case, items=ITEMS5, weights=WEIGHTS5, capacity=CAP57)
    overs = 0
    for s in range(16):
        a = s % 2
        env.set_actions([a])
        over = env.apply()
        assert bool(over[0]) == ref.apply(a)
        if over[0]:
            overs += 1
            env.reset()
            ref.reset()
        b, it = env.view()
        _same(b, ref.bins(), "bins, call %d" % s)
        _same(it, ref.items(), "items, call %d" % s)
        assert env.get(_lib.VENV_RNG)[0] == ref.rng.state
    assert overs > 0
    env.close()


# ------------------------------------------------ 3. threshold boundary ----
@pytest.mark.parametrize("B", [8, 128])
def test_a_draw_on_the_threshold_takes_the_next_item(ctx, B):
    """u the canonical draw of an env's item: the set with weights (u, 1 - u)
    has c_0 <= u, so the env gets item 1; with (nextafter(u, 1), 1 - u) it has
    u < c_0 and gets item 0.  For the construction draw and for the draw
    inside the first act (after set_item_set), 8 envs each."""
    from oracle import pyoracle as po
    from dependence_free_rl_amd import item_set_thresholds
    D, N = 2, BOUNDARY_N
    case = (B, D, N, 0, N)
    two = [(1, 1), (2, 2)]
    rows = np.zeros((N, B), np.float32)
    rows[:, 3] = 1.0

    def sides(u):
        ws = [(u, 1.0 - u), (np.nextafter(u, 1.0), 1.0 - u)]
        c = [item_set_thresholds(two, w)[0] for w in ws]
        assert c[0] <= u < c[1], (u, c)  # on the host, before any launch
        return ws

    checked = 0
    for e in range(8):
        # the construction draw: engine position 2 e
        u = po.Rng(po.minstd_jump(BOUNDARY_X0, 2 * e)).canonical()
        for w, want in zip(sides(u), (1, 0)):
            env = _venv(ctx, case, x0=BOUNDARY_X0, items=two, weights=w)
            got = env.view()[1]
            env.close()
            ref = _ref(case, two, w, None, x0=BOUNDARY_X0)
            _same(got, ref.items(), "construction, env %d" % e)
            assert tuple(got[e]) == two[want], (e, want)
            checked += 1
        # the draw inside the first act: two draws after the env's turn starts
        start = _ref(case, two, None, None, x0=BOUNDARY_X0)
        u = po.Rng(po.minstd_jump(int(start.streams()[e]), 2)).canonical()
        for w, want in zip(sides(u), (1, 0)):
            ref = _ref(case, two, None, None, x0=BOUNDARY_X0)
            env = _venv(ctx, case, x0=BOUNDARY_X0, items=two)
            ref.set_item_set(two, w)
            env.set_item_set(two, w)
            r = ref.act(rows)
            a, _, _, done = env.act(rows)
            got = env.view()[1]
            env.close()
            assert not r["done"].any() and not done.any()
            _same(a, r["action"], "action, env %d" % e)
            _same(got, ref.items(), "first act, env %d" % e)
            assert tuple(got[e]) == two[want], (e, want)
            checked += 1
    assert checked == 32  # no case skipped


# ------------------------------------- 4. downstream at capacity (5, 7) ----
def _obs32(bins, items, cap):
    """observation::to_vector by numpy float32 division, [rows][B][2D]."""
    capf = np.asarray(cap, np.float32)
    b = bins.astype(np.float32) / capf
    it = np.broadcast_to((items.astype(np.float32) / capf)[:, None, :], b.shape)
    out = np.concatenate([b, it], axis=2)
    assert out.dtype == np.float32
    return out


def _next_state(rec, present, D):
    """venv_learn_ref.next_rows' states as integers: (bins [P N][B][D], items
    [P N][D])."""
    pb, pi = present
    bins = rec["bins"].astype(np.int64)
    P, N, B, _ = bins.shape
    items = rec["items"].astype(np.int64)[:, :, :D]
    nb = np.concatenate([bins[1:], pb.astype(np.int64)[None]])
    ni = np.concatenate([items[1:], pi.astype(np.int64)[None][:, :, :D]])
    for t in range(P):
        for e in range(N):
            if rec["done"][t, e]:
                eb = bins[t, e].copy()
                eb[rec["action"][t, e]] -= items[t, e]
                nb[t, e], ni[t, e] = eb, items[t, e]
    return nb.reshape(P * N, B, D), ni.reshape(P * N, D)


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=CASE_ID)
def test_mask_record_obs_and_advantages_at_capacity_5_7(ctx, case):
    """With the action mask on, legal() and the recorded legal words are the
    restatement's; record_obs of both views (the terminal view of an ended
    transition included), through a run of rows and through a shuffled index
    list, is numpy's float32 division by (5, 7); advantages on that record
    equal venv_learn_ref's (an unchanged path)."""
    B, D, N, offset, Ng = case
    T = 8
    g = np.random.default_rng(B)
    rows = (g.random((T, N, B)) + 0.05).astype(np.float32)
    rows[:, ::4, :] = 1e-6
    rows[:, ::4, 0] = 1.0  # these envs overflow bin 0 when nothing else fits
    # nearly full bins, so that legal sets differ and episodes end in T steps
    # (about 8 bins per env with room for a small item, one bin empty)
    bins0 = (g.integers(0, 3, (N, B, D)) *
             (g.random((N, B, 1)) < 8.0 / B)).astype(np.int8)
    bins0[:, 1] = CAP57
    ref = _ref(case, ITEMS5, WEIGHTS5, CAP57)
    for e, env_ref in enumerate(ref.envs):
        env_ref.bins[:] = bins0[e]
    want = run(ref, rows, masked=True)
    assert want["done"].any(), "an ended transition"
    assert not want["legal"].all() and want["legal"].any(axis=2).all()
    env = _venv(ctx, case, items=ITEMS5, weights=WEIGHTS5, capacity=CAP57)
    from dependence_free_rl_amd import XhError, _lib
    with pytest.raises(XhError, match="capacity 5"):
        env.set(_lib.VENV_BINS, np.full((N, B, D), 6, np.int8))
    env.set(_lib.VENV_BINS, bins0)  # (5, 7) passes: the check is per dim
    env.set_action_mask(True)
    env.set_record(T)
    for s in range(T):
        _same(env.legal(), want["legal"][s], "legal, step %d" % s)
        a, p, r, d = env.act(rows[s])
        _same(a, want["action"][s], "action, step %d" % s)
        _same(d, want["done"][s], "done, step %d" % s)
    rec = env.record()
    _same(rec["legal"], want["legal"][:T], "record legal")
    _same(rec["bins"], want["bins"][:T], "record bins")
    present = env.view()
    _same(present[0], want["bins"][T], "bins")
    # STATE: slots 0 .. T
    sb = np.concatenate([rec["bins"], present[0][None]]).reshape(-1, B, D)
    si = np.concatenate([rec["items"][:, :, :D],
                         present[1][None]]).reshape(-1, D)
    state = _obs32(sb, si, CAP57)
    _same(state, want["obs"].reshape(-1, B, 2 * D), "the restatement's obs")
    nb, ni = _next_state(rec, present, D)
    assert (nb < 0).any(), "a terminal view with a negative bin"
    nxt = _obs32(nb, ni, CAP57)
    for view, full in (("state", state), ("next", nxt)):
        _same(env.record_obs(view), full, view + ": every row")
        _same(env.record_obs(view, first=N + 3, count=2 * N + 1),
              full[N + 3:3 * N + 4], view + ": a run of rows")
        idx = g.permutation(len(full))[:len(full) // 2].astype(np.int32)
        _same(env.record_obs(view, rows=idx), full[idx], view + ": index list")
    values = g.uniform(-1, 1, (T + 1, N)).astype(np.float32)
    got = env.advantages(values, gamma=0.99, lam=0.95)
    _same(got["adv"], vl.gae_reward_f32(rec["done"], rec["reward"], values,
                                        0.99, 0.95), "adv")
    _same(got["td_target"], vl.td_targets_reward_f32(
        rec["done"], rec["reward"], values, None, 0.99), "td_target")
    env.close()


# --------------------------------------------------------- 5. curriculum --
def test_set_item_set_switches_the_mix_from_the_next_draw(ctx):
    """6 steps on set A, set_item_set(B) at the same capacity, 6 more: held
    items stay, every later draw is from B, the streams are the restatement's.
    A set with another capacity is refused and changes nothing.  And a venv
    created without a set switches to the general kernels on its first set."""
    from dependence_free_rl_amd import XhError, _lib
    case = CASES[0]
    B, D, N, offset, Ng = case
    set_a = ([(3, 1), (1, 4)], [1.0, 1.0])
    set_b = ([(2, 2), (5, 7), (1, 1)], [1.0, 0.5, 2.0])
    assert not {tuple(x) for x in set_a[0]} & {tuple(x) for x in set_b[0]}
    rows = mixed_rows(77, 12, N, B)
    ref = _ref(case, *set_a, CAP57)
    env = _venv(ctx, case, items=set_a[0], weights=set_a[1], capacity=CAP57)
    for s in range(12):
        if s == 6:
            held = ref.items().copy()
            assert _raw_set(env, *set_b, (5, 8)) == _lib.XH_ERR_INVALID
            assert b"capacity" in _lib.lib.xh_last_error()
            with pytest.raises(XhError, match="item set"):
                env.set_item_set([(6, 1)])  # above the venv's capacity 5
            np.testing.assert_array_equal(env.item_set()["items"],
                                          np.asarray(set_a[0]))
            ref.set_item_set(*set_b)
            env.set_item_set(*set_b)
            _same(env.view()[1], held, "held items stay")
            _same(env.get(_lib.VENV_RNG), ref.streams(), "no stream moved")
            got = env.item_set()
            np.testing.assert_array_equal(got["items"], np.asarray(set_b[0]))
            np.testing.assert_array_equal(got["capacity"], np.asarray(CAP57))
        items_before = ref.items().copy()
        want = ref.act(rows[s])
        a, p, r, d = env.act(rows[s])
        _same(a, want["action"], "action, step %d" % s)
        _same(d, want["done"], "done, step %d" % s)
        b, it = env.view()
        _same(b, ref.bins(), "bins, step %d" % s)
        _same(it, ref.items(), "items, step %d" % s)
        _same(env.get(_lib.VENV_RNG), ref.streams(), "streams, step %d" % s)
        if s >= 6:  # an item that changed in this step was drawn from B
            new = {tuple(x) for x, y in zip(it, items_before)
                   if tuple(x) != tuple(y)}
            assert new and new <= {tuple(x) for x in set_b[0]}, s
    env.close()
    # a venv created without a set: its first set switches it
    ref = _ref(case, DEFAULT_ITEMS[D], DEFAULT_WEIGHTS, 8)
    env = _venv(ctx, case)
    assert env.item_set()["thresholds"].tolist() == [0.4, 1.0]
    assert _raw_set(env, ITEMS5, WEIGHTS5, CAP57) == _lib.XH_ERR_INVALID
    assert b"capacity" in _lib.lib.xh_last_error()
    small = ([(3, 1), (2, 2), (1, 4), (8, 8), (1, 1)], WEIGHTS5)
    for s in range(6):
        if s == 3:
            ref.set_item_set(*small)
            env.set_item_set(*small)
        want = ref.act(rows[s])
        a, _, _, _ = env.act(rows[s], write_obs=True)
        _same(a, want["action"], "builtin venv: action, step %d" % s)
        _same(env.view()[1], ref.items(), "builtin venv: items, step %d" % s)
        _same(env.get(_lib.VENV_OBS), ref.obs(), "builtin venv: obs, step %d" % s)
    env.close()


# ------------------------------------------------- 6. episode statistics --
def test_episode_statistics_on_a_five_item_set(ctx):
    """episode_stats() after 40 act steps equals the lengths the restatement
    counts."""
    case = CASES[0]
    B, D, N, offset, Ng = case
    S = 40
    rows = mixed_rows(5, S, N, B)
    ref = _ref(case, ITEMS5, WEIGHTS5, CAP57)
    done = np.stack([ref.act(rows[s])["done"] for s in range(S)]) != 0
    live = np.ones((S, N), bool)
    want, running, first, hist = er.rows_of_history(done, live, [S])
    assert want[0, er.EPISODES] == done.sum() > N
    env = _venv(ctx, case, items=ITEMS5, weights=WEIGHTS5, capacity=CAP57)
    env.set_episode_stats(4)
    for s in range(S):
        env.act(rows[s], fetch=False)
    env.episode_row()
    got = env.episode_stats()
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    r, f = env.episode_state()
    _same(r, running, "running")
    _same(f, first, "first")
    lengths = sorted(x for per_env in hist.lengths for x in per_env)
    assert got[0, er.LEN_SUM] == sum(lengths)
    assert got[0, er.LEN_MIN] == lengths[0] and got[0, er.LEN_MAX] == lengths[-1]
    env.close()


# ----------------------------------- 7. the builtin venv is what it was ----
def test_a_plain_venv_still_matches_the_act_reference(ctx):
    """After everything above: xh_venv_create's venv against venv_act_ref, the
    comparison of test_gpu_venv_act on its first case."""
    from dependence_free_rl_amd import _lib
    case = CASES[0]
    B, D, N, offset, Ng = case
    S = 16
    rows = mixed_rows(B * 10 + D, S, N, B)
    ref = act_run(B, D, N, X0, rows, n_global=Ng, offset=offset)
    env = _venv(ctx, case)
    _same(env.get(_lib.VENV_RNG), ref["rng"][0], "streams at construction")
    for s in range(S):
        got = env.act(rows[s], write_obs=True)
        for name, g in zip(("action", "pchoice", "reward", "done"), got):
            _same(g, ref[name][s], "%s, step %d" % (name, s))
        b, it = env.view()
        _same(b, ref["bins"][s + 1], "bins, step %d" % s)
        _same(it, ref["item"][s + 1], "items, step %d" % s)
        _same(env.get(_lib.VENV_RNG), ref["rng"][s + 1], "streams, step %d" % s)
        _same(env.get(_lib.VENV_OBS), ref["obs"][s + 1], "obs, step %d" % s)
    env.close()
    assert ActRef(B, D, N, X0, n_global=Ng, offset=offset).rng.state == \
        _ref(case, DEFAULT_ITEMS[D], DEFAULT_WEIGHTS, 8).rng.state
