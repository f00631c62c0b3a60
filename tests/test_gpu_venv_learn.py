"""GPU tests of the learner's side of a recorded window: xh_venv_record_obs
(STATE / NEXT observations of recorded rows, runs and shuffled minibatches),
xh_venv_record_ends and xh_venv_advantages, against tests/venv_learn_ref.py
(pinned on the CPU by tests/test_venv_learn_ref.py) and the reference
trajectories of tests/venv_act_ref.py.

Shapes: test_gpu_venv_act.py's -- 8 bins (one lane per row, a partial wave),
32 bins 1-D with N = 70, 64 bins 2-D with N = 40 (a partial last wave), 128
bins 3-D with N = 5 (eight lanes per row), 16 bins 3-D -- with T = 16 recorded
steps in a record of 17 slots (the cursor inside the record), so that step 17
can continue the trajectory."""
import ctypes as C
import functools

import numpy as np
import pytest

import long_window_ref as lw
import venv_learn_ref as vl
from venv_act_ref import mixed_rows, run

pytestmark = pytest.mark.gpu

CASES = [(8, 2, 19), (32, 1, 70), (64, 2, 40), (128, 3, 5), (16, 3, 9)]
IDS = ["B%d-D%d-N%d" % c for c in CASES]
STEPS, X0 = 16, 4242
GAMMA, LAM = 0.99, 0.95


@functools.lru_cache(maxsize=None)
def _trajectory(case):
    """(rows [STEPS+1][N][B], reference run of STEPS + 1 steps) of a case,
    computed once and left unchanged; slots 0 .. STEPS - 1 are recorded."""
    B, D, N = case
    rows = mixed_rows(B * 10 + D, STEPS + 1, N, B)
    ref = run(B, D, N, X0, rows)
    ended = ref["done"][:STEPS].any(axis=0)
    assert ended.any() and not ended.all(), "some envs end, not all"
    return rows, ref


def _ref_record(case):
    _, ref = _trajectory(case)
    T = STEPS
    record = {"bins": ref["bins"][:T], "items": ref["item"][:T],
              "action": ref["action"][:T], "done": ref["done"][:T]}
    return record, (ref["bins"][T], ref["item"][T])


def _recorded(ctx, case, slots=STEPS + 1):
    """A venv after STEPS recorded act() calls on the case's rows."""
    from dependence_free_rl_amd import VecEnv
    B, D, N = case
    rows, _ = _trajectory(case)
    env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=X0)
    env.set_record(slots)
    for s in range(STEPS):
        env.act(rows[s], fetch=False)
    assert env.record_pos() == STEPS
    return env


# device memory of the test's own (the caller's side of the pointer forms)
def _dev_alloc(ctx, nbytes):
    from dependence_free_rl_amd import _lib
    p = C.c_void_p()
    _lib.check(_lib.tensor_alloc(ctx.h, (nbytes + 3) // 4, C.byref(p)))
    return p.value


def _dev_free(ctx, ptr):
    from dependence_free_rl_amd import _lib
    _lib.check(_lib.tensor_free(ctx.h, ptr))


def _dev_put(ctx, ptr, a):
    from dependence_free_rl_amd import _lib
    a = np.ascontiguousarray(a)
    assert a.nbytes % 4 == 0
    _lib.check(_lib.tensor_copy(ctx.h, ptr, a.ctypes.data, a.nbytes // 4,
                                _lib.COPY_H2D))


def _dev_get(ctx, ptr, dtype, shape):
    from dependence_free_rl_amd import _lib
    out = np.zeros(shape, dtype)
    assert out.nbytes % 4 == 0
    _lib.check(_lib.tensor_copy(ctx.h, out.ctypes.data, ptr, out.nbytes // 4,
                                _lib.COPY_D2H))
    return out


def _flat(obs):
    return obs.reshape(obs.shape[0], -1).astype(np.float64)


def _assert_bits(got, want, what=""):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32),
                                  err_msg=what)


# ------------------------------------------------------------------ 1, 2 --
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_record_obs_state(ctx, case):
    """STATE: all (P + 1) N rows are the reference trajectory's observations
    exactly; slot P is what xh_venv_observe gives; the run of rows and the
    identity index list agree."""
    B, D, N = case
    record, present = _ref_record(case)
    want = vl.state_rows(record, *present)
    env = _recorded(ctx, case)
    got = env.record_obs("state")
    assert got.dtype == np.float32 and got.shape == ((STEPS + 1) * N, B, 2 * D)
    np.testing.assert_array_equal(_flat(got), want)
    np.testing.assert_array_equal(got[STEPS * N:], env.observe())
    listed = env.record_obs("state", rows=np.arange((STEPS + 1) * N))
    _assert_bits(listed, got)
    # a run inside the record: first / count without a list
    part = env.record_obs("state", first=3 * N + 2, count=2 * N + 1)
    _assert_bits(part, got[3 * N + 2:5 * N + 3])
    env.close()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_record_obs_next(ctx, case):
    """NEXT: every row equals next_rows -- S_t+1, and the terminal view E_t on
    the ended rows, of which the reference has some in every shape."""
    B, D, N = case
    record, present = _ref_record(case)
    ended = np.nonzero(record["done"].reshape(-1))[0]
    assert 0 < len(ended) < STEPS * N
    want = vl.next_rows(record, present)
    env = _recorded(ctx, case)
    got = env.record_obs("next")
    assert got.shape == (STEPS * N, B, 2 * D)
    np.testing.assert_array_equal(_flat(got)[ended], want[ended])
    np.testing.assert_array_equal(_flat(got), want)
    _assert_bits(env.record_obs("next", rows=ended), got[ended])
    env.close()


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("case", [CASES[0], CASES[2], CASES[3]],
                         ids=[IDS[0], IDS[2], IDS[3]])
def test_minibatch_gather(ctx, case):
    """A seeded permutation of all rows in three uneven chunks through first
    / count equals the permuted rows of the linear result: STATE through a
    host list and host results, NEXT through device pointers for the list and
    the output."""
    B, D, N = case
    env = _recorded(ctx, case)
    g = np.random.default_rng(B + N)
    row = B * 2 * D
    for view, total in (("state", (STEPS + 1) * N), ("next", STEPS * N)):
        linear = env.record_obs(view)
        perm = g.permutation(total).astype(np.int32)
        cuts = [0, total // 7, total // 7 + total // 2 + 1, total]
        if view == "state":
            for a, b in zip(cuts[:-1], cuts[1:]):
                got = env.record_obs(view, rows=perm, first=a, count=b - a)
                _assert_bits(got, linear[perm[a:b]], "%s %d:%d" % (view, a, b))
            continue
        rows_dev = _dev_alloc(ctx, total * 4)
        out_dev = _dev_alloc(ctx, total * row * 4)
        _dev_put(ctx, rows_dev, perm)
        for a, b in zip(cuts[:-1], cuts[1:]):
            # chunk [a, b) of the list into rows a .. b - 1 of the output
            assert env.record_obs(view, rows=rows_dev, first=a, count=b - a,
                                  out=out_dev + a * row * 4) is None
        env.synchronize()
        _assert_bits(_dev_get(ctx, out_dev, np.float32, (total, B, 2 * D)),
                     linear[perm])
        _dev_free(ctx, rows_dev)
        _dev_free(ctx, out_dev)
    env.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_bad_indices_and_bad_pointers(ctx, case):
    """An index >= (P + 1) N (or negative) leaves its output row as prefilled
    and synchronize reports XH_ERR_INVALID once, the other rows correct; a
    misaligned obs_dev is XH_ERR_INVALID at the call; a run past the view's
    rows too; a record without states is XH_ERR_STATE."""
    from dependence_free_rl_amd import VecEnv, XhError, _lib
    B, D, N = case
    env = _recorded(ctx, case)
    total = (STEPS + 1) * N
    linear = env.record_obs("state")
    rows = np.array([5, total, 0, 2 ** 31 - 1, total - 1, -1, N + 1], np.int32)
    bad = (rows < 0) | (rows >= total)
    out_dev = _dev_alloc(ctx, len(rows) * B * 2 * D * 4 + 16)
    fill = np.full((len(rows), B, 2 * D), -77.5, np.float32)
    _dev_put(ctx, out_dev, fill)
    env.record_obs("state", rows=rows, out=out_dev)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()
    env.synchronize()  # reported once
    got = _dev_get(ctx, out_dev, np.float32, fill.shape)
    _assert_bits(got[bad], fill[bad])
    _assert_bits(got[~bad], linear[rows[~bad]])
    # NEXT has P N rows: row P N is outside it
    _dev_put(ctx, out_dev, fill)
    env.record_obs("next", rows=np.array([STEPS * N, 1], np.int32), out=out_dev)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()
    got = _dev_get(ctx, out_dev, np.float32, fill.shape)
    _assert_bits(got[0], fill[0])
    _assert_bits(got[1], env.record_obs("next")[1])
    for off in (4, 8):
        with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
            env.record_obs("state", first=0, count=2, out=out_dev + off)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.record_obs("state", first=total - 1, count=2, out=out_dev)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.record_obs("next", first=STEPS * N, count=1, out=out_dev)
    env.synchronize()  # nothing was launched by the refused calls
    _dev_free(ctx, out_dev)
    env.close()
    bare = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=X0)
    rows_in, _ = _trajectory(case)
    for states in (None, False):
        if states is not None:
            bare.set_record(3, states=states)
            bare.act(rows_in[0], fetch=False)
        with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_STATE):
            bare.record_obs("state")
    bare.close()


# --------------------------------------------------------------------- 4 --
def _ends_of(done):
    e, t = np.nonzero(np.asarray(done).T != 0)
    return (t * done.shape[1] + e).astype(np.int32)


@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_record_ends(ctx, case):
    """The ended transitions t N + e, env-major with t ascending, and their
    count, from the record alone (N = 70: the three-pass list, N = 40: one
    workgroup); an empty record gives an empty list."""
    env = _recorded(ctx, case)
    done = env.record()["done"]
    np.testing.assert_array_equal(done, _ref_record(case)[0]["done"])
    want = _ends_of(done)
    assert 0 < len(want) < done.size
    got = env.record_ends()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    env.rewind()
    assert env.record_ends().size == 0
    env.close()


def test_record_ends_past_one_workgroup(ctx):
    """N = 8200 (a multiple of 4 above 8192): the parallel passes."""
    from dependence_free_rl_amd import VecEnv
    B, D, N, T = 8, 1, 8200, 6
    rows = np.full((N, B), 0.03 / (B - 1), np.float32)
    rows[:, 0] = 0.97  # peaked at bin 0: the envs overflow and reset
    rows[1::3] = 1.0   # uniform rows: those envs rarely end in T steps
    env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=X0)
    env.set_record(T, states=False)
    for _ in range(T):
        env.act(rows, fetch=False)
    done = env.record()["done"]
    per_env = (done != 0).sum(axis=0)
    assert (per_env > 0).any() and (per_env == 0).any() and per_env.max() > 1
    np.testing.assert_array_equal(env.record_ends(), _ends_of(done))
    env.close()


# --------------------------------------------------------------------- 5 --
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_advantages_from_the_record(ctx, case):
    """The record's window with seeded values and v_term: adv and td_target
    are gae_f32 / td_targets_f32 bit for bit (the venv's rewards are the
    implied ones), lambda_return is the restatement; v_term = NULL is a zero
    array; the record's own reward with the caller's done is the same."""
    B, D, N = case
    record, _ = _ref_record(case)
    done = record["done"]
    g = np.random.default_rng(B + D + N)
    values = g.normal(0.5, 1.5, (STEPS + 1, N)).astype(np.float32)
    v_term = g.normal(0.5, 1.5, (STEPS, N)).astype(np.float32)
    adv = lw.gae_f32(done, values, GAMMA, LAM)
    env = _recorded(ctx, case)
    names = ("adv", "td_target", "lambda_return")
    got = env.advantages(values, v_term=v_term, gamma=GAMMA, lam=LAM,
                         returns=names)
    _assert_bits(got["adv"], adv, "adv")
    _assert_bits(got["td_target"],
                 lw.td_targets_f32(done, values, v_term, GAMMA), "td_target")
    _assert_bits(got["lambda_return"], vl.lambda_return_f32(adv, values),
                 "lambda_return")
    np.testing.assert_array_equal(got["stats"][2:], [STEPS * N, (done != 0).sum()])
    none = env.advantages(values, gamma=GAMMA, lam=LAM)
    assert sorted(none) == ["adv", "stats", "td_target"]
    _assert_bits(none["adv"], adv)
    _assert_bits(none["td_target"], lw.td_targets_f32(
        done, values, np.zeros((STEPS, N), np.float32), GAMMA))
    # pointers: the values on the device, results on the host
    vdev = _dev_alloc(ctx, values.nbytes)
    _dev_put(ctx, vdev, values)
    _assert_bits(env.advantages(vdev, gamma=GAMMA, lam=LAM,
                                returns=("adv",))["adv"], adv)
    _dev_free(ctx, vdev)
    env.close()


# --------------------------------------------------------------------- 6 --
@functools.lru_cache(maxsize=None)
def _window(T, N):
    """A caller's window and its references, computed once: rewards in [-2,
    2], values and v_term in [-50, 50], done with terminals on the chunk
    edges, env 1 all-terminal, env 0 never ending."""
    g = np.random.default_rng(1000 * T + N)
    done = vl.edge_done(T, N, T + N)
    assert done[:, 1].all() and not done[:, 0].any()
    reward = g.uniform(-2.0, 2.0, (T, N)).astype(np.float32)
    values = g.uniform(-50.0, 50.0, (T + 1, N)).astype(np.float32)
    v_term = g.uniform(-50.0, 50.0, (T, N)).astype(np.float32)
    adv = vl.gae_reward_f32(done, reward, values, GAMMA, LAM)
    a64, S = vl.gae_reward_f64_forward(done, reward, values, GAMMA, LAM)
    # the bound holds for the restatement (a condition on the reference)
    assert np.all(np.abs(adv.astype(np.float64) - a64) <= 4 * lw.U32 * S)
    return {"done": done, "reward": reward, "values": values, "v_term": v_term,
            "adv": adv, "a64": a64, "S": S,
            "td": vl.td_targets_reward_f32(done, reward, values, v_term, GAMMA),
            "lr": vl.lambda_return_f32(adv, values)}


@pytest.mark.parametrize("N", [70, 300])
@pytest.mark.parametrize("T", [1, 7, 8, 9, 17, 1000])
def test_advantages_on_a_callers_window(ctx, T, N):
    """steps > 0 with the caller's reward and done: bit-identical to the
    restatements, and within 4 * 2^-24 * S_t of the float64 forward sum."""
    from dependence_free_rl_amd import VecEnv
    w = _window(T, N)
    env = VecEnv(ctx, num_envs=N, bins=8, dims=1, rng_state=X0)
    got = env.advantages(w["values"], v_term=w["v_term"], reward=w["reward"],
                         done=w["done"], gamma=GAMMA, lam=LAM,
                         returns=("adv", "td_target", "lambda_return"))
    err = np.abs(got["adv"].astype(np.float64) - w["a64"])
    print("T=%d N=%d: max err / (2^-24 S) = %.3f"
          % (T, N, (err / (lw.U32 * w["S"])).max()))
    _assert_bits(got["adv"], w["adv"], "adv")
    _assert_bits(got["td_target"], w["td"], "td_target")
    _assert_bits(got["lambda_return"], w["lr"], "lambda_return")
    assert np.all(err <= 4 * lw.U32 * w["S"])
    np.testing.assert_array_equal(got["stats"][2:],
                                  [T * N, (w["done"] != 0).sum()])
    env.close()


def test_advantages_argument_errors(ctx):
    from dependence_free_rl_amd import VecEnv, XhError, _lib
    N = 12
    env = VecEnv(ctx, num_envs=N, bins=8, dims=1, rng_state=X0)
    v = np.zeros((1, N), np.float32)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_STATE):
        env.advantages(v)  # steps 0 and no record
    a = _lib.VenvAdv()
    a.steps = 3
    a.values = a.adv = env.device_ptr(_lib.VENV_OBS)
    assert _lib.lib.xh_venv_advantages(env.h, C.byref(a)) == _lib.XH_ERR_INVALID
    assert b"reward and done" in _lib.lib.xh_last_error()
    a.steps = -1
    assert _lib.lib.xh_venv_advantages(env.h, C.byref(a)) == _lib.XH_ERR_INVALID
    assert _lib.lib.xh_struct_size(b"xh_venv_adv") == C.sizeof(_lib.VenvAdv)
    env.synchronize()
    env.close()


# --------------------------------------------------------------------- 7 --
def _positive_window(T, N, seed):
    """Rewards in [0.5, 2] and values in [0, 1]: the advantages are mostly
    positive, so their sum does not cancel and a bound relative to the sum is
    a bound relative to the terms."""
    g = np.random.default_rng(seed)
    done = vl.edge_done(T, N, seed)
    reward = g.uniform(0.5, 2.0, (T, N)).astype(np.float32)
    values = g.uniform(0.0, 1.0, (T + 1, N)).astype(np.float32)
    return done, reward, values


@pytest.mark.parametrize("T,N", [(16, 40), (17, 300), (1000, 70)])
def test_normalize_and_stats(ctx, T, N):
    """stats = [sum A, sum A^2, rows, ended rows]: the counts exactly, the
    sums within 2^-50 (relative) of the exact sums -- the device adds the
    float32 advantages (and their exact double squares) in double: a lane's
    sum over its T steps compensated (one rounding), then 6 wave steps, 2
    block steps and adv_stats_kernel's one wave, about 15 roundings of 2^-53
    in the worst case whatever T is.  The normalised advantages are within 2
    float32 ulps of adv_normalize_f64; two runs give the same bits.  (16, 40)
    is the 64-bin record's window with the venv's own rewards."""
    from dependence_free_rl_amd import VecEnv
    if (T, N) == (16, 40):
        env = _recorded(ctx, CASES[2])
        done = _ref_record(CASES[2])[0]["done"]
        reward = np.where(done != 0, 0.0, 1.0).astype(np.float32)
        values = np.random.default_rng(3).uniform(0, 1, (T + 1, N)).astype(
            np.float32)
        args = {}
    else:
        env = VecEnv(ctx, num_envs=N, bins=8, dims=1, rng_state=X0)
        done, reward, values = _positive_window(T, N, T + N)
        args = {"reward": reward, "done": done}
    adv = vl.gae_reward_f32(done, reward, values, GAMMA, LAM)
    want = vl.stats_f64(adv, done)
    a64 = adv.astype(np.float64)
    assert np.abs(a64).sum() <= 2 * abs(want[0]), "the sum does not cancel"
    plain = env.advantages(values, gamma=GAMMA, lam=LAM, **args)
    runs = [env.advantages(values, gamma=GAMMA, lam=LAM, normalize=True,
                           returns=("adv", "lambda_return"), **args)
            for _ in range(2)]
    _assert_bits(plain["adv"], adv)
    for r in runs:
        st = r["stats"]
        rel = np.abs(st[:2] - want[:2]) / np.abs(want[:2])
        print("T=%d N=%d: stats rel err / 2^-53 = %s" % (T, N, rel * 2.0 ** 53))
        np.testing.assert_array_equal(st[2:], want[2:])
        assert np.all(rel <= 2.0 ** -50)
        norm = lw.adv_normalize_f64(adv, adv.size)
        ulps = lw.ulp_distance_f32(r["adv"], norm)
        print("    normalised adv: max %d ulps" % ulps.max())
        assert ulps.max() <= 2
        # the lambda return keeps the un-normalised advantage
        _assert_bits(r["lambda_return"], vl.lambda_return_f32(adv, values))
    assert runs[0]["stats"].tobytes() == runs[1]["stats"].tobytes()
    assert runs[0]["stats"].tobytes() == plain["stats"].tobytes()
    _assert_bits(runs[0]["adv"], runs[1]["adv"])
    env.close()


def test_normalize_zero_variance_is_finite(ctx):
    """Every row terminal with one reward and one value: all advantages are
    equal, the variance is zero, and the normalised output is finite (zero)."""
    from dependence_free_rl_amd import VecEnv
    T, N = 9, 70
    env = VecEnv(ctx, num_envs=N, bins=8, dims=1, rng_state=X0)
    done = np.ones((T, N), np.uint8)
    reward = np.full((T, N), 1.0, np.float32)
    values = np.full((T + 1, N), 0.3, np.float32)
    adv = vl.gae_reward_f32(done, reward, values, GAMMA, LAM)
    assert (adv == adv[0, 0]).all()
    got = env.advantages(values, reward=reward, done=done, gamma=GAMMA,
                         lam=LAM, normalize=True)
    assert np.isfinite(got["adv"]).all()
    np.testing.assert_array_equal(got["adv"], 0.0)
    np.testing.assert_array_equal(got["stats"][2:], [T * N, T * N])
    env.close()


# --------------------------------------------------------------------- 8 --
@pytest.mark.parametrize("case", [CASES[2], CASES[4]], ids=[IDS[2], IDS[4]])
def test_nothing_else_moved(ctx, case):
    """After every new call the venv's bins, items, stream states, record and
    cursor are what they were, and step 17 continues the reference trajectory
    bit for bit."""
    from dependence_free_rl_amd import _lib
    B, D, N = case
    rows, ref = _trajectory(case)
    env = _recorded(ctx, case)

    def state():
        rec = env.record()
        return ([env.get(w) for w in (_lib.VENV_BINS, _lib.VENV_ITEMS,
                                      _lib.VENV_RNG)] +
                [rec[k] for k in sorted(rec)] + [np.array(env.record_pos())])

    before = state()
    np.testing.assert_array_equal(before[0], ref["bins"][STEPS])
    np.testing.assert_array_equal(before[2], ref["rng"][STEPS])
    g = np.random.default_rng(1)
    env.record_obs("state")
    env.record_obs("next", rows=g.permutation(STEPS * N)[:N + 3])
    env.record_ends()
    values = g.normal(0, 1, (STEPS + 1, N)).astype(np.float32)
    env.advantages(values, v_term=values[1:], normalize=True,
                   returns=("adv", "td_target", "lambda_return"))
    done = vl.edge_done(9, N, 2)
    env.advantages(g.normal(0, 1, (10, N)).astype(np.float32),
                   reward=g.normal(0, 1, (9, N)).astype(np.float32), done=done)
    env.synchronize()
    after = state()
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)
    got = env.act(rows[STEPS])
    for name, x in zip(("action", "pchoice", "reward", "done"), got):
        np.testing.assert_array_equal(x, ref[name][STEPS], name)
    b, i = env.view()
    np.testing.assert_array_equal(b, ref["bins"][STEPS + 1])
    np.testing.assert_array_equal(i, ref["item"][STEPS + 1])
    np.testing.assert_array_equal(env.get(_lib.VENV_RNG), ref["rng"][STEPS + 1])
    assert env.record_pos() == STEPS + 1
    env.close()
