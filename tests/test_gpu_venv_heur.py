"""GPU tests of xh_venv_act_heuristic (VecEnv.act_heuristic, the four heuristic
agents as an act of the venv; heuristic_baseline) against the host restatement
tests/venv_heur_ref.py (pinned to the oracle by tests/test_venv_heur_ref.py,
which also asserts that these fixtures contain resets, steps where nothing
fits, exact best-fit ties and maxima that are no multiple of 1/8) and against
xh_venv_act of the same library on host-computed score rows.

Shapes: test_gpu_venv_items' -- 8 bins 2-D N = 19 (a partial wave), 32 bins 1-D
N = 70, 64 bins 2-D N = 40 (a partial last wave), 128 bins 3-D N = 5 (eight
lanes per env) and sharded cases at an offset inside a larger job; the builtin
instance and four custom sets, one with zero entries.  The bins are preset to
seeded near-full states, so every run of 24 steps has all of that."""
import numpy as np
import pytest

import venv_episode_ref as er
import venv_heur_ref as hr

pytestmark = pytest.mark.gpu

SETUP_NAMES = list(hr.SETUPS)


def _venv(ctx, name, kind, **kw):
    """A VecEnv on SETUPS[name] for `kind`, its bins preset as the
    restatement's."""
    from dependence_free_rl_amd import VecEnv, _lib
    case, items, weights, capacity = hr.SETUPS[name]
    B, D, N, offset, Ng = case
    if items is not None:
        kw.update(items=items, weights=weights, capacity=capacity)
    env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=hr.X0,
                 env_offset=offset, num_envs_global=Ng,
                 policy_draws=2 if kind == "random" else 0, **kw)
    env.set(_lib.VENV_BINS, hr.trajectory(name, kind)["preset"])
    return env


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _buffers(env, pchoice=True):
    from dependence_free_rl_amd import _lib
    which = [_lib.VENV_ACTIONS, _lib.VENV_REWARD, _lib.VENV_DONE,
             _lib.VENV_BINS, _lib.VENV_ITEMS, _lib.VENV_RNG, _lib.VENV_OBS,
             _lib.VENV_MASK]
    if pchoice:
        which.append(_lib.VENV_PCHOICE)
    return {w: env.get(w) for w in which}


def _check_step(env, want, D, what):
    from dependence_free_rl_amd import _lib
    for name, which in (("action", _lib.VENV_ACTIONS),
                        ("pchoice", _lib.VENV_PCHOICE),
                        ("reward", _lib.VENV_REWARD), ("done", _lib.VENV_DONE),
                        ("rng", _lib.VENV_RNG), ("obs", _lib.VENV_OBS)):
        _same(env.get(which), want[name], "%s, %s" % (name, what))
    b, it = env.view()
    _same(b, want["bins"], "bins, " + what)
    _same(it, want["item"], "items, " + what)


# --------------------------------------------- 1. against the restatement --
@pytest.mark.parametrize("kind", hr.KINDS)
@pytest.mark.parametrize("name", SETUP_NAMES)
def test_every_step_is_the_restatement_bit_for_bit(ctx, name, kind):
    """After every step: action, PCHOICE (1.0f, or (float)(1 / B)), reward,
    done, bins, items, stream states and OBS equal the restatement's bytes."""
    from dependence_free_rl_amd import _lib
    case = hr.SETUPS[name][0]
    B, D = case[:2]
    t = hr.trajectory(name, kind)
    env = _venv(ctx, name, kind)
    _same(env.view()[1], t["first"]["item"], "items at construction")
    _same(env.get(_lib.VENV_RNG), t["first"]["rng"], "streams at construction")
    for s, want in enumerate(t["steps"]):
        got = env.act_heuristic(kind, write_obs=True, fetch=True)
        _same(got[0], want["action"], "fetched action, step %d" % s)
        _check_step(env, want, D, "step %d" % s)
        pc = np.float32(1.0 / B) if kind == "random" else np.float32(1.0)
        assert (got[1] == pc).all()
    env.close()


# -------------------------------------------------- 2. device against device --
@pytest.mark.parametrize("kind", hr.DETERMINISTIC)
@pytest.mark.parametrize("name", SETUP_NAMES)
def test_deterministic_kinds_equal_act_argmax_on_host_scores(ctx, name, kind):
    """A second venv on the same seed driven by act(scores, "logits",
    "argmax") with score rows computed on the host from its own bins and
    items: every buffer but POLICY / PCHOICE identical at every step."""
    case = hr.SETUPS[name][0]
    B, D, N = case[:3]
    a = _venv(ctx, name, kind)
    b = _venv(ctx, name, kind)
    cap = a.item_set()["capacity"]
    ended = 0
    for s in range(hr.STEPS):
        bins, items = b.view()
        rows = np.stack([hr.scores(kind, bins[e], items[e], cap)
                         for e in range(N)])
        a.act_heuristic(kind, write_obs=True)
        b.act(rows, kind="logits", mode="argmax", write_obs=True, fetch=False)
        x, y = _buffers(a, False), _buffers(b, False)
        for w in x:
            _same(x[w], y[w], "buffer %d, step %d" % (w, s))
        ended += int(x[2].sum())
    assert ended > 0
    a.close()
    b.close()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("name", SETUP_NAMES)
def test_random_equals_act_sample_on_the_constant_row(ctx, name, masked):
    """The second venv runs act(const_row, "probs", "sample"): every buffer
    including PCHOICE identical, with the action mask off and on."""
    case = hr.SETUPS[name][0]
    B, D, N = case[:3]
    rows = np.full((N, B), np.float32(1.0 / B), np.float32)
    a = _venv(ctx, name, "random")
    b = _venv(ctx, name, "random")
    for env in (a, b):
        env.set_action_mask(masked)
    t = hr.trajectory(name, "random", masked)
    for s in range(hr.STEPS):
        a.act_heuristic("random", write_obs=True)
        b.act(rows, kind="probs", mode="sample", write_obs=True, fetch=False)
        x, y = _buffers(a), _buffers(b)
        for w in x:
            _same(x[w], y[w], "buffer %d, step %d" % (w, s))
        _same(x[0], t["steps"][s]["action"], "action, step %d" % s)
    a.close()
    b.close()


# ------------------------------------------------------------- 3. record --
@pytest.mark.parametrize("kind", hr.KINDS)
@pytest.mark.parametrize("name", ["default-B64-D2", "K5-cap57-sharded",
                                  "K3-cap683-B128"])
def test_the_record_is_the_restatements_trajectory(ctx, name, kind):
    """set_record(T, states=True): the six arrays equal the trajectory; the
    call on a full record is XH_ERR_STATE; rewind starts over."""
    from dependence_free_rl_amd import _lib
    case = hr.SETUPS[name][0]
    D = case[1]
    t = hr.trajectory(name, kind)
    T = len(t["steps"])
    env = _venv(ctx, name, kind)
    env.set_record(T, states=True)
    for s in range(T):
        env.act_heuristic(kind)
    assert env.record_pos() == T
    rec = env.record()
    assert sorted(rec) == ["action", "bins", "done", "items", "pchoice",
                           "reward"]
    before = [t["first"]] + t["steps"][:-1]
    for name_ in ("action", "pchoice", "reward", "done"):
        _same(rec[name_], np.stack([s[name_] for s in t["steps"]]),
              "record " + name_)
    _same(rec["bins"], np.stack([s["bins"] for s in before]), "record bins")
    _same(rec["items"][:, :, :D], np.stack([s["item"] for s in before]),
          "record items")
    assert not rec["items"][:, :, D:].any()
    state = _buffers(env)
    st = _lib.lib.xh_venv_act_heuristic(env.h, _lib.HEURISTICS[kind], 0)
    assert st == _lib.XH_ERR_STATE
    assert b"full" in _lib.lib.xh_last_error()
    after = _buffers(env)
    for w in state:
        _same(after[w], state[w], "buffer %d after the refusal" % w)
    assert env.record_pos() == T
    env.rewind()
    assert env.record_pos() == 0
    bins_before = env.get(_lib.VENV_BINS)
    got = env.act_heuristic(kind, fetch=True)
    assert env.record_pos() == 1
    rec = env.record()
    _same(rec["action"][0], got[0], "slot 0 after the rewind")
    _same(rec["bins"][0], bins_before, "slot 0's state after the rewind")
    env.close()


@pytest.mark.parametrize("kind", hr.KINDS)
@pytest.mark.parametrize("name", ["default-B8-D2", "K16-cap75-B64",
                                  "zero-cap64-sharded", "default-B128-D3"])
def test_masked_run_records_the_legal_words(ctx, name, kind):
    """With the action mask on the legal-word record equals legal() of each
    pre-step state; the deterministic actions equal the unmasked run's and
    random's equal the restatement's masked run."""
    t = hr.trajectory(name, kind, kind == "random")
    T = len(t["steps"])
    env = _venv(ctx, name, kind)
    env.set_action_mask(True)
    env.set_record(T, states=True)
    before = [t["first"]] + t["steps"][:-1]
    for s in range(T):
        if s % 6 == 0:
            _same(env.legal(), before[s]["legal"], "legal(), step %d" % s)
        env.act_heuristic(kind)
    rec = env.record()
    _same(rec["legal"], np.stack([s["legal"] for s in before]),
          "record legal")
    assert not rec["legal"].all() and rec["legal"].all(axis=2).any()
    for name_ in ("action", "pchoice", "reward", "done"):
        _same(rec[name_], np.stack([s[name_] for s in t["steps"]]),
              "record " + name_)
    env.close()


# ------------------------------------------------- 4. episode statistics --
@pytest.mark.parametrize("kind", hr.KINDS)
@pytest.mark.parametrize("name", ["default-B8-D2", "K16-cap75-B64",
                                  "K5-cap57-sharded"])
def test_episode_rows_equal_the_episode_restatement(ctx, name, kind):
    """Rows after 10 and after all steps equal venv_episode_ref fed with the
    restatement's done flags (the statistics are switched on after the
    preset: set(VENV_BINS) restarts the running lengths)."""
    t = hr.trajectory(name, kind)
    done = np.stack([s["done"] for s in t["steps"]]) != 0
    S, N = done.shape
    want, running, first, _ = er.rows_of_history(done, np.ones((S, N), bool),
                                                 [10, S])
    assert want[:, er.EPISODES].sum() == done.sum() > 0
    env = _venv(ctx, name, kind)
    env.set_episode_stats(4)
    for s in range(S):
        if s == 10:
            env.episode_row()
        env.act_heuristic(kind)
    env.episode_row()
    got = env.episode_stats()
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), (got, want)
    r, f = env.episode_state()
    _same(r, running, "running")
    _same(f, first, "first")
    env.close()


# ------------------------------------------------------------ 5. refusals --
def test_refusals_leave_the_venv_unchanged(ctx):
    """Random on a venv with policy_draws == 0 is XH_ERR_INVALID, any kind with
    a distribution record on is XH_ERR_STATE, an unknown kind is
    XH_ERR_INVALID; the buffers and the record's cursor stay."""
    from dependence_free_rl_amd import XhError, _lib
    lib = _lib.lib
    name = "K5-cap57-B8"
    env = _venv(ctx, name, "firstfit")          # policy_draws 0
    env.set_record(4, states=True)
    env.act_heuristic("bestfit", write_obs=True)
    state, pos = _buffers(env), env.record_pos()
    assert pos == 1

    def unchanged(what):
        after = _buffers(env)
        for w in state:
            _same(after[w], state[w], "buffer %d after %s" % (w, what))
        assert env.record_pos() == pos, what

    assert lib.xh_venv_act_heuristic(env.h, _lib.HEURISTICS["random"], 1) == \
        _lib.XH_ERR_INVALID
    assert b"policy_draws" in lib.xh_last_error()
    unchanged("random without draws")
    with pytest.raises(XhError, match="policy_draws"):
        env.act_heuristic("random")
    for bad in (-1, 4, 99):
        assert lib.xh_venv_act_heuristic(env.h, bad, 1) == _lib.XH_ERR_INVALID
        assert b"heuristic" in lib.xh_last_error()
    unchanged("an unknown kind")
    env.close()
    for kind in hr.KINDS:
        env = _venv(ctx, name, kind)
        env.set_record(4, states=True, distrib=True)
        state, pos = _buffers(env), env.record_pos()
        assert lib.xh_venv_act_heuristic(env.h, _lib.HEURISTICS[kind], 1) == \
            _lib.XH_ERR_STATE
        assert b"distribution" in lib.xh_last_error()
        unchanged("%s with a distribution record" % kind)
        # off again: the call goes through
        assert lib.xh_venv_set_record_distrib(env.h, 0) == _lib.XH_OK
        env.act_heuristic(kind)
        assert env.record_pos() == 1
        env.close()


# ------------------------------------------------------- 6. set_item_set --
@pytest.mark.parametrize("kind", ["bestfit", "random"])
def test_set_item_set_mid_run_draws_from_the_new_set(ctx, kind):
    name = "K5-cap57-B8"
    case = hr.SETUPS[name][0]
    D = case[1]
    new = ([(2, 3), (1, 1), (4, 5)], [1.0, 2.0, 1.0])
    ref, preset = hr.make_ref(name, kind)
    env = _venv(ctx, name, kind)
    from dependence_free_rl_amd import _lib
    for s in range(16):
        if s == 5:
            ref.set_item_set(*new)
            env.set_item_set(*new)
            _same(env.view()[1], ref.items(), "held items stay")
        before = ref.items().copy()
        want = ref.act_heuristic(kind)
        got = env.act_heuristic(kind, fetch=True)
        _same(got[0], want["action"], "action, step %d" % s)
        _same(got[3], want["done"], "done, step %d" % s)
        b, it = env.view()
        _same(b, ref.bins(), "bins, step %d" % s)
        _same(it, ref.items(), "items, step %d" % s)
        _same(env.get(_lib.VENV_RNG), ref.streams(), "streams, step %d" % s)
        if s >= 5:
            drawn = {tuple(x) for x, y in zip(it, before)
                     if tuple(x) != tuple(y)}
            assert drawn <= {tuple(x) for x in new[0]}, s
    assert (ref.items()[:, None, :] == np.asarray(new[0])[None]).all(2).any(1) \
        .all(), "every env holds an item of the new set by now"
    env.close()


# ------------------------------------------------- 7. heuristic_baseline --
@pytest.mark.parametrize("kind", ["firstfit", "random"])
def test_heuristic_baseline_first_episode_mean_is_exact(ctx, kind):
    """8 bins, 2-D, the default instance, 300 envs from full bins: the
    first-episode statistics equal the restatement's over the same envs
    (integers summed, so exactly)."""
    from dependence_free_rl_amd import heuristic_baseline
    B, D, N, x0 = 8, 2, 300, 777
    ref = hr.HeurRef(B, D, N, x0, policy_draws=2 if kind == "random" else 0)
    first = np.full(N, -1, np.int64)
    steps = 0
    while (first < 0).any():
        steps += 1
        assert steps < 400
        done = ref.act_heuristic(kind)["done"] != 0
        first[done & (first < 0)] = steps
    # every env runs from construction, so its first length is the step count
    row_every = 16
    got = heuristic_baseline(ctx, kind, B, D, N, rng_state=x0,
                             row_every=row_every)
    assert got["finished"] and got["episodes"] == N
    assert got["len_mean"] == float(first.sum()) / N
    assert got["return_mean"] == float(first.sum()) / N - 1.0
    assert (got["len_min"], got["len_max"]) == (first.min(), first.max())
    assert got["steps"] == -(-steps // row_every) * row_every
    few = heuristic_baseline(ctx, kind, B, D, N, rng_state=x0, max_steps=3,
                             row_every=2)
    assert few["steps"] == 3 and not few["finished"]
    assert few["episodes"] == int((first <= 3).sum())


def test_heuristic_baseline_on_a_custom_set(ctx):
    from dependence_free_rl_amd import heuristic_baseline
    got = {k: heuristic_baseline(ctx, k, 8, 2, 64, items=hr.ITEMS5,
                                 weights=hr.WEIGHTS5, capacity=hr.CAP57,
                                 rng_state=5, row_every=8)
           for k in ("random", "firstfit")}
    assert all(g["finished"] for g in got.values())
    # packing by a rule fills the bins; picking blindly overflows one at once
    assert got["firstfit"]["len_mean"] > 2 * got["random"]["len_mean"]
