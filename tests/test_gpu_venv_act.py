"""GPU parity of xh_venv_act (react's sampling + agent::step in one launch) and
of the trajectory record it writes, against the host reference
tests/venv_act_ref.py (pinned to the oracle by tests/test_venv_act_ref.py).

Shapes: 8 bins (a partial wave), 32 bins 1-D with N = 70, 64 bins 2-D with N
= 40 (a partial last wave), 128 bins 3-D with N = 5 (eight lanes per env), and
one case at 16 bins at an offset inside a larger job."""
import ctypes as C
import functools

import numpy as np
import pytest

from sampling_ties import TIE_TOL, cumulative
from venv_act_ref import (BOUNDARY_N, BOUNDARY_X0, ActRef, boundary_rows,
                          mixed_rows, run)

pytestmark = pytest.mark.gpu

CASES = [(8, 2, 19, 0, 19), (32, 1, 70, 0, 70), (64, 2, 40, 0, 40),
         (128, 3, 5, 0, 5), (16, 3, 9, 6, 21)]
STEPS, X0 = 16, 4242


def _venv(ctx, B, D, N, offset=0, Ng=None, x0=X0, policy_draws=2):
    from dependence_free_rl_amd import VecEnv
    return VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=x0,
                  env_offset=offset, num_envs_global=Ng or N,
                  policy_draws=policy_draws)


@functools.lru_cache(maxsize=None)
def _sampled(case):
    """(rows, reference run) of a case, computed once and left unchanged."""
    B, D, N, offset, Ng = case
    rows = mixed_rows(B * 10 + D, STEPS, N, B)
    ref = run(B, D, N, X0, rows, n_global=Ng, offset=offset)
    resets = ref["done"].any(axis=0)
    assert resets.any() and not resets.all(), "resets: some envs, not all"
    return rows, ref


def _assert_state(env, bins, item, rng=None):
    from dependence_free_rl_amd._lib import VENV_RNG
    b, i = env.view()
    np.testing.assert_array_equal(b, bins)
    np.testing.assert_array_equal(i, item)
    if rng is not None:
        np.testing.assert_array_equal(env.get(VENV_RNG), rng)


@pytest.mark.parametrize("via", ["buffer", "pointer"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-D%d-N%d-o%d-Ng%d" % c)
def test_probs_sample_is_the_reference_bit_for_bit(ctx, case, via):
    """PROBS / SAMPLE: actions, PCHOICE, reward, done, bins, items, the stream
    states and OBS equal the reference at every step -- through the venv's own
    XH_VENV_POLICY buffer and through a pointer from xh_tensor_alloc."""
    from dependence_free_rl_amd import _lib
    B, D, N, offset, Ng = case
    rows, ref = _sampled(case)
    env = _venv(ctx, B, D, N, offset, Ng)
    lib = _lib.lib
    dev = C.POINTER(C.c_float)()
    if via == "pointer":
        lib.xh_tensor_alloc.argtypes = [C.c_void_p, C.c_size_t,
                                        C.POINTER(C.POINTER(C.c_float))]
        lib.xh_tensor_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_size_t, C.c_int]
        lib.xh_tensor_free.argtypes = [C.c_void_p, C.c_void_p]
        _lib.check(lib.xh_tensor_alloc(ctx.h, N * B, C.byref(dev)))
        addr = C.cast(dev, C.c_void_p).value
    _assert_state(env, ref["bins"][0], ref["item"][0], ref["rng"][0])
    for s in range(STEPS):
        if via == "pointer":
            r = np.ascontiguousarray(rows[s])
            _lib.check(lib.xh_tensor_copy(ctx.h, addr, r.ctypes.data, N * B, 0))
            got = env.act(addr, write_obs=True)
        else:
            got = env.act(rows[s], write_obs=True)
        for name, g in zip(("action", "pchoice", "reward", "done"), got):
            np.testing.assert_array_equal(g, ref[name][s], err_msg="%s, step %d"
                                          % (name, s))
        _assert_state(env, ref["bins"][s + 1], ref["item"][s + 1],
                      ref["rng"][s + 1])
        np.testing.assert_array_equal(env.get(_lib.VENV_OBS), ref["obs"][s + 1])
    if via == "pointer":
        _lib.check(lib.xh_tensor_free(ctx.h, addr))
    env.close()


@pytest.mark.parametrize("B", [8, 64, 128])
def test_boundary_rows_take_the_exact_path(ctx, B):
    """Rows whose second cumulative boundary lies within rounding of the
    env's draw u, and their one-ulp neighbours on the other side of u
    (test_venv_act_ref.py proves the construction): the device's pick is
    or_discrete's on both, which the unnormalised tree sums alone cannot
    promise -- the sampler's sequential restatement, run deterministically."""
    D, N = 2, BOUNDARY_N
    us = ActRef(B, D, N, BOUNDARY_X0).draws()
    pairs = [boundary_rows(u, B) for u in us]
    made = [e for e in range(N) if pairs[e] is not None]
    assert len(made) >= 4
    picks = []
    for side in (0, 1):
        rows = np.zeros((N, B), np.float32)
        rows[:, 3] = 1.0
        for e in made:
            rows[e] = pairs[e][side]
        want = ActRef(B, D, N, BOUNDARY_X0).act(rows)
        env = _venv(ctx, B, D, N, x0=BOUNDARY_X0)
        act, pch, _, _ = env.act(rows)
        env.close()
        np.testing.assert_array_equal(act, want["action"])
        np.testing.assert_array_equal(pch, want["pchoice"])
        picks.append(act[made])
    assert set(np.unique(picks[0] + picks[1])) == {3}  # bins 1 and 2, each once


@pytest.mark.parametrize("case", [(8, 2, 19), (64, 2, 40), (128, 3, 5)],
                         ids=lambda c: "B%d-D%d-N%d" % c)
def test_argmax_first_maximum_and_no_draws(ctx, case):
    """ARGMAX: ties go to the lowest bin; nothing is drawn (the streams of a
    policy_draws = 0 or_venv_run); on a policy_draws = 2 venv the two draws
    are skipped as xh_venv_step skips them; SAMPLE needs policy_draws = 2."""
    from oracle import pyoracle as po
    from dependence_free_rl_amd import XhError
    from dependence_free_rl_amd._lib import VENV_RNG
    B, D, N = case
    S = 12
    rows = mixed_rows(B + 1, S, N, B)
    top = rows.max(axis=2)
    rows[:, :, B - 1] = top          # a repeated maximum in every row ...
    rows[:, 1::2, B // 2] = top[:, 1::2]  # ... and a third in every other
    for pd in (0, 2):
        ref = run(B, D, N, X0, rows, mode="argmax", policy_draws=pd)
        np.testing.assert_array_equal(ref["action"], rows.argmax(axis=2))
        env = _venv(ctx, B, D, N, policy_draws=pd)
        for s in range(S):
            got = env.act(rows[s], mode="argmax")
            for name, g in zip(("action", "pchoice", "reward", "done"), got):
                np.testing.assert_array_equal(g, ref[name][s])
            _assert_state(env, ref["bins"][s + 1], ref["item"][s + 1],
                          ref["rng"][s + 1])
        drv = po.venv_run(B, D, N, X0, ref["action"], policy_draws=pd)
        assert env.get(VENV_RNG)[0] == drv["x_end"]
        if pd == 0:
            with pytest.raises(XhError, match="policy_draws"):
                env.act(rows[0], mode="sample")
            _assert_state(env, ref["bins"][S], ref["item"][S], ref["rng"][S])
        env.close()


# seeds at which no draw of the reference trajectory lies within TIE_TOL of a
# cumulative boundary (asserted below, on the CPU, before the device runs)
LOGIT_CASES = [(8, 2, 19, 1), (64, 2, 40, 13), (128, 3, 5, 17)]


def _softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


@pytest.mark.parametrize("case", LOGIT_CASES, ids=lambda c: "B%d-D%d-N%d-s%d" % c)
def test_logits_softmax_and_picks(ctx, case):
    """LOGITS: PCHOICE within (B + 4) 2^-24 (relative) of a float64 softmax --
    one-ulp expf on both sides, an f32 sum of B positive terms, one division;
    the picks and states equal the reference's on the float64 softmax's rows,
    no draw of that trajectory lying within 1e-4 of a boundary."""
    B, D, N, seed = case
    S = 12
    g = np.random.default_rng(seed)
    z = (g.standard_normal((S, N, B)) * 6.0).astype(np.float32)
    z[:, ::4, 0] = 12.0  # peaked at bin 0: those envs overflow and reset
    p64 = _softmax64(z)
    ref = run(B, D, N, X0, p64.astype(np.float32))
    resets = ref["done"].any(axis=0)
    assert resets.any() and not resets.all()
    for s in range(S):
        for e in range(N):
            cp = cumulative(p64[s, e].astype(np.float32))[:-1]
            assert np.abs(cp - ref["u"][s, e]).min() > TIE_TOL, (s, e)
    env = _venv(ctx, B, D, N)
    for s in range(S):
        act, pch, reward, done = env.act(z[s], kind="logits")
        np.testing.assert_array_equal(act, ref["action"][s])
        want = p64[s, np.arange(N), act]
        print("logits B=%d step %d: max rel PCHOICE error %.3g (bound %.3g)"
              % (B, s, np.abs(pch / want - 1).max(), (B + 4) * 2.0 ** -24))
        assert np.all(np.abs(pch - want) <= (B + 4) * 2.0 ** -24 * want)
        np.testing.assert_array_equal(reward, ref["reward"][s])
        np.testing.assert_array_equal(done, ref["done"][s])
        _assert_state(env, ref["bins"][s + 1], ref["item"][s + 1],
                      ref["rng"][s + 1])
    env.close()


@pytest.mark.parametrize("case", [CASES[0], CASES[3]],
                         ids=lambda c: "B%d-D%d-N%d-o%d-Ng%d" % c)
def test_record_is_what_the_steps_returned(ctx, case):
    """After T calls the record holds what the step-by-step gets returned,
    the states before each step included; call T + 1 is XH_ERR_STATE; after a
    rewind the next call writes slot 0; off, the record has no bytes."""
    from dependence_free_rl_amd import XhError, _lib
    B, D, N, offset, Ng = case
    rows, ref = _sampled(case)
    T = 6
    env = _venv(ctx, B, D, N, offset, Ng)
    bytes_of = lambda w: _lib.lib.xh_venv_record_bytes(env.h, w)  # noqa: E731
    assert all(bytes_of(w) == 0 for w in range(_lib.VREC_COUNT))
    assert env.record() == {}
    env.set_record(T)
    assert bytes_of(_lib.VREC_ACTION) == T * N * 4
    assert bytes_of(_lib.VREC_BINS) == T * N * B * D
    seen = {k: [] for k in ("action", "pchoice", "reward", "done", "bins",
                            "items")}
    for s in range(T):
        b, _ = env.view()
        seen["bins"].append(b)
        seen["items"].append(env.get(_lib.VENV_ITEMS))
        got = env.act(rows[s])
        for name, g in zip(("action", "pchoice", "reward", "done"), got):
            seen[name].append(g)
        assert env.record_pos() == s + 1
    rec = env.record()
    for name in seen:
        np.testing.assert_array_equal(rec[name], np.stack(seen[name]), name)
    np.testing.assert_array_equal(rec["action"], ref["action"][:T])
    np.testing.assert_array_equal(rec["bins"], ref["bins"][:T])
    np.testing.assert_array_equal(rec["items"][:, :, :D], ref["item"][:T])
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_STATE):
        env.act(rows[T])
    _assert_state(env, ref["bins"][T], ref["item"][T], ref["rng"][T])
    env.rewind()
    got = env.act(rows[T])
    rec = env.record()
    assert env.record_pos() == 1 and len(rec["action"]) == 1
    np.testing.assert_array_equal(rec["action"][0], got[0])
    np.testing.assert_array_equal(rec["action"][0], ref["action"][T])
    np.testing.assert_array_equal(rec["bins"][0], ref["bins"][T])
    env.step(fetch=False)  # step / apply / reset do not record
    assert env.record_pos() == 1
    env.set_record(3, states=False)  # a record without the states
    env.act(rows[0], fetch=False)
    rec = env.record()
    assert sorted(rec) == ["action", "done", "pchoice", "reward"]
    assert bytes_of(_lib.VREC_BINS) == 0 and bytes_of(_lib.VREC_DONE) == 3 * N
    env.set_record(0)
    assert all(bytes_of(w) == 0 for w in range(_lib.VREC_COUNT))
    env.act(rows[1], fetch=False)  # off: not bounded by a cursor
    env.synchronize()
    env.close()


@pytest.mark.parametrize("case", [(8, 2, 19), (128, 3, 5)],
                         ids=lambda c: "B%d-D%d-N%d" % c)
def test_bad_rows_are_refused(ctx, case):
    """A NaN row, a negative entry and an all-zero row: each env keeps its
    state and stream, its DONE is 0, synchronize reports XH_ERR_INVALID, the
    other envs of the call match the reference -- and the record's slot of a
    refused env is zero."""
    from dependence_free_rl_amd import XhError, _lib
    B, D, N = case
    rows = mixed_rows(5, 3, N, B)
    ref = ActRef(B, D, N, X0)
    env = _venv(ctx, B, D, N)
    env.set_record(2)
    want0 = ref.act(rows[0])
    got = env.act(rows[0])  # a clean step first: done flags to overwrite
    np.testing.assert_array_equal(got[0], want0["action"])
    bad = rows[1].copy()
    refuse = (1, 2, 4)
    bad[1, B - 1] = np.nan
    bad[2, 0] = -0.125
    bad[4, :] = 0.0
    before = (ref.bins(), ref.items(), ref.streams())
    want = ref.act(bad, refuse=refuse)
    env.act(bad, fetch=False)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.synchronize()
    env.synchronize()  # reported once
    ok = np.array([e not in refuse for e in range(N)])
    rng = env.get(_lib.VENV_RNG)
    _assert_state(env, ref.bins(), ref.items())
    np.testing.assert_array_equal(rng[ok], ref.streams()[ok])
    for e in refuse:
        np.testing.assert_array_equal(ref.bins()[e], before[0][e])
        assert rng[e] == before[2][e]
    done = env.get(_lib.VENV_DONE)
    assert (done[~ok] == 0).all()
    np.testing.assert_array_equal(done[ok], want["done"][ok])
    for which, name in ((_lib.VENV_ACTIONS, "action"),
                        (_lib.VENV_PCHOICE, "pchoice"),
                        (_lib.VENV_REWARD, "reward")):
        np.testing.assert_array_equal(env.get(which)[ok], want[name][ok])
    rec = env.record()
    for name in ("action", "pchoice", "reward", "done"):
        np.testing.assert_array_equal(rec[name][1], want[name], name)
    np.testing.assert_array_equal(rec["bins"][1], before[0])
    env.close()


def test_act_and_step_interleave(ctx):
    """A venv driven by act and step calls in turn matches the reference
    driven the same way."""
    from dependence_free_rl_amd._lib import VENV_DONE, VENV_REWARD
    B, D, N, offset, Ng = CASES[4]
    rows = mixed_rows(11, 14, N, B)
    g = np.random.default_rng(2)
    ref = ActRef(B, D, N, X0, n_global=Ng, offset=offset)
    env = _venv(ctx, B, D, N, offset, Ng)
    for s in range(14):
        if s % 3 == 1:
            acts = g.integers(0, 2, N).astype(np.int32)
            want = ref.step(acts)
            env.set_actions(acts)
            env.step(fetch=False)
        else:
            mode = "argmax" if s % 3 == 2 else "sample"
            want = ref.act(rows[s], mode)
            got = env.act(rows[s], mode=mode)
            np.testing.assert_array_equal(got[0], want["action"])
            np.testing.assert_array_equal(got[1], want["pchoice"])
        np.testing.assert_array_equal(env.get(VENV_REWARD), want["reward"])
        np.testing.assert_array_equal(env.get(VENV_DONE), want["done"])
        _assert_state(env, ref.bins(), ref.items(), ref.streams())
    env.close()
