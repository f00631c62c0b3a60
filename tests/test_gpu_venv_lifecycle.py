"""GPU tests of the VecEnv's allocation state machine: which of the record's
eight arrays (the six XH_VREC_* ones, the distributions, the legal words)
exist after each xh_venv_set_record / set_action_mask / set_record_distrib,
with which sizes, what the refusals leave behind, and who frees the context.
No kernel's arithmetic is checked here (test_gpu_venv_act.py and its siblings
do that); every call is made on the C ABI so that the status codes show.

Shapes: the smallest that take every branch -- 3 envs, 8 bins (one legal word
per env), 1 dim, policy_draws 2, a record of 2 steps."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, B, D, T = 3, 8, 1, 2
DISTRIB, LEGAL = 6, 7            # after the six XH_VREC_* arrays
NAMES = ("venv record %d", "venv record distrib", "venv record legal")


def _venv(ctx):
    from dependence_free_rl_amd import VecEnv
    return VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7, policy_draws=2)


def _want(steps, states, distrib, legal):
    """The header's byte counts of the eight arrays."""
    from dependence_free_rl_amd import legal_words
    TN = steps * N
    return [TN * 4, TN * 4, TN * 4, TN, TN * B * D if states else 0,
            TN * 4 if states else 0, TN * B * 4 if distrib else 0,
            TN * legal_words(B) * 4 if legal else 0]


def _sizes(env):
    """(bytes, pointer) of the eight arrays; a pointer is non-NULL exactly
    when its byte count is non-zero."""
    from dependence_free_rl_amd import _lib
    lib, h = _lib.lib, env.h
    got = [(lib.xh_venv_record_bytes(h, w), lib.xh_venv_record_ptr(h, w))
           for w in range(_lib.VREC_COUNT)]
    got.append((lib.xh_venv_record_distrib_bytes(h),
                lib.xh_venv_record_distrib_ptr(h)))
    got.append((lib.xh_venv_record_legal_bytes(h),
                lib.xh_venv_record_legal_ptr(h)))
    for nbytes, ptr in got:
        assert bool(ptr) == (nbytes != 0), got
    return [nbytes for nbytes, _ in got]


def _get(env, which, buf, nbytes):
    from dependence_free_rl_amd import _lib
    lib = _lib.lib
    if which == DISTRIB:
        return lib.xh_venv_get_record_distrib(env.h, buf, nbytes)
    if which == LEGAL:
        return lib.xh_venv_get_record_legal(env.h, buf, nbytes)
    return lib.xh_venv_get_record(env.h, which, buf, nbytes)


def _contents(env):
    """The bytes of every array that exists, by index."""
    from dependence_free_rl_amd import _lib
    out = {}
    for which, nbytes in enumerate(_sizes(env)):
        if nbytes:
            buf = C.create_string_buffer(nbytes)
            assert _get(env, which, buf, nbytes) == _lib.XH_OK, which
            out[which] = buf.raw
    return out


def _all_zero(env):
    return all(not any(raw) for raw in _contents(env).values())


def _full(env):
    """All eight arrays: a record with states, the mask, the distributions."""
    env.set_record(T, states=True, distrib=True)
    env.set_action_mask(True)
    assert _sizes(env) == _want(T, True, True, True)


def _last_error():
    from dependence_free_rl_amd import _lib
    return _lib.lib.xh_last_error().decode()


# --------------------------------------------------------------------- 1 --
def test_a_fresh_venv_holds_no_record(ctx):
    from dependence_free_rl_amd import _lib
    lib, env = _lib.lib, _venv(ctx)
    assert _sizes(env) == [0] * 8
    buf = C.create_string_buffer(16)
    for which in (-1, _lib.VREC_COUNT):
        assert lib.xh_venv_record_bytes(env.h, which) == 0
        assert lib.xh_venv_record_ptr(env.h, which) is None
        assert lib.xh_venv_get_record(env.h, which, buf, 0) == \
            _lib.XH_ERR_INVALID
        assert "venv record %d:" % which in _last_error()
    env.close()


# --------------------------------------------------------------------- 2 --
def test_the_record_states_in_order(ctx):
    from dependence_free_rl_amd import _lib
    lib, env = _lib.lib, _venv(ctx)
    env.set_record(T, states=True)
    assert _sizes(env) == _want(T, True, False, False) and _all_zero(env)
    env.set_action_mask(True)
    assert _sizes(env) == _want(T, True, False, True) and _all_zero(env)
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_OK
    assert _sizes(env) == _want(T, True, True, True) and _all_zero(env)
    env.close()


# --------------------------------------------------------------------- 3 --
def test_the_mask_first_gives_the_same_end_state(ctx):
    from dependence_free_rl_amd import _lib
    lib, env = _lib.lib, _venv(ctx)
    env.set_action_mask(True)               # no record yet: nothing to hold
    assert _sizes(env) == [0] * 8
    env.set_record(T, states=True)          # the second of the two allocates
    assert _sizes(env) == _want(T, True, False, True) and _all_zero(env)
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_OK
    assert _sizes(env) == _want(T, True, True, True) and _all_zero(env)
    env.close()


# --------------------------------------------------------------------- 4 --
def test_options_at_a_non_zero_cursor(ctx):
    from dependence_free_rl_amd import _lib
    lib, env = _lib.lib, _venv(ctx)
    _full(env)
    act = lambda: lib.xh_venv_act(env.h, None, _lib.ACT_LOGITS,
                                  _lib.ACT_SAMPLE, 0)
    assert act() == _lib.XH_OK and act() == _lib.XH_OK  # all-zero logits
    env.synchronize()
    assert env.record_pos() == T
    assert act() == _lib.XH_ERR_STATE and "slots are full" in _last_error()
    assert env.record_pos() == T
    before = _contents(env)
    assert sorted(before) == list(range(8))
    assert lib.xh_venv_set_record_distrib(env.h, 1) == _lib.XH_ERR_STATE
    assert "the cursor is at %d" % T in _last_error()
    assert lib.xh_venv_set_action_mask(env.h, 1) == _lib.XH_ERR_STATE
    assert "cursor is at %d" % T in _last_error()
    assert _sizes(env) == _want(T, True, True, True)
    assert _contents(env) == before
    # off is allowed anywhere: only the legal words go
    assert lib.xh_venv_set_action_mask(env.h, 0) == _lib.XH_OK
    assert _sizes(env) == _want(T, True, True, False)
    del before[LEGAL]
    assert _contents(env) == before
    assert env.record_pos() == T
    env.close()


# --------------------------------------------------------------------- 5 --
def test_dropping_the_record(ctx):
    from dependence_free_rl_amd import _lib
    lib, env = _lib.lib, _venv(ctx)
    _full(env)
    env.set_record(0)
    assert _sizes(env) == [0] * 8
    env.set_action_mask(False)
    env.set_record(T, states=False)
    assert _sizes(env) == _want(T, False, False, False) and _all_zero(env)
    assert lib.xh_venv_record_bytes(env.h, _lib.VREC_BINS) == 0
    assert lib.xh_venv_record_bytes(env.h, _lib.VREC_ITEMS) == 0
    assert lib.xh_venv_record_obs(env.h, _lib.VOBS_STATE, None, 0, N,
                                  None) == _lib.XH_ERR_STATE
    assert "the record was made without states" in _last_error()
    env.close()


# --------------------------------------------------------------------- 6 --
def test_a_wrong_size_names_its_array(ctx):
    from dependence_free_rl_amd import _lib
    env = _venv(ctx)
    _full(env)
    for which, nbytes in enumerate(_sizes(env)):
        name = NAMES[max(0, which - DISTRIB + 1)]
        if which < DISTRIB:
            name = name % which
        for off in (-1, 1):
            buf = C.create_string_buffer(nbytes + 1)
            assert _get(env, which, buf, nbytes + off) == _lib.XH_ERR_INVALID
            assert _last_error() == "%s: %d bytes, expected %d" % (
                name, nbytes + off, nbytes)
    env.close()


# --------------------------------------------------------------------- 7 --
def test_the_last_venv_frees_a_destroyed_context():
    """xh_ctx_destroy with two venvs alive only marks the context; both venvs
    go on working on it, and each destroy succeeds -- the second one is the
    context's last owner."""
    from dependence_free_rl_amd import Context, _lib
    lib, own = _lib.lib, Context(device=0)
    a, b = _venv(own), _venv(own)
    first = a.get(_lib.VENV_BINS)
    assert lib.xh_ctx_destroy(own.h) == _lib.XH_OK
    own.h = C.c_void_p()                    # ours no longer
    assert lib.xh_venv_act(a.h, None, _lib.ACT_LOGITS, _lib.ACT_SAMPLE,
                           0) == _lib.XH_OK
    assert np.array_equal(b.get(_lib.VENV_BINS), first)  # the same seed
    assert lib.xh_venv_destroy(a.h) == _lib.XH_OK
    a.h = C.c_void_p()
    assert lib.xh_venv_act(b.h, None, _lib.ACT_LOGITS, _lib.ACT_SAMPLE,
                           0) == _lib.XH_OK
    b.synchronize()
    assert lib.xh_venv_destroy(b.h) == _lib.XH_OK
    b.h = C.c_void_p()
