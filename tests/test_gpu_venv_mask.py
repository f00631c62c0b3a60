"""GPU tests of the VecEnv's invalid-action masking: xh_venv_legal, the MASK
instantiations of xh_venv_act and of the loss head (xh_venv_policy_loss_
masked), the recorded legal words and the state rules -- against tests/
venv_mask_ref.py (pinned on the CPU by tests/test_venv_mask_ref.py) and ActRef
(tests/venv_act_ref.py).  Everything asserted is bit equality.

Shapes: every B in {8, 16, 32, 64, 128} x D in {1, 2, 3} with N = 70 envs,
which fills the last wave at no shape (a wave holds 64 / max(1, B / 16)
envs); the loss cases take 4 x 70 = 280 rows, one workgroup tile and a partial
one at 8 bins, several and a partial one at 64 and 128."""
import numpy as np
import pytest

import venv_mask_ref as mr
from test_gpu_venv_loss import Dev, _bits
from venv_act_ref import ActRef, mixed_rows

pytestmark = pytest.mark.gpu

f32 = np.float32
N, X0 = 70, 4242
SHAPES = [(B, D) for B in (8, 16, 32, 64, 128) for D in (1, 2, 3)]
SHAPE_IDS = ["B%d-D%d" % s for s in SHAPES]


def _venv(ctx, B, D, n=N, x0=X0):
    from dependence_free_rl_amd import VecEnv
    return VecEnv(ctx, num_envs=n, bins=B, dims=D, rng_state=x0)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert got.tobytes() == want.tobytes(), what


def _drain(env):
    """Synchronise; True where the call reports (and clears) a refusal."""
    from dependence_free_rl_amd import XhError, _lib
    try:
        env.synchronize()
    except XhError as e:
        assert "status %d" % _lib.XH_ERR_INVALID in str(e) and "refused" in str(e)
        return True
    return False


def _random_state(g, B, D, n=N):
    """bins in [0, 8], items in [1, 5] with the padding entries at 9 (read,
    they would make every bin illegal); env 3 has no legal bin, env 5 one
    exact fit (its last bin), env 6 exact fits only."""
    bins = g.integers(0, 9, (n, B, D)).astype(np.int8)
    items = np.full((n, 4), 9, np.int8)
    items[:, :D] = g.integers(1, 6, (n, D))
    bins[3] = items[3, :D] - 1
    bins[3, :, 1:] = 8                      # short in dimension 0 only
    bins[5] = 0
    bins[5, B - 1] = items[5, :D]
    bins[6] = items[6, :D]
    return bins, items


def _state(env):
    from dependence_free_rl_amd import _lib
    return env.get(_lib.VENV_BINS), env.get(_lib.VENV_ITEMS)


# --------------------------------------------------------------------- 1 --
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_legal_against_the_reference(ctx, shape):
    """xh_venv_legal on states set through xh_venv_set equals eff(legal_ref)
    -- random fills, a row with no legal bin, exact fits -- as bools, as words,
    in the venv's buffer and in the caller's, where the words past the last
    env stay untouched; with the mask off and on."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    W = mr.words_per_env(B)
    g = np.random.default_rng(100 * B + D)
    bins, items = _random_state(g, B, D)
    env = _venv(ctx, B, D)
    assert _lib.lib.xh_venv_legal_words(env.h) == W
    env.set(_lib.VENV_BINS, bins)
    env.set(_lib.VENV_ITEMS, items)
    lg = mr.legal_ref(bins, items)
    assert not lg[3].any() and lg[5].tolist() == [False] * (B - 1) + [True]
    assert lg[6].all() and 0 < lg.sum() < lg.size
    want = mr.eff(lg)
    assert want[3].all()
    got = env.legal()
    assert got.dtype == bool and got.shape == (N, B)
    assert np.array_equal(got, want)
    _same(env.legal(packed=True), mr.pack(want), "the words")
    dev = Dev(ctx)
    guard = np.full((N + 6) * W, 0xdeadbeef, np.uint32)
    ptr = dev.put(guard)
    env.set_action_mask(True)               # the same with the mask on
    assert env.legal(out=ptr) is None
    back = dev.get(ptr, np.uint32, ((N + 6) * W,))
    _same(back[:N * W].reshape(N, W), mr.pack(want), "the caller's array")
    assert (back[N * W:] == 0xdeadbeef).all()
    # the state is as it was
    b2, i2 = _state(env)
    _same(b2, bins, "bins")
    _same(i2, items, "items")
    dev.free()
    env.close()


# --------------------------------------------------------------------- 2 --
GETS = ("VENV_ACTIONS", "VENV_PCHOICE", "VENV_REWARD", "VENV_DONE",
        "VENV_BINS", "VENV_ITEMS", "VENV_RNG", "VENV_OBS")
T_ACT = 6


@pytest.mark.parametrize("mode", ["sample", "argmax"])
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_act_is_the_unmasked_act_on_premasked_rows(ctx, shape, kind, mode):
    """Venv A masks, venv B is fed premask(rows) computed on the host from
    A's states: after every one of 6 steps of mixed_rows (envs overflow and
    reset) the eight per-env arrays are equal bit for bit, then the six record
    arrays and the distribution record; in sample mode the steps are ActRef's
    on the premasked probabilities.  Every fifth env starts with all bins
    full -- nothing fits, so its first pick ends the episode under masking too
    -- and env 1 with bin 2 full and a one-hot row on it: under probabilities
    its legal entries sum to zero and it is refused, as a zero-sum row is."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    rows = mixed_rows(7 * B + D, T_ACT, N, B)
    rows[0, 1] = 0
    rows[0, 1, 2] = 1
    if kind == "logits":
        rows = np.log(rows + f32(1e-3)).astype(f32)
    a, b = _venv(ctx, B, D), _venv(ctx, B, D)
    a.set_action_mask(True)
    bins0 = a.get(_lib.VENV_BINS)
    bins0[1, 2] = 0
    bins0[2::5] = 0
    for env in (a, b):
        env.set(_lib.VENV_BINS, bins0)
        env.set_record(T_ACT, states=True, distrib=True)
    refused, pre, masked_any = [], [], 0
    for t in range(T_ACT):
        e = mr.eff(mr.legal_ref(*_state(a)))
        masked_any += int((~e).sum())
        pm = mr.premask(rows[t], e, kind)
        pre.append(pm)
        a.act(rows[t], kind=kind, mode=mode, write_obs=True, fetch=False)
        b.act(pm, kind=kind, mode=mode, write_obs=True, fetch=False)
        ra, rb = _drain(a), _drain(b)
        assert ra == rb
        # a probability row whose legal entries sum to zero is refused
        zero = [] if kind == "logits" else np.flatnonzero(
            pm.astype(np.float64).sum(axis=1) == 0).tolist()
        assert ra == bool(zero) and (1 in zero) == (t == 0 and kind == "probs")
        refused.append(zero)
        for name in GETS:
            which = getattr(_lib, name)
            _same(a.get(which), b.get(which), "%s after step %d" % (name, t))
    assert masked_any > 0
    ra, rb = a.record(), b.record()
    assert sorted(ra) == sorted(list(rb) + ["legal"])
    for k in rb:
        _same(ra[k], rb[k], "record %s" % k)
    assert ra["done"][0, 2::5].all()        # envs overflowed and were reset
    assert (ra["bins"][1, 2::5] == 8).all()
    if mode == "sample":
        ref = ActRef(B, D, N, X0)
        ref.envs[1].bins[2] = 0
        for e in range(2, N, 5):
            ref.envs[e].bins[:] = 0
        keep = np.ones(N, bool)             # a refused env's stream stays
        for t in range(T_ACT):              # behind ActRef's from then on
            keep[refused[t]] = False
            _same(ref.bins()[keep], ra["bins"][t][keep], "ActRef bins %d" % t)
            p = pre[t] if kind == "probs" else ra["distrib"][t]
            r = ref.act(p, refuse=set(refused[t]))
            for k in ("action", "pchoice", "reward", "done"):
                _same(r[k][keep], ra[k][t][keep], "ActRef %s %d" % (k, t))
    a.close()
    b.close()


# --------------------------------------------------------------------- 3 --
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_recorded_words(ctx, shape, kind):
    """The recorded words are eff(legal_ref) of the record's own bins / items
    in every slot, a refused env's too.  A NaN in a legal entry refuses the
    env; a NaN in an illegal entry is not seen."""
    from dependence_free_rl_amd import _lib
    B, D = shape
    T, lib = 4, _lib.lib
    W = mr.words_per_env(B)
    g = np.random.default_rng(31 * B + D)
    env = _venv(ctx, B, D)
    env.set_action_mask(True)
    assert lib.xh_venv_record_legal_bytes(env.h) == 0
    assert lib.xh_venv_record_legal_ptr(env.h) is None
    env.set_record(T, states=True)
    assert lib.xh_venv_record_legal_bytes(env.h) == T * N * W * 4
    assert lib.xh_venv_record_legal_ptr(env.h)
    assert env.record()["legal"].shape == (0, N, B)
    # bins part full, so illegal bins exist from the first step on
    bins = g.integers(0, 9, (N, B, D)).astype(np.int8)
    env.set(_lib.VENV_BINS, bins)
    rows = (g.random((T, N, B)) * 4.0 + 0.25).astype(f32)
    nan_t = 1
    for t in range(T):
        r = rows[t].copy()
        if t == nan_t:
            lg = mr.legal_ref(*_state(env))
            mixed = np.flatnonzero(lg.any(axis=1) & ~lg.all(axis=1))
            assert len(mixed) >= 2
            e_ref, e_ok = int(mixed[0]), int(mixed[1])
            r[e_ref, np.flatnonzero(lg[e_ref])[-1]] = np.nan   # legal: refused
            r[e_ok, np.flatnonzero(~lg[e_ok])[0]] = np.nan     # illegal: unseen
            before = _state(env)
        env.act(r, kind=kind, fetch=False)
        assert _drain(env) == (t == nan_t)
        if t == nan_t:
            after = _state(env)
            _same(after[0][e_ref], before[0][e_ref], "the refused env's bins")
            assert not np.array_equal(after[0][e_ok], before[0][e_ok]) or \
                not np.array_equal(after[1][e_ok], before[1][e_ok])
    rec = env.record()
    want = mr.eff(mr.legal_ref(rec["bins"], rec["items"]))
    assert want.shape == (T, N, B) and not want.all()
    assert np.array_equal(rec["legal"], want)
    raw = np.zeros((T, N, W), np.uint32)
    _lib.check(lib.xh_venv_get_record_legal(env.h, raw.ctypes.data, raw.nbytes))
    _same(raw, mr.pack(want), "the words")
    assert lib.xh_venv_get_record_legal(env.h, raw.ctypes.data,
                                        raw.nbytes - 4) == _lib.XH_ERR_INVALID
    assert rec["pchoice"][nan_t, e_ref] == 0 and rec["done"][nan_t, e_ref] == 0
    assert rec["pchoice"][nan_t, e_ok] > 0
    assert want[nan_t, e_ok, rec["action"][nan_t, e_ok]]
    # every pick of an env that acted is in its set
    tt, ee = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    acted = rec["pchoice"] > 0
    assert acted.sum() == T * N - 1
    assert want[tt, ee, rec["action"]][acted].all()
    # rewind keeps the block, a new record brings a new zero-filled one
    env.rewind()
    assert lib.xh_venv_record_legal_bytes(env.h) == T * N * W * 4
    env.set_record(2, states=False)
    assert lib.xh_venv_record_legal_bytes(env.h) == 2 * N * W * 4
    raw2 = np.ones((2, N, W), np.uint32)
    _lib.check(lib.xh_venv_get_record_legal(env.h, raw2.ctypes.data,
                                            raw2.nbytes))
    assert not raw2.any()
    env.set_record(0)
    assert lib.xh_venv_record_legal_bytes(env.h) == 0
    env.close()


# --------------------------------------------------------------------- 4 --
def test_masking_ends_fewer_episodes(ctx):
    """The case tests/test_venv_mask_ref.py pinned on the host, on the
    device: uniform rows, B = 8, D = 2, N = 64, T = 48.  Masked ends are fewer
    than unmasked ends, and done under masking implies an empty legal_ref row;
    both runs are the host's, bit for bit."""
    out = {}
    uniform = np.full((mr.EP_N, mr.EP_B), 1.0 / mr.EP_B, f32)
    for masked in (False, True):
        env = _venv(ctx, mr.EP_B, mr.EP_D, n=mr.EP_N, x0=mr.EP_X0)
        env.set_action_mask(masked)
        env.set_record(mr.EP_T, states=True)
        for _ in range(mr.EP_T):
            env.act(uniform, kind="probs", fetch=False)
        env.synchronize()
        out[masked] = env.record()
        env.close()
    ends_u, ends_m = int(out[False]["done"].sum()), int(out[True]["done"].sum())
    print("ended transitions: unmasked %d, masked %d" % (ends_u, ends_m))
    assert 0 < ends_m < ends_u
    rec = out[True]
    lg = mr.legal_ref(rec["bins"], rec["items"])
    assert not lg[rec["done"] == 1].any()
    assert np.array_equal(rec["legal"], mr.eff(lg))
    for masked in (False, True):
        done, _ = mr.episode_counts(ActRef, masked)
        _same(out[masked]["done"], done, "the host's run (masked=%s)" % masked)


# --------------------------------------------------------------------- 5 --
T_LOSS = 4


def _recorded(ctx, B, D, kind, seed):
    """A masked venv with T_LOSS recorded steps (states, distributions) from
    part-full bins, and its record."""
    from dependence_free_rl_amd import _lib
    g = np.random.default_rng(seed)
    env = _venv(ctx, B, D)
    env.set_action_mask(True)
    env.set_record(T_LOSS, states=True, distrib=True)
    env.set(_lib.VENV_BINS, g.integers(0, 9, (N, B, D)).astype(np.int8))
    rows = _rows(g, kind, (T_LOSS, N, B))
    for t in range(T_LOSS):
        env.act(rows[t], kind=kind, fetch=False)
    env.synchronize()
    return env, env.record(), rows, g


def _rows(g, kind, shape):
    if kind == "logits":
        return (g.standard_normal(shape) * 3.0).astype(f32)
    return (g.random(shape) * 5.0 + 1e-3).astype(f32)


def _same_outputs(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        if want[k].dtype == f32:
            _bits(got[k], want[k], "%s: %s" % (what, k))
        else:
            _same(got[k], want[k], "%s: %s" % (what, k))


@pytest.mark.parametrize("loss", ["clipped", "log", "kl"])
@pytest.mark.parametrize("kind", ["logits", "probs"])
@pytest.mark.parametrize("B", [8, 64, 128])
def test_loss_is_the_unmasked_loss_on_premasked_rows(ctx, B, kind, loss):
    """policy_loss(legal=True) on a shuffled minibatch with a partial last
    tile equals policy_loss on the premasked minibatch in grad, probs, dvalue,
    stats and kl_stats; so do the caller's-array forms (host bools, host
    words, a device pointer), where an all-zero row is an unmasked row."""
    D = 2
    env, rec, _, g = _recorded(ctx, B, D, kind, 1000 + B)
    total = T_LOSS * N
    eff = rec["legal"].reshape(total, B)
    assert not eff.all() and eff.any(axis=1).all()
    idx = g.permutation(total).astype(np.int32)
    count = total - 3                        # a partial last tile
    policy = _rows(g, kind, (count, B))
    adv = g.standard_normal(total).astype(f32)
    target = g.standard_normal(total).astype(f32)
    values = g.standard_normal(count).astype(f32)
    kw = dict(kind=kind, loss=loss, rows=idx, count=count, values=values,
              target=target, want_probs=True, want_stats=True, want_kl=True,
              beta=0.05, scale=0.5, value_scale=0.25)
    pm = mr.premask(policy, eff[idx[:count]], kind)
    assert not np.array_equal(pm, policy, equal_nan=True)
    want = env.policy_loss(pm, adv, **kw)
    got = env.policy_loss(policy, adv, legal=True, **kw)
    _same_outputs(got, want, "the record's words")
    assert got["stats"][0] == count          # XH_VLOSS_ROWS
    plain = env.policy_loss(policy, adv, **kw)
    # (under probs + clipped the gradient reads the chosen entry alone)
    assert not np.array_equal(plain["probs"], got["probs"], equal_nan=True)
    assert (got["probs"][~eff[idx[:count]]] == 0).all()

    # the caller's arrays: the record's rows handed over as the caller's own
    own = dict(kw, action=rec["action"].reshape(-1),
               p_old=rec["pchoice"].reshape(-1),
               distrib=rec["distrib"].reshape(total, B))
    cut = eff.copy()
    zero = idx[:count:7]
    cut[zero] = False                        # all-zero words: unmasked rows
    eff2 = eff.copy()
    eff2[zero] = True
    want2 = env.policy_loss(mr.premask(policy, eff2[idx[:count]], kind), adv,
                            **own)
    dev = Dev(ctx)
    forms = {"host bools": cut, "host words": mr.pack(cut),
             "a device pointer": dev.put(mr.pack(cut))}
    for what, legal in forms.items():
        _same_outputs(env.policy_loss(policy, adv, legal=legal, **own), want2,
                      what)
    none = env.policy_loss(policy, adv, legal=np.zeros((total, B), bool), **own)
    _same_outputs(none, env.policy_loss(policy, adv, **own), "all rows zero")
    dev.free()
    env.close()


# --------------------------------------------------------------------- 6 --
@pytest.mark.parametrize("B", [8, 32, 64, 128])
def test_epoch_zero_under_masking(ctx, B):
    """The recorded logits fed straight back: p[choice] has PCHOICE's bits, so
    every ratio is exactly 1.0f; CLIPPED, LOGR_SUM, LOGR_SQSUM and K3_SUM are
    exactly 0, KL(q || p) is exactly 0, and the gradient is 0 at masked
    bins."""
    from dependence_free_rl_amd import _lib
    env, rec, rows, g = _recorded(ctx, B, 2, "logits", 2000 + B)
    total = T_LOSS * N
    eff = rec["legal"].reshape(total, B)
    adv = g.standard_normal(total).astype(f32)
    for loss in ("clipped", "kl"):
        out = env.policy_loss(rows.reshape(total, B), adv, kind="logits",
                              loss=loss, legal=True, want_probs=True,
                              want_stats=True, want_kl=True, beta=0.05)
        p_ch = out["probs"][np.arange(total), rec["action"].reshape(-1)]
        _bits(p_ch, rec["pchoice"].reshape(-1), "p[choice] is PCHOICE")
        ratio = p_ch / rec["pchoice"].reshape(-1)
        assert ratio.dtype == f32 and (ratio == f32(1.0)).all()
        _bits(out["probs"], rec["distrib"].reshape(total, B), "p is q")
        st, kl = out["stats"], out["kl_stats"]
        assert st[_lib.VLOSS_ROWS] == total and st[_lib.VLOSS_SKIPPED] == 0
        for k in (_lib.VLOSS_CLIPPED, _lib.VLOSS_LOGR_SUM,
                  _lib.VLOSS_LOGR_SQSUM, _lib.VLOSS_K3_SUM):
            assert st[k] == 0.0, k
        assert kl[_lib.VKL_ROWS] == total and kl[_lib.VKL_KL_SUM] == 0.0
        assert kl[_lib.VKL_KL_SQSUM] == 0.0
        assert not eff.all() and (out["grad"][~eff] == 0).all()
        assert np.isfinite(out["grad"]).all() and out["grad"][eff].any()
    env.close()


# --------------------------------------------------------------------- 7 --
def test_state_rules(ctx):
    """set_action_mask at a non-zero cursor is XH_ERR_STATE; legal=True
    without a block is XH_ERR_STATE; turning the mask off restores the
    unmasked bits and record() loses its "legal" key."""
    from dependence_free_rl_amd import XhError, _lib
    B, D = 32, 2
    lib = _lib.lib
    g = np.random.default_rng(5)
    bins = g.integers(0, 9, (N, B, D)).astype(np.int8)
    rows = (g.random((2, N, B)) + 0.05).astype(f32)
    env = _venv(ctx, B, D)
    env.set(_lib.VENV_BINS, bins)
    env.set_record(3, states=True)
    assert "legal" not in env.record()
    env.act(rows[0], fetch=False)
    assert lib.xh_venv_set_action_mask(env.h, 1) == _lib.XH_ERR_STATE
    assert b"cursor" in lib.xh_last_error()
    assert lib.xh_venv_record_legal_bytes(env.h) == 0
    adv = np.ones(N, f32)
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_STATE):
        env.policy_loss(rows[0], adv, kind="probs", legal=True)
    env.rewind()
    env.set_action_mask(True)
    env.set_action_mask(True)                # on already: nothing done
    assert "legal" in env.record()
    env.act(rows[0], fetch=False)
    env.policy_loss(rows[0], adv, kind="probs", legal=True)
    # the record's words go with the record's rows
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_INVALID):
        env.policy_loss(rows[0], adv, kind="probs", legal=True,
                        action=np.zeros(N, np.int32), p_old=np.ones(N, f32))
    env.set_action_mask(False)               # off at any cursor
    assert lib.xh_venv_record_legal_bytes(env.h) == 0
    assert "legal" not in env.record()
    with pytest.raises(XhError, match="status %d" % _lib.XH_ERR_STATE):
        env.policy_loss(rows[0], adv, kind="probs", legal=True)
    # one act call with the mask off again against a fresh unmasked venv
    fresh = _venv(ctx, B, D)
    for e in (env, fresh):
        e.set(_lib.VENV_BINS, bins)
        e.set(_lib.VENV_ITEMS, fresh.get(_lib.VENV_ITEMS))
        e.set(_lib.VENV_RNG, fresh.get(_lib.VENV_RNG))
        e.set_record(1, states=True)
    got = env.act(rows[1], write_obs=True)
    want = fresh.act(rows[1], write_obs=True)
    for x, y in zip(got, want):
        _same(x, y, "act with the mask off again")
    for name in GETS:
        _same(env.get(getattr(_lib, name)), fresh.get(getattr(_lib, name)),
              name)
    ra, rb = env.record(), fresh.record()
    assert sorted(ra) == sorted(rb) and "legal" not in ra
    for k in rb:
        _same(ra[k], rb[k], "record %s" % k)
    # and the unmasked pick does leave the legal sets here
    lg = mr.legal_ref(ra["bins"][0], ra["items"][0])
    assert not lg[np.arange(N), ra["action"][0]].all()
    env.close()
    fresh.close()
