"""Trainer-state checkpoints on the device (xh_trainer_save_state / load_state /
state_digest; Trainer.state / set_state / state_digest): a run that is saved,
destroyed, restored into a differently initialised trainer and continued
produces the bits of the run that was never interrupted.  Every comparison is
bitwise -- rollout() and learn() form every sum in a fixed order -- so there is
no tolerance here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = M = 2  # iterations before the save / after the restore


def _case(name):
    """Trainer arguments, optimizers of the saved run, optimizers the
    restoring trainer starts with (None: the config's sgd)."""
    return {
        # the f32 kernels; adam's moments and step counter on both nets
        "ppo_b8": (dict(algo="ppo", bins=8, dims=2, num_envs=16, steps=4,
                        widths=(128, 64)),
                   {0: ("adam", 1e-3), 1: ("adam", 1e-3)},
                   {0: ("adam", 3e-3), 1: ("adam", 3e-3)}),
        # the wave-specialised train kernel, PPO's epoch-0 reuse, the bf16
        # value net's W0 fragments; the restore allocates the velocity
        "ppo_b64": (dict(algo="ppo", bins=64, dims=2, num_envs=128, steps=4,
                         widths=(128, 128), epochs=4),
                    {1: ("momentum", 1e-5)}, None),
        # carries beta; the restore takes the policy back from adam to sgd
        "klppo_b32": (dict(algo="klppo", bins=32, dims=1, num_envs=64, steps=4,
                           widths=(64, 64)),
                      None, {0: ("adam", 1e-3)}),
        "ac_b128": (dict(algo="ac", bins=128, dims=3, num_envs=32, steps=4,
                         widths=(128, 128)), None, None),
        # REINFORCE: one whole episode per env and iteration
        "pg_b8": (dict(algo="pg", bins=8, dims=1, num_envs=8, steps=1,
                       widths=(64, 32)), None, None),
    }[name]


def _make(ctx, kw, opts, rng_state, seed, **extra):
    from dependence_free_rl_amd import (POLICY, VALUE, Trainer, init_full_policy,
                                        init_policy, init_value)
    tr = Trainer(ctx, rng_state=rng_state, **dict(kw, **extra))
    B, D = kw["bins"], kw["dims"]
    if kw["algo"] == "pg":
        tr.set_params(POLICY, init_full_policy(B, D, kw["widths"], seed=seed))
    else:
        tr.set_params(POLICY, init_policy(D, *kw["widths"], seed=seed))
        tr.set_params(VALUE, init_value(B, D, seed=seed + 1))
    for which, (kind, lr) in (opts or {}).items():
        tr.set_optimizer(which, kind, lr)
    return tr


def _iterate(tr, n):
    for _ in range(n):
        tr.rollout()
        tr.learn()


def _snapshot(tr):
    """What a continued run has to reproduce, after its last learn()."""
    from dependence_free_rl_amd import POLICY, VALUE
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_ADV, BUF_DONE,
                                                BUF_KL, BUF_LEN, BUF_POLD,
                                                BUF_POLICY_GRADS, BUF_RNG)
    pg = tr.cfg.algo == 3
    out = {"policy": tr.params(POLICY), "rng": tr.buffer(BUF_RNG),
           "grads": tr.buffer(BUF_POLICY_GRADS), "digest": tr.state_digest()}
    k = tr.kernel_info()
    out["kernels"] = (k["rollout_step"]["kernel"], k["policy_train"]["kernel"],
                      k["value"])
    # REINFORCE's grids are [Tmax][N]: env e wrote its first len[e] steps
    mask = (np.arange(tr.T)[:, None] < tr.buffer(BUF_LEN)[None, :]) if pg else None
    for name, b in (("action", BUF_ACTION), ("pold", BUF_POLD),
                    ("done", BUF_DONE), ("adv", BUF_ADV)):
        a = tr.buffer(b)
        out[name] = a[mask] if pg else a
    if not pg:
        out["value"] = tr.params(VALUE)
        out["env_bins"], out["env_items"] = tr.env_state()
    if tr.cfg.algo == 2:
        out["kl"] = tr.buffer(BUF_KL)
    return out


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert got[k].dtype == want[k].dtype, k
            # bit patterns, so that a NaN or a signed zero counts as a value
            np.testing.assert_array_equal(got[k].view(np.uint8),
                                          want[k].view(np.uint8), err_msg=k)
        else:
            assert got[k] == want[k], k


@pytest.mark.parametrize("name", ["ppo_b8", "ppo_b64", "klppo_b32", "ac_b128",
                                  "pg_b8"])
def test_resumed_run_equals_the_uninterrupted_one(ctx, name):
    kw, opts, other_opts = _case(name)
    a = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(a, K + M)
    want = _snapshot(a)
    a.close()

    b = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(b, K)
    blob = b.state()
    b.close()

    # another run: its own streams, parameters, optimizer state, W0 fragments,
    # epoch-0 records and a pending forget() shift, all of which must go
    c = _make(ctx, kw, other_opts, rng_state=977, seed=70)
    _iterate(c, 1)
    c.set_state(blob)
    _iterate(c, M)
    got = _snapshot(c)
    c.close()
    _assert_same(got, want)
    assert want["digest"]["policy_params"] != 0
    if name == "klppo_b32":
        assert want["digest"]["kl_beta"] != 0
        assert want["digest"]["policy_opt_m"] == 0  # back on sgd
    if name == "ppo_b64":
        assert want["digest"]["value_opt_m"] != 0
        assert want["kernels"][1] == "policy_train_spec8_kernel"


def test_statistics_continue(ctx):
    """The episode-length columns of the rows after a restore agree with the
    uninterrupted run's only if the running lengths were restored."""
    from dependence_free_rl_amd import STAT_EPISODES, STAT_EPLEN_SUM, STAT_ITER
    kw, opts, other_opts = _case("ppo_b8")

    def make(rng_state, seed, o):
        tr = _make(ctx, kw, o, rng_state, seed)
        tr.set_stats(16)
        return tr

    a = make(4242, 7, opts)
    _iterate(a, K + M)
    want = a.stats()[-M:]
    a.close()
    b = make(4242, 7, opts)
    _iterate(b, K)
    blob = b.state()
    b.close()
    c = make(977, 70, other_opts)
    _iterate(c, 1)
    c.set_state(blob)
    _iterate(c, M)
    got = c.stats()[-M:]
    c.close()
    cols = [k for k in range(want.shape[1]) if k != STAT_ITER]
    np.testing.assert_array_equal(got[:, cols].view(np.uint64),
                                  want[:, cols].view(np.uint64))
    np.testing.assert_array_equal(want[:, STAT_ITER], [K, K + 1])
    np.testing.assert_array_equal(got[:, STAT_ITER], [1, 2])
    # episodes that began before the save ended after it: lengths beyond what
    # the M windows alone could have counted would be the tell
    assert want[:, STAT_EPISODES].sum() > 0
    assert want[:, STAT_EPLEN_SUM].sum() > 0


def test_global_checkpoint_restores_into_shards(ctx):
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_BINS, BUF_DONE,
                                                BUF_ITEMS, BUF_POLD, BUF_RNG)
    kw, opts, _ = _case("ppo_b8")
    g = _make(ctx, kw, opts, rng_state=4242, seed=7, num_envs=32)
    _iterate(g, 1)
    blob = g.state()
    g.rollout()
    bufs = (BUF_ACTION, BUF_POLD, BUF_DONE, BUF_BINS, BUF_ITEMS)
    want = {b: g.buffer(b) for b in bufs}
    want_rng = g.buffer(BUF_RNG)
    g.close()
    for off in (0, 16):
        s = _make(ctx, kw, None, rng_state=31 + off, seed=90, num_envs=16,
                  num_envs_global=32, env_offset=off)
        s.set_state(blob)
        s.rollout()
        for b in bufs:
            np.testing.assert_array_equal(s.buffer(b), want[b][:, off:off + 16],
                                          err_msg="buffer %d, envs from %d" % (b, off))
        np.testing.assert_array_equal(s.buffer(BUF_RNG), want_rng[off:off + 16])
        s.close()


def test_nets_only_leaves_envs_and_streams(ctx):
    from dependence_free_rl_amd.trainer import BUF_RNG
    kw, opts, _ = _case("ppo_b8")
    src = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(src, 2)
    blob, want = src.state(), src.state_digest()
    src.close()
    dst = _make(ctx, kw, None, rng_state=55, seed=33, num_envs=32, steps=8)
    _iterate(dst, 1)
    bins, items = dst.env_state()
    rng, before = dst.buffer(BUF_RNG), dst.state_digest()
    with pytest.raises(Exception, match="status 1.*steps"):
        dst.set_state(blob)  # a whole state needs the same steps
    dst.set_state(blob, nets_only=True)
    got = dst.state_digest()
    for k in ("policy_params", "value_params", "policy_opt_m", "policy_opt_v",
              "value_opt_m", "value_opt_v"):
        assert got[k] == want[k] != 0, k
    for k in ("env_bins", "env_items", "rng"):
        assert got[k] == before[k], k
    b2, i2 = dst.env_state()
    np.testing.assert_array_equal(b2, bins)
    np.testing.assert_array_equal(i2, items)
    np.testing.assert_array_equal(dst.buffer(BUF_RNG), rng)
    _iterate(dst, 1)  # adam continues from the restored moments and t
    assert np.isfinite(dst.params(0)).all()
    dst.close()


def test_overflowed_start_state_keeps_the_f32_rollout(ctx):
    """A restored bin below -capacity sends the next rollout step to the f32
    kernel, as the same state set by hand does (T = 1: the one step reported
    is the one that reads it)."""
    from dependence_free_rl_amd.trainer import (BUF_ACTION, BUF_BINS, BUF_DONE,
                                                BUF_POLD, BUF_RNG)
    kw = dict(algo="ppo", bins=64, dims=2, num_envs=16, steps=1, widths=(128, 128))
    x = _make(ctx, kw, None, rng_state=4242, seed=7)
    bins, items = x.env_state(3, 1)
    bins[0, 5, 1] = -12
    x.set_env_state(3, bins, items)
    blob = x.state()
    y = _make(ctx, kw, None, rng_state=977, seed=70)
    y.set_state(blob)
    for tr in (x, y):
        tr.rollout()
    kx, ky = (tr.kernel_info()["rollout_step"] for tr in (x, y))
    assert kx["kernel"] == ky["kernel"] and kx["math"] == ky["math"] == "f32_mfma"
    for b in (BUF_ACTION, BUF_POLD, BUF_DONE, BUF_BINS, BUF_RNG):
        np.testing.assert_array_equal(x.buffer(b), y.buffer(b), err_msg=str(b))
    assert (y.buffer(BUF_BINS)[0] == -12).sum() == 1
    x.close()
    y.close()


def test_pending_overrides_are_part_of_the_state(ctx):
    kw, opts, _ = _case("ppo_b8")
    x = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(x, 1)
    bins, items = x.env_state()
    nb = np.full((2,) + bins.shape[1:], 3, np.int8)
    ni = np.array([[4, 2], [1, 2]], np.int8)
    x.set_env_state(5, nb[:1], ni[:1])
    x.set_env_state(11, nb[1:], ni[1:])
    with pytest.raises(Exception, match="status 4"):
        x.state_digest()  # the device does not hold them yet
    blob = x.state()
    y = _make(ctx, kw, None, rng_state=977, seed=70)
    y.set_state(blob)
    b2, i2 = y.env_state()
    bins[5], bins[11], items[5], items[11] = nb[0], nb[1], ni[0], ni[1]
    np.testing.assert_array_equal(b2, bins)
    np.testing.assert_array_equal(i2, items)
    np.testing.assert_array_equal(x.env_state()[0], bins)
    x.close()
    y.close()


def test_refused_calls_change_nothing(ctx):
    kw, opts, _ = _case("ppo_b8")
    tr = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(tr, 1)
    good = tr.state()
    tr.rollout()
    before = tr.state_digest()
    with pytest.raises(Exception, match="status 4"):
        tr.state()  # between rollout() and learn()
    with pytest.raises(Exception, match="status 4"):
        tr.set_state(good)
    assert tr.state_digest() == before
    tr.learn()
    before = tr.state_digest()

    other = _make(ctx, dict(kw, steps=8), opts, rng_state=4242, seed=7)
    shard = _make(ctx, kw, opts, rng_state=4242, seed=7, num_envs=8,
                  num_envs_global=16, env_offset=8)
    refused = {
        "steps": other.state(),            # another shape: the field is named
        "envs": shard.state(),             # a slice that does not cover ours
        "truncated": good[:-16],
        "corrupted": good[:-1] + bytes([good[-1] ^ 0x40]),
        "flipped parameter": good[:1000] + bytes([good[1000] ^ 1]) + good[1001:],
    }
    other.close()
    shard.close()
    for why, blob in refused.items():
        with pytest.raises(Exception, match="status 1") as e:
            tr.set_state(blob)
        if why in ("steps", "envs"):
            assert why in str(e.value), str(e.value)
        assert tr.state_digest() == before, why
    tr.set_state(good)  # and the good one still loads
    assert tr.state_digest() != before
    tr.close()


def test_device_digest_equals_the_host_digest_of_each_buffer(ctx):
    from dependence_free_rl_amd import POLICY, VALUE, describe_state, digest
    from dependence_free_rl_amd.trainer import BUF_BINS, BUF_ITEMS, BUF_RNG
    kw, _, _ = _case("ppo_b8")
    tr = _make(ctx, kw, None, rng_state=4242, seed=7)

    def check(slot, moments):
        d = tr.state_digest()
        assert d["policy_params"] == digest(tr.params(POLICY))
        assert d["value_params"] == digest(tr.params(VALUE))
        assert d["env_bins"] == digest(tr.buffer(BUF_BINS)[slot])
        assert d["env_bins"] == digest(tr.env_state()[0])
        assert d["env_items"] == digest(tr.buffer(BUF_ITEMS)[slot])
        assert d["rng"] == digest(tr.buffer(BUF_RNG))
        assert d["kl_beta"] == 0
        # the moments have no accessor of their own: the blob's section
        # digests are xh_digest_host of the downloaded arrays
        sec = {s["name"]: int(s["digest"], 16)
               for s in describe_state(tr.state())["sections"]}
        for k in ("policy_opt_m", "policy_opt_v", "value_opt_m", "value_opt_v"):
            assert (d[k] != 0) == moments, k
            assert d[k] == sec.get(k, 0), k
        for k in ("policy_params", "value_params", "env_bins", "env_items", "rng"):
            assert d[k] == sec[k], k

    check(0, False)  # fresh, sgd
    tr.set_optimizer(POLICY, "adam", 1e-3)
    tr.set_optimizer(VALUE, "adam", 1e-3)
    _iterate(tr, 2)
    check(tr.T, True)  # the next rollout starts from slot T
    tr.close()


def test_state_file_round_trip(ctx, tmp_path):
    kw, opts, _ = _case("ppo_b8")
    tr = _make(ctx, kw, opts, rng_state=4242, seed=7)
    _iterate(tr, 1)
    path = tmp_path / "run.state"
    tr.save_state(str(path))
    assert path.read_bytes() == tr.state()
    assert [p.name for p in tmp_path.iterdir()] == ["run.state"]
    want = tr.state_digest()
    _iterate(tr, 1)
    tr.load_state(str(path))
    assert tr.state_digest() == want
    tr.close()
