"""CPU pins of tests/venv_mask_ref.py on hand-made states -- the legality rule
at its edges, eff, the word and bit order, premask -- and the premise of the
GPU episode-count case: on ActRef (tests/venv_act_ref.py), uniform rows
against premasked uniform rows at one fixed engine state."""
import numpy as np
import pytest

import venv_mask_ref as mr

f32 = np.float32


@pytest.mark.parametrize("D", [1, 2, 3])
def test_legality_rule(D):
    """bin >= item in every dimension: an exact fit is legal, one dimension
    short by 1 is not; the item's entries past D are not read."""
    item = np.array([4, 2, 3, 7], np.int8)   # entry D.. is padding
    B = 8
    bins = np.zeros((B, D), np.int8)
    bins[0] = item[:D]                       # fits exactly
    bins[1] = item[:D] + 1                   # room to spare
    bins[2] = item[:D]
    bins[2, D - 1] -= 1                      # the last dimension short by 1
    bins[3] = item[:D]
    bins[3, 0] -= 1                          # the first dimension short by 1
    bins[4] = 8                              # an empty bin
    bins[5] = -1                             # an overflowed bin
    bins[6] = 0
    bins[7] = item[:D] + np.arange(D)        # >= in every dimension
    got = mr.legal_ref(bins, item)
    assert got.dtype == bool and got.shape == (B,)
    assert got.tolist() == [True, True, False, False, True, False, False, True]
    # batched, with a [..][4] item array
    both = mr.legal_ref(np.stack([bins, bins[::-1]]), np.stack([item, item]))
    assert both.shape == (2, B)
    assert both[1].tolist() == got[::-1].tolist()


@pytest.mark.parametrize("D", [1, 2, 3])
def test_no_bin_legal_means_every_bin(D):
    item = np.full(4, 4, np.int8)
    bins = np.full((2, 8, D), 3, np.int8)    # env 0: nothing fits
    bins[1, 5] = 4                           # env 1: bin 5 fits exactly
    lg = mr.legal_ref(bins, np.stack([item, item]))
    assert not lg[0].any() and lg[1].tolist() == [False] * 5 + [True] + [False] * 2
    e = mr.eff(lg)
    assert e[0].all() and (e[1] == lg[1]).all()
    assert mr.pack(e).tolist() == [[0xff], [1 << 5]]


@pytest.mark.parametrize("B", [8, 32, 64, 128])
def test_word_and_bit_order(B):
    """W = max(1, B / 32); bit b % 32 of word b / 32 is bin b."""
    W = mr.words_per_env(B)
    assert W == {8: 1, 32: 1, 64: 2, 128: 4}[B]
    for b in sorted({0, 1, 7, 15, 16, 31, 32, 33, 63, 64, 100, 127}):
        if b >= B:
            continue
        one = np.zeros(B, bool)
        one[b] = True
        w = mr.pack(one)
        assert w.shape == (W,) and w.dtype == np.uint32
        want = [0] * W
        want[b // 32] = 1 << (b % 32)
        assert w.tolist() == want, b
    full = mr.pack(np.ones(B, bool))
    assert full.tolist() == [(1 << min(B, 32)) - 1] * W
    g = np.random.default_rng(B)
    lg = g.random((5, 3, B)) < 0.5
    assert (mr.unpack(mr.pack(lg), B) == lg).all()
    # the package's vectorised packing is the same map
    import dependence_free_rl_amd as pkg
    assert pkg.legal_words(B) == W
    assert (pkg.pack_legal(lg) == mr.pack(lg)).all()
    assert (pkg.unpack_legal(mr.pack(lg), B) == lg).all()


def test_premask():
    rows = np.array([[0.5, np.nan, 2.0, -1.0]], f32)
    keep = np.array([[True, False, True, False]])
    z = mr.premask(rows, keep, "logits")
    assert z.dtype == f32 and z[0, 0] == f32(0.5) and z[0, 2] == f32(2.0)
    assert np.isneginf(z[0, 1]) and np.isneginf(z[0, 3])
    p = mr.premask(rows, keep, "probs")
    assert p.view(np.uint32).tolist() == [[f32(0.5).view(np.uint32), 0,
                                           f32(2.0).view(np.uint32), 0]]
    assert np.isnan(rows[0, 1])              # the input is left as it was


def test_episode_count_premise():
    """The GPU episode-count case's premise on the host: B = 8, D = 2, N = 64,
    T = 48 at engine state EP_X0.  Both runs end episodes; masking ends
    strictly fewer; every end under masking had no legal bin."""
    from venv_act_ref import ActRef
    done_u, _ = mr.episode_counts(ActRef, masked=False)
    done_m, legal_m = mr.episode_counts(ActRef, masked=True)
    assert done_u.shape == (mr.EP_T, mr.EP_N)
    ends_u, ends_m = int(done_u.sum()), int(done_m.sum())
    print("ended transitions: unmasked %d, masked %d" % (ends_u, ends_m))
    assert ends_u > 0 and ends_m > 0
    assert ends_m < ends_u
    assert not legal_m[done_m == 1].any()
    # and a masked pick with a legal bin never ends the episode
    assert (done_m[legal_m.any(axis=-1)] == 0).all()
