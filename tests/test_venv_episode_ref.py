"""CPU pins of tests/venv_episode_ref.py: hand-made histories with known rows
(the NaN rules, the window against the cumulative entries, restarts), and on
ActRef runs (tests/venv_act_ref.py) the lengths recovered from the done flags
against the steps counted between the oracle env's own resets -- sampling,
masked (rows premasked through tests/venv_mask_ref.py) and step."""
import numpy as np

import venv_episode_ref as er
from venv_act_ref import ActRef, mixed_rows

f32 = np.float32


def test_hand_made_history():
    """3 envs, 6 calls.  env 0 ends at calls 2 and 3 (lengths 2, 1), env 1 at
    call 5 (length 4: not live at call 1), env 2 never."""
    T, F = True, False
    live = np.array([[T, T, T], [T, F, T], [T, T, T], [T, T, T], [T, T, T],
                     [T, T, T]])
    done = np.array([[F, F, F], [T, F, F], [T, F, F], [F, F, F], [F, T, F],
                     [F, F, F]])
    rows, running, first, ref = er.rows_of_history(done, live, [0, 1, 3, 3, 6])
    nan = np.nan
    want = np.array([
        # ROW CALLS EP SUM SQ MIN MAX FIN FSUM FSQ RSUM RMAX
        [0, 0, 0, 0, 0, nan, nan, 0, 0, 0, 0, 0],
        [1, 1, 0, 0, 0, nan, nan, 0, 0, 0, 3, 1],
        [2, 2, 2, 3, 5, 1, 2, 1, 2, 4, 2 + 3, 3],
        [3, 0, 0, 0, 0, nan, nan, 1, 2, 4, 2 + 3, 3],
        [4, 3, 1, 4, 16, 4, 4, 2, 6, 20, 3 + 1 + 6, 6]], np.float64)
    assert rows.shape == (5, er.COUNT)
    assert np.array_equal(rows, want, equal_nan=True)
    assert running.tolist() == [3, 1, 6] and first.tolist() == [2, 4, -1]
    assert ref.lengths == [[2, 1], [4], []]
    assert er.lengths_from_done(done, live) == [[2, 1], [4], []]


def test_restart_and_set_state():
    ref = er.EpisodeRef(3)
    on = np.ones(3, bool)
    ref.call(on, [False, False, False])
    ref.call(on, [False, True, False])
    ref.restart([True, False, False])          # env 0's episode is abandoned
    assert ref.running.tolist() == [0, 0, 2] and ref.window == [2]
    ref.call([True, False, True], [True, False, False])
    r = ref.row()
    assert r[er.EPISODES] == 2 and r[er.LEN_SUM] == 3 and r[er.CALLS] == 3
    assert r[er.LEN_MIN] == 1 and r[er.LEN_MAX] == 2
    assert ref.first.tolist() == [1, 2, -1]
    ref.restart()
    assert ref.running.tolist() == [0, 0, 0] and ref.first.tolist() == [1, 2, -1]
    ref.set_state([5, 6, 7], [-1, -1, 9])
    ref.call(on, [True, False, False])
    r = ref.row()
    assert r[er.ROW] == 1 and r[er.LEN_SUM] == 6 and r[er.ENVS_FINISHED] == 2
    assert r[er.FIRST_LEN_SUM] == 15 and r[er.RUNNING_SUM] == 15
    assert r[er.RUNNING_MAX] == 8


def _check_against_resets(closed, done, live):
    got = er.lengths_from_done(done, live)
    assert got == closed
    assert sum(len(x) for x in got) == int(done.sum()) > 0
    return got


def test_lengths_are_the_steps_between_the_oracle_envs_resets_sampling():
    B, D, N, S = 8, 2, 12, 20
    ref = ActRef(B, D, N, 4242)
    closed = er.count_between_resets(ref)
    done, live = er.act_history(ref, mixed_rows(3, S, N, B))
    got = _check_against_resets(closed, done, live)
    assert any(len(x) >= 2 for x in got)


def test_lengths_under_masking():
    """The masked history premasks by venv_mask_ref's sets, so no episode ends
    while a bin still fits, and episodes are longer than the unmasked ones."""
    import venv_mask_ref as mr
    B, D, N, S = 8, 1, 6, 40
    uniform = np.full((S, N, B), 1.0 / B, f32)
    out = {}
    for masked in (False, True):
        ref = ActRef(B, D, N, mr.EP_X0)
        closed = er.count_between_resets(ref)
        done, live = er.act_history(ref, uniform, masked=masked)
        out[masked] = _check_against_resets(closed, done, live)
    mean = {m: np.mean([n for x in out[m] for n in x]) for m in out}
    assert mean[True] > mean[False]


def test_lengths_with_a_refused_env_and_step():
    B, D, N, S = 8, 2, 5, 16
    ref = ActRef(B, D, N, 77)
    closed = er.count_between_resets(ref)
    rows = mixed_rows(9, S, N, B)
    done, live = er.act_history(ref, rows, refuse={2: {0}, 3: {0, 4}})
    assert not live[2, 0] and not live[3, 4] and live.sum() == S * N - 3
    _check_against_resets(closed, done, live)
    ref = ActRef(B, D, N, 78)
    closed = er.count_between_resets(ref)
    actions = np.zeros((S, N), np.int32)       # always bin 0: it overflows
    actions[:, 1] = np.arange(S) % B
    done, live = er.step_history(ref, actions)
    got = _check_against_resets(closed, done, live)
    assert len(got[0]) >= 2
