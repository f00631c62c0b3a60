"""CPU checks of tests/venv_value_ref.py, the case list of the record-reading
value net's GPU tests: every window has the row counts it says, episodes end
inside it (at least one ended transition in every NEXT view), its float32
observations are record_obs's divisions, and every listed gradient case meets
its conditioning -- numpy's own float32 gradient within conftest's default
budgets of the float64 one and, up to WELL_ROWS rows, no nearly cancelling H1.
Judged on the restatements alone."""
import numpy as np
import pytest

import venv_net_ref as nr
import venv_value_ref as vr
from conftest import GRAD_UNITS_MEDIAN, GRAD_UNITS_P99, grad_units


@pytest.mark.parametrize("B,D,builtin", vr.WINDOWS)
def test_windows_have_their_rows_and_ended_transitions(B, D, builtin):
    w = vr.window(B, D, builtin)
    assert w["state"].shape == (vr.STATE_ROWS, B, 2 * D) == (144, B, 2 * D)
    assert w["next"].shape == (vr.NEXT_ROWS, B, 2 * D) == (120, B, 2 * D)
    assert w["state"].dtype == w["next"].dtype == np.float32
    done = w["record"]["done"].reshape(-1) != 0
    assert w["ended"] == int(done.sum()) >= 1
    assert w["ended"] < vr.NEXT_ROWS  # and transitions that go on
    cap = w["cap"].astype(np.float32)
    rec, (pb, pi) = w["record"], w["present"]
    # STATE: slot t's state, slot T the present one, record_obs's divisions
    bins = np.concatenate([rec["bins"], pb[None]]).reshape(-1, B, D)
    items = np.concatenate([rec["items"], pi[None]]).reshape(-1, D)
    assert np.array_equal(w["state"][:, :, :D], bins.astype(np.float32) / cap)
    assert np.array_equal(w["state"][:, :, D:],
                          np.broadcast_to((items.astype(np.float32) / cap)[:, None],
                                          (vr.STATE_ROWS, B, D)))
    # NEXT: the successor where the transition went on, the terminal view (the
    # chosen bin below zero in some dim) where it ended
    q = np.arange(vr.NEXT_ROWS)
    assert np.array_equal(w["next"][~done], w["state"][(q + vr.N)[~done]])
    act = rec["action"].reshape(-1)
    for r in np.flatnonzero(done):
        chosen = w["next"][r, act[r], :D]
        assert (chosen < 0).any()
        assert np.array_equal(w["next"][r, :, D:], w["state"][r, :, D:])
    if not builtin:
        assert not np.array_equal(w["cap"], np.full(D, 8))


def test_the_default_venv_is_among_the_windows():
    assert sum(1 for _, _, builtin in vr.WINDOWS if builtin) == 1
    assert {(B, D) for B, D, builtin in vr.WINDOWS if not builtin} == \
        {(8, 1), (8, 2), (16, 3), (64, 2), (128, 3)}


def test_every_gradient_case_is_conditioned():
    cases = vr.grad_cases()
    assert {(B, D) for B, D, _, _ in cases} == set(vr.SHAPES)
    assert {c for _, _, c, _ in cases} == {1, 9, 120}
    assert {c for _, _, c, _ in vr.grid_cases()} == {vr.STATE_ROWS}
    for B, D, count, seed in cases + vr.grid_cases():
        w = vr.window(B, D)
        p, rows, dout = vr.grad_inputs(B, D, count, seed)
        view = vr.grad_view(count)
        assert rows.size == count == dout.size
        assert len(set(rows.tolist())) == count
        assert rows.min() >= 0 and rows.max() < w[view].shape[0]
        obs = w[view][rows]
        assert vr.float32_in_budget(p, obs, dout, B, D), (B, D, count, seed)
        assert vr.conditioned(p, obs, dout, B, D), (B, D, count, seed)
        if count <= vr.WELL_ROWS:
            assert vr.well_conditioned(p, obs, B, D), (B, D, count, seed)
        g, mag = nr.gradient("value", p, obs, dout, B, D, vr.WIDTHS)
        g32, _ = nr.gradient("value", p, obs, dout, B, D, vr.WIDTHS, np.float32)
        u, _, _ = grad_units(g32, g, mag)
        assert np.median(u) <= GRAD_UNITS_MEDIAN
        assert np.percentile(u, 99) <= GRAD_UNITS_P99
        if count > 1:
            assert (dout == 0).any() and (dout != 0).any()
    # the whole NEXT view holds the window's ended rows
    assert vr.grad_view(120) == "next" and vr.NEXT_ROWS == 120


@pytest.mark.parametrize("B,D", vr.SHAPES)
def test_float32_forward_meets_the_bound(B, D):
    """Plain float32 arithmetic is within (2BD + 64 + 32 + 11) u mag of the
    float64 values on both views."""
    w = vr.window(B, D)
    p = vr.make_params(B, D, 40 + B + D)
    for view in ("state", "next"):
        want, mag = nr.forward("value", p, w[view], B, D, vr.WIDTHS)
        f32, _ = nr.forward("value", p, w[view], B, D, vr.WIDTHS, np.float32)
        assert np.all(np.abs(f32 - want) <= vr.forward_bound(B, D, mag)), view
