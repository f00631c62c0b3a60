"""Pins tests/venv_heur_ref.py (the restatement the GPU tests of
xh_venv_act_heuristic compare against) to the CPU oracle's or_heuristic_eval
on the reference's instance, and asserts on the shared fixtures the conditions
that make a green GPU run mean something.  CPU only."""
import numpy as np
import pytest

from oracle import pyoracle as po
import venv_heur_ref as hr

X0 = 90210
EPISODES = {8: 6, 64: 2}


@pytest.mark.parametrize("kind", hr.KINDS)
@pytest.mark.parametrize("D", [1, 2, 3])
@pytest.mark.parametrize("B", [8, 64])
def test_the_restatement_is_the_oracles_heuristic_agent(B, D, kind):
    """One env, the default set: the per-episode lengths and the engine state
    after E episodes equal or_heuristic_eval's."""
    E = EPISODES[B]
    total, lens, x_end = po.heuristic_eval(B, D, kind, E, X0)
    ref = hr.HeurRef(B, D, 1, X0, policy_draws=2 if kind == "random" else 0)
    got, n = [], 0
    while len(got) < E:
        n += 1
        assert n < 20000
        if ref.act_heuristic(kind)["done"][0]:
            got.append(n)
            n = 0
    assert got == lens.tolist()
    assert ref.rng.state == x_end
    assert total == sum(got) - E


def test_scores_as_the_header_states_them():
    f = np.float32
    cap = (8, 8)
    bins = np.array([[4, 2], [2, 4], [8, 8], [3, 9], [6, 2], [2, 2]])
    sc = hr.scores("bestfit", bins, (2, 2), cap)
    assert sc.dtype == np.float32
    assert sc.tolist() == [1.5, 1.5, 0.5,
                           float(f(f(2) / f(3)) + f(f(2) / f(9))),
                           float(f(f(2) / f(6)) + f(1)), 2.0]
    assert hr.argmax_first(sc[:2]) == 0          # the lower bin wins the tie
    assert hr.scores("firstfit", bins, (3, 3), cap).tolist() == [
        0.0, 0.0, 1.0, 1.0, 0.0, 0.0]
    # zero entries: the term is +0, nothing is divided
    z = hr.scores("bestfit", np.array([[0, 4], [5, 1], [0, 2]]), (0, 2), (6, 4))
    assert z.tolist() == [0.5, -1.0, 1.0] and not np.signbit(z[0])
    # min-waste: exactly one dim at half the capacity, every other at zero
    mw = hr.scores("minwaste", np.array([[5, 2], [2, 5], [5, 5], [2, 2],
                                         [1, 9], [6, 3]]), (2, 2), (6, 6))
    assert mw.tolist() == [0.0, 0.0, 1.0, 1.0, -1.0, 1.0]
    mw = hr.scores("minwaste", np.array([[5, 2], [2, 4], [2, 5]]), (2, 2),
                   (6, 4))                        # a capacity per dim: 3 and 2
    assert mw.tolist() == [0.0, 0.0, 1.0]


@pytest.mark.parametrize("name", list(hr.SETUPS))
def test_fixtures_exercise_what_the_gpu_tests_rely_on(name):
    """In the restatement's own run of every setup and kind: an env ends an
    episode and a step occurs where no bin fits.  Best-fit: some maximum is
    shared by two fitting bins of different contents (which cannot happen at D
    = 1: item / b1 == item / b2 in f32 only for b1 == b2 at these sizes), and
    some maximum is no multiple of 1/8.  The three deterministic kinds pick
    different bins from one another on some state of the runs."""
    case = hr.SETUPS[name][0]
    D = case[1]
    differ = np.zeros(3, int)
    for kind in hr.KINDS:
        t = hr.trajectory(name, kind)
        assert len(t["steps"]) == hr.STEPS
        done = np.stack([s["done"] for s in t["steps"]])
        diag = {k: np.stack([s["diag"][k] for s in t["steps"]])
                for k in ("nofit", "tie", "odd", "picks")}
        assert done.any(), kind
        assert diag["nofit"].any(), kind
        # a step where nothing fits ends the episode, whatever is picked
        assert done[diag["nofit"]].all(), kind
        if kind == "bestfit":
            assert diag["tie"].any() == (D >= 2)
            assert diag["odd"].any()
        if kind != "random":
            p = diag["picks"]
            differ += [(p[..., 0] != p[..., 1]).sum(),
                       (p[..., 1] != p[..., 2]).sum(),
                       (p[..., 0] != p[..., 2]).sum()]
            i = hr.DETERMINISTIC.index(kind)
            act = np.stack([s["action"] for s in t["steps"]])
            np.testing.assert_array_equal(act, p[..., i])
            assert (np.stack([s["pchoice"] for s in t["steps"]]) == 1).all()
        else:
            B = case[0]
            pc = np.stack([s["pchoice"] for s in t["steps"]])
            assert (pc == np.float32(1.0 / B)).all()
    assert (differ > 0).all(), differ


def test_masked_random_picks_inside_the_legal_set():
    name = "K5-cap57-B8"
    t = hr.trajectory(name, "random", True)
    before = [t["first"]] + t["steps"][:-1]
    inside = [b["legal"][np.arange(len(s["action"])), s["action"]].all()
              for b, s in zip(before, t["steps"])]
    assert all(inside)
    u = hr.trajectory(name, "random")
    assert any((a["action"] != b["action"]).any()
               for a, b in zip(t["steps"], u["steps"]))


def test_set_item_set_takes_effect_from_the_next_draw():
    ref, _ = hr.make_ref("K5-cap57-B8", "firstfit")
    ref.act_heuristic("firstfit")
    held = ref.items().copy()
    ref.set_item_set([(2, 3)], [1.0])
    np.testing.assert_array_equal(ref.items(), held)
    for _ in range(3):
        ref.act_heuristic("firstfit")
    assert (ref.items() == (2, 3)).all()
