#!/usr/bin/env python3
"""A complete PPO on a VecEnv with its own item set, torch-free: the policy and
the value net are the library's device-resident nets (PolicyNet / ValueNet),
and every stage between them is a launch of the venv chain.

    python examples/venv_ppo.py
    python examples/venv_ppo.py --bins 16 --envs 2048 --iterations 60
    python examples/venv_ppo.py --table
    python examples/venv_ppo.py --table --value-record

Per iteration: T masked act() steps from PolicyNet.forward(venv) with the
record on; record_obs of the window; ValueNet.forward; advantages (GAE and TD
targets); `--epochs` passes over shuffled minibatches of record_obs ->
forward -> policy_loss(clipped, legal, ent_coef, value head) -> backward
(accumulating over the epoch's minibatches) and one clipped step per net;
episode_row().  Every `--eval-every` iterations the current policy plays a
fresh VecEnv greedily until every env has finished its first episode (one
episode per env: the unbiased sample), and that first-episode return is
printed beside heuristic_baseline(...) of the same item set.

--table (opt-in) runs the policy on its logit table instead of on per-bin
rows: a per-bin logit depends on (bin state, item) alone, E = K * prod(capacity
+ 1) = 308 points for this set, so PolicyNet.forward(table_obs) once per
iteration and once per epoch replaces every per-row forward; the rollout is
act_table(), the minibatches are table_logits -> policy_loss -> table_grad
(accumulating), and one PolicyNet.backward(table_obs, G) per step gives the
epoch's parameter gradient.  The value net sees whole observations and keeps
its path.

--value-record (opt-in) runs the value net straight on the record:
ValueNet.forward_record / backward_record read the int8 states of the window's
rows themselves, so the window's values and every minibatch's value forward and
backward need no record_obs.  Without --table the policy's minibatches still
form their observations; with --table no f32 observation is formed at all."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITEMS = [[5, 1], [2, 3], [3, 3], [1, 1]]
WEIGHTS = [0.3, 0.3, 0.2, 0.2]
CAPACITY = [10, 6]


def evaluate(ctx, pol, a, seed):
    """First-episode return of the greedy policy: mean over one episode per
    env of a fresh venv."""
    from dependence_free_rl_amd import VENV_POLICY, VEP_ENVS_FINISHED, VecEnv
    env = VecEnv(ctx, a.eval_envs, bins=a.bins, dims=2, rng_state=seed,
                 policy_draws=0, items=ITEMS, weights=WEIGHTS,
                 capacity=CAPACITY)
    try:
        env.set_action_mask(True)
        env.set_episode_stats(2)
        env.observe()
        steps = 0
        while steps < a.eval_max_steps:
            for _ in range(32):
                pol.forward(env, out=env.device_ptr(VENV_POLICY))
                env.act(None, kind="logits", mode="argmax", write_obs=True,
                        fetch=False)
            steps += 32
            env.episode_row()
            if env.episode_stats(count=1)[0][VEP_ENVS_FINISHED] == a.eval_envs:
                break
        first = env.first_episode_lengths()
        return float(first.mean()) - 1.0 if first.size else float("nan"), \
            int(first.size)
    finally:
        env.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--minibatch", type=int, default=4096)
    ap.add_argument("--widths", type=int, nargs=2, default=[64, 64])
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--ent-coef", type=float, default=0.01)
    ap.add_argument("--max-norm", type=float, default=0.5)
    ap.add_argument("--eval-every", type=int, default=10)
    ap.add_argument("--eval-envs", type=int, default=512)
    ap.add_argument("--eval-max-steps", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--table", action="store_true",
                    help="act and train the policy on its logit table")
    ap.add_argument("--value-record", action="store_true",
                    help="run the value net straight on the recorded window")
    a = ap.parse_args()

    from dependence_free_rl_amd import (VENV_POLICY, VLOSS_CLIPPED,
                                        VLOSS_ENTROPY_SUM, VLOSS_K3_SUM,
                                        VLOSS_ROWS, Context, PolicyNet,
                                        ValueNet, VecEnv, heuristic_baseline)
    ctx = Context(device=0)
    B, D, N, T = a.bins, 2, a.envs, a.steps
    for kind in ("random", "firstfit", "bestfit", "minwaste"):
        h = heuristic_baseline(ctx, kind, B, D, a.eval_envs, items=ITEMS,
                               weights=WEIGHTS, capacity=CAPACITY, rng_state=5)
        print("baseline %-9s first-episode return %.2f (%d episodes)"
              % (kind, h["return_mean"], h["episodes"]), flush=True)

    venv = VecEnv(ctx, N, bins=B, dims=D, rng_state=a.seed, items=ITEMS,
                  weights=WEIGHTS, capacity=CAPACITY)
    pol, val = PolicyNet(ctx, B, D, tuple(a.widths)), ValueNet(ctx, B, D)
    pol.init(a.seed)
    val.init(a.seed + 1)
    pol.set_optimizer("adam", a.lr)
    val.set_optimizer("adam", a.lr)
    venv.set_record(T)
    venv.set_action_mask(True)
    venv.set_episode_stats(a.iterations)
    venv.observe()
    rng = np.random.default_rng(a.seed)
    total = T * N
    if a.table:
        info = venv.table_info()
        tobs = venv.table_obs()  # [R][B][2D], fixed while the set is
        print("logit table: %d entries, %d rows of %d bins"
              % (info["entries"], info["rows"], B), flush=True)
    for it in range(a.iterations):
        venv.rewind()
        if a.table:
            table = pol.forward(tobs)  # once per iteration
            for _ in range(T):  # the value net reads the record: no OBS
                venv.act_table(table)
        for _ in range(0 if a.table else T):
            pol.forward(venv, out=venv.device_ptr(VENV_POLICY))
            venv.act(None, kind="logits", write_obs=True, fetch=False)
        if a.value_record:
            values = val.forward_record(venv, "state").reshape(T + 1, N)
        else:
            states = venv.record_obs("state")  # [(T + 1) N][B][2D]
            values = val.forward(states).reshape(T + 1, N)
        adv = venv.advantages(values, normalize=True,
                              returns=("adv", "td_target"))
        for epoch in range(a.epochs):
            perm = rng.permutation(total).astype(np.int32)
            if a.table:
                table = pol.forward(tobs)  # once per epoch
            for first in range(0, total, a.minibatch):
                count = min(a.minibatch, total - first)
                at = dict(rows=perm, first=first, count=count)
                if not (a.table and a.value_record):  # somebody reads them
                    obs = venv.record_obs("state", **at)
                logits = venv.table_logits(
                    table, **at) if a.table else pol.forward(obs)
                v_mb = val.forward_record(venv, "state", **at) \
                    if a.value_record else val.forward(obs)
                res = venv.policy_loss(
                    logits, adv["adv"], kind="logits",
                    loss="clipped", rows=perm, first=first, count=count,
                    scale=1.0 / total, legal=True, ent_coef=a.ent_coef,
                    values=v_mb, target=adv["td_target"],
                    value_scale=1.0 / total, want_stats=True,
                    accumulate=first > 0)
                if a.table:
                    G = venv.table_grad(res["grad"], rows=perm, first=first,
                                        count=count, accumulate=first > 0)
                else:
                    pol.backward(obs, res["grad"], accumulate=first > 0)
                if a.value_record:
                    val.backward_record(venv, res["dvalue"], "state",
                                        accumulate=first > 0, **at)
                else:
                    val.backward(obs, res["dvalue"], accumulate=first > 0)
            if a.table:  # the epoch's gradient: one backward on the table
                pol.backward(tobs, G.reshape(info["rows"], B))
            pol.step(max_norm=a.max_norm)
            val.step(max_norm=a.max_norm)
        venv.episode_row()
        s = res["stats"]
        c = venv.episode_curve()
        line = ("iter %3d  window return %.2f (%d episodes)  entropy %.3f  "
                "k3 %.2e  clipped %.3f" % (
                    it, c["return_mean"][-1], int(c["episodes"][-1]),
                    s[VLOSS_ENTROPY_SUM] / s[VLOSS_ROWS],
                    s[VLOSS_K3_SUM] / s[VLOSS_ROWS],
                    s[VLOSS_CLIPPED] / s[VLOSS_ROWS]))
        if (it + 1) % a.eval_every == 0 or it == 0:
            r, k = evaluate(ctx, pol, a, 1000 + it)
            line += "  | greedy first-episode return %.2f (%d episodes)" % (r, k)
        print(line, flush=True)
    pol.close()
    val.close()
    venv.close()
    ctx.close()


if __name__ == "__main__":
    main()
