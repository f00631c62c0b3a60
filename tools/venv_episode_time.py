#!/usr/bin/env python3
"""Kernel time of xh_venv_act (PROBS / SAMPLE, no record) and of xh_venv_step
with the episode statistics (xh_venv_set_episode_stats) off and on, and of the
xh_venv_episode_row launch alone, from xh_venv_kernel_time (HIP events around
each launch): ms per launch and the achieved GB/s over the algorithmic bytes,
at 64 bins, 2-D, with 32768 and 1,048,576 envs.

    python tools/venv_episode_time.py
    python tools/venv_episode_time.py --package-root build/prev_tree
                        # the parent commit's package, built in its own tree:
                        # the arms without statistics only

Bytes per env step: step 2 B D + 13 and act 4 B + 8 more (tools/
venv_act_time.py); statistics add 8 (the env's running length,
read and written) and, for the share of steps that end an episode -- printed
with the "on" arms, from the rows -- one 32-byte accumulator line and the
env's first length.  The row launch reads 40 bytes per env (running, first,
accumulators) and writes 32 where the env finished an episode since the last
row.  Each figure is the mean over --launches launches, repeated --reps times:
median [min .. max] of the repetitions.  For an A/B of two libraries run the
script once per library, alternating, in one session."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(env, launch, launches, reps, warmup):
    for _ in range(warmup):
        launch()
    env.synchronize()
    out = []
    for _ in range(reps):
        env.set_timing(True)
        for _ in range(launches):
            launch()
        ms, n = env.kernel_time()
        env.set_timing(False)
        assert n == launches, (n, launches)
        out.append(ms / n)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 1048576])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--package-root", default=REPO,
                    help="import dependence_free_rl_amd from this tree (a "
                    "checkout of another commit with its library built)")
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))

    from dependence_free_rl_amd import Context, VecEnv, _lib
    B, D = a.bins, a.dims
    has_stats = hasattr(VecEnv, "set_episode_stats")
    ctx = Context(device=0)
    rows = []
    for N in a.envs:
        env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7,
                     policy_draws=2)
        g = np.random.default_rng(N)
        env.set_actions(g.integers(0, B, N).astype(np.int32))
        env.set(_lib.VENV_POLICY,
                g.random((N, B), dtype=np.float32) + np.float32(0.01))
        step_bytes = 2 * B * D + 13
        act_bytes = step_bytes + 4 * B + 8
        cases = [("step", False, step_bytes), ("act", False, act_bytes)]
        if has_stats:
            cases += [("step+stats", True, step_bytes + 8),
                      ("act+stats", True, act_bytes + 8),
                      ("episode_row", True, 40)]
        for name, on, nbytes in cases:
            if has_stats:
                env.set_episode_stats(4 if on else 0)
            if name.startswith("step"):
                launch = lambda: env.step(fetch=False)  # noqa: E731
            elif name.startswith("act"):
                launch = lambda: env.act(fetch=False)  # noqa: E731
            else:
                launch = env.episode_row
            per = measure(env, launch, a.launches, a.reps, a.warmup)
            med = float(np.median(per))
            row = {"lib": _lib.LIB_PATH, "kernel": name, "envs": N, "bins": B,
                   "dims": D, "bytes_per_env": nbytes, "ms": med,
                   "ms_min": min(per), "ms_max": max(per),
                   "gb_s": N * nbytes / med / 1e6}
            note = ""
            if on and name != "episode_row":
                env.episode_row()
                r = env.episode_stats(count=1)[0]
                row["end_share"] = r[_lib.VEP_EPISODES] / (r[_lib.VEP_CALLS] * N)
                note = "  %.2f%% of the steps end an episode" % (
                    100 * row["end_share"])
            rows.append(row)
            print("%-12s %8d envs  %.4f ms [%.4f .. %.4f]  %7.1f GB/s  (%d B "
                  "per env)%s" % (name, N, med, min(per), max(per),
                                  row["gb_s"], nbytes, note), flush=True)
        env.close()
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
