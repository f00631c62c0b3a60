#!/usr/bin/env python3
"""What general item sets (xh_item_set) cost, and that the builtin path costs
what it did: kernel time of xh_venv_step and xh_venv_act (PROBS / SAMPLE, no
record, no observations; --obs adds act with the observations) from
xh_venv_kernel_time, at 64 bins, 2-D, with 32768 and 1,048,576 envs.

    python tools/venv_items_time.py --parent-lib build/parent/libxylo_hip.so \\
        --jsonl profiles/venv_items_ab.jsonl

Arms, each measured in a process of its own (a library is chosen when the
package is imported), one process at a time:
  parent    the parent commit's library (--parent-lib, loaded through
            XH_LIB_PATH), the builtin path;
  builtin   this tree's library, a venv created without an item set;
  default   this tree's library, the general kernels on the default set;
  k5 / k16  the general kernels on a 5-item and a 16-item set.
parent and builtin alternate for --rounds rounds; the general arms run once
per round after them.  A figure is the mean over --launches launches, repeated
--reps times; a round's value is the median of its repetitions.

The summary gives, per kernel and size: the medians over the rounds; the
parent's spread against itself (max - min of its rounds' values); the builtin
path's difference to the parent (gate: within that spread -- it is meant to be
the same code); and the general arms' ratios to the builtin path (no gate)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ITEMS5 = [(3, 1), (2, 2), (1, 4), (4, 2), (1, 1)]
ITEMS16 = [(1 + k % 7, 1 + (3 * k) % 5) for k in range(16)]
SETS = {"default": dict(items=[(4, 2), (1, 2)], weights=[0.4, 0.6]),
        "k5": dict(items=ITEMS5, weights=[2.0, 1.0, 1.0, 0.5, 3.25]),
        "k16": dict(items=ITEMS16,
                    weights=[1.0 + (5 * k) % 7 for k in range(16)])}


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


def child(a):
    """One arm in this process: a JSON line per (kernel, envs) on stdout."""
    sys.path.insert(0, REPO)
    from dependence_free_rl_amd import Context, VecEnv, _lib
    B, D = a.bins, a.dims
    ctx = Context(device=0)
    kw = SETS.get(a.arm, {})
    for N in a.envs:
        env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7,
                     policy_draws=2, **kw)
        g = np.random.default_rng(N)
        env.set_actions(g.integers(0, B, N).astype(np.int32))
        env.set(_lib.VENV_POLICY,
                g.random((N, B), dtype=np.float32) + np.float32(0.01))
        kernels = [("step", lambda: env.step(fetch=False)),
                   ("act", lambda: env.act(fetch=False))]
        if a.obs:  # + 8 B D bytes per env step; the general path divides
            kernels.append(("act+obs", lambda: env.act(write_obs=True,
                                                       fetch=False)))
        for name, launch in kernels:
            per = measure(env, launch, a.launches, a.reps, a.warmup)
            print(json.dumps({"arm": a.arm, "lib": _lib.LIB_PATH,
                              "kernel": name, "envs": N, "bins": B, "dims": D,
                              "ms": float(np.median(per)), "ms_min": min(per),
                              "ms_max": max(per)}), flush=True)
        env.close()
    ctx.close()


def run_arm(a, arm, rnd):
    env = dict(os.environ)
    env.pop("XH_LIB_PATH", None)
    if arm == "parent":
        env["XH_LIB_PATH"] = os.path.abspath(a.parent_lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--arm", arm,
           "--bins", str(a.bins), "--dims", str(a.dims), "--launches",
           str(a.launches), "--reps", str(a.reps), "--warmup", str(a.warmup),
           "--envs"] + [str(n) for n in a.envs] + (["--obs"] if a.obs else [])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True,
                         text=True, timeout=a.arm_timeout).stdout
    rows = [json.loads(line) for line in out.splitlines() if line[:1] == "{"]
    for r in rows:
        r["round"] = rnd
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 1048576])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--arm-timeout", type=int, default=240)
    ap.add_argument("--obs", action="store_true",
                    help="add act with write_obs (the general path's f32 "
                    "divisions by the capacities)")
    ap.add_argument("--parent-lib", help="the parent commit's libxylo_hip.so")
    ap.add_argument("--label", default="", help="session / library label "
                    "written into every line")
    ap.add_argument("--jsonl", help="append the rows and the summary here")
    ap.add_argument("--arm", help="(internal) measure this arm in this process")
    a = ap.parse_args()
    if a.arm:
        return child(a)
    arms = (["parent"] if a.parent_lib else []) + ["builtin"]
    rows = []
    for rnd in range(a.rounds):
        for arm in arms + list(SETS):
            got = run_arm(a, arm, rnd)
            rows += got
            for r in got:
                print("round %d %-8s %-4s %8d envs  %.4f ms [%.4f .. %.4f]"
                      % (rnd, arm, r["kernel"], r["envs"], r["ms"],
                         r["ms_min"], r["ms_max"]), flush=True)
    summary = []
    for kernel in ("step", "act") + (("act+obs",) if a.obs else ()):
        for N in a.envs:
            val = {arm: [r["ms"] for r in rows if r["arm"] == arm and
                         r["kernel"] == kernel and r["envs"] == N]
                   for arm in arms + list(SETS)}
            med = {arm: float(np.median(v)) for arm, v in val.items()}
            s = {"summary": True, "kernel": kernel, "envs": N, "bins": a.bins,
                 "dims": a.dims, "rounds": a.rounds, "median_ms": med,
                 "general_over_builtin": {
                     k: med[k] / med["builtin"] for k in SETS}}
            if a.parent_lib:
                s["parent_spread_ms"] = max(val["parent"]) - min(val["parent"])
                s["builtin_minus_parent_ms"] = med["builtin"] - med["parent"]
                s["builtin_within_parent_spread"] = bool(
                    abs(s["builtin_minus_parent_ms"]) <= s["parent_spread_ms"])
            summary.append(s)
            print(json.dumps(s), flush=True)
    if a.jsonl:
        with open(a.jsonl, "a") as f:
            for r in rows + summary:
                f.write(json.dumps(dict(r, label=a.label)) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
