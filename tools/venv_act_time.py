#!/usr/bin/env python3
"""Kernel time of xh_venv_act (PROBS / SAMPLE) and of xh_venv_step, from
xh_venv_kernel_time (HIP events around each launch): ms per launch and the
achieved GB/s over the algorithmic bytes, at 64 bins, 2-D, with 32768 and
1,048,576 envs, the trajectory record off and on (with the states), and with
--distrib also with the distribution record (xh_venv_set_record_distrib).

    python tools/venv_act_time.py                  # act and step
    python tools/venv_act_time.py --distrib --bins 128 --envs 32768
    python tools/venv_act_time.py --mask --envs 32768   # + the masked arms
    python tools/venv_act_time.py --step-only --package-root build/prev_tree
                        # the parent commit's package, built in its own tree

Bytes per env step: step 2 B D + 13 (bins read and written, item read and
written, action, stream state read and written ... DESIGN.md §3.2); act adds
the policy row and the two outputs, 4 B + 8; the record adds 13, and B D + 4
with the states, and 4 B with the distributions; --mask repeats the act arms
with invalid-action masking on (xh_venv_set_action_mask), which adds 4 W, W =
max(1, B / 32), where there is a record.  Each figure is the mean over --launches launches, repeated
--reps times: median [min .. max] of the repetitions.  For an A/B of two
libraries run the script once per library, alternating, in one session."""
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
    ap.add_argument("--step-only", action="store_true",
                    help="xh_venv_step alone (a library without xh_venv_act)")
    ap.add_argument("--distrib", action="store_true",
                    help="add the arm with the distribution record on")
    ap.add_argument("--mask", action="store_true",
                    help="repeat the act arms with the action mask on")
    ap.add_argument("--package-root", default=REPO,
                    help="import dependence_free_rl_amd from this tree (a "
                    "checkout of another commit with its library built)")
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))

    from dependence_free_rl_amd import Context, VecEnv, _lib
    B, D = a.bins, a.dims
    ctx = Context(device=0)
    rows = []
    if a.mask and not hasattr(VecEnv, "set_action_mask"):
        ap.error("--mask: this package has no VecEnv.set_action_mask")
    for N in a.envs:
        env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7,
                     policy_draws=2)
        g = np.random.default_rng(N)
        env.set_actions(g.integers(0, B, N).astype(np.int32))
        step_bytes = 2 * B * D + 13
        cases = [("step", None, step_bytes)]
        if not a.step_only:
            env.set(_lib.VENV_POLICY,
                    g.random((N, B), dtype=np.float32) + np.float32(0.01))
            act_bytes = step_bytes + 4 * B + 8
            cases += [("act", 0, act_bytes),
                      ("act+record", a.launches, act_bytes + 13 + B * D + 4)]
            if a.distrib:
                cases += [("act+rec+dist", a.launches,
                           act_bytes + 13 + B * D + 4 + 4 * B)]
            if a.mask:
                W = max(1, B // 32)
                cases += [(n + "+mask", r, nb + (4 * W if r else 0))
                          for n, r, nb in cases[1:]]
        for name, record, nbytes in cases:
            if a.mask and name != "step":
                env.set_record(0)  # the mask is switched at cursor 0
                env.set_action_mask(name.endswith("+mask"))
            if name.startswith("act+rec+dist"):
                env.set_record(record, distrib=True)
            elif record is not None:
                env.set_record(record)

            def launch():
                if name == "step":
                    env.step(fetch=False)
                    return
                if record and env.record_pos() == record:
                    env.rewind()
                env.act(fetch=False)
            per = measure(env, launch, a.launches, a.reps, a.warmup)
            med = float(np.median(per))
            row = {"lib": _lib.LIB_PATH, "kernel": name, "envs": N, "bins": B,
                   "dims": D, "bytes_per_env": nbytes, "ms": med,
                   "ms_min": min(per), "ms_max": max(per),
                   "gb_s": N * nbytes / med / 1e6}
            rows.append(row)
            print("%-17s %8d envs  %.4f ms [%.4f .. %.4f]  %7.1f GB/s  (%d B "
                  "per env step)" % (name, N, med, min(per), max(per),
                                     row["gb_s"], nbytes), flush=True)
        env.close()
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
