#!/usr/bin/env python3
"""Time of a venv learner's policy on its logit table (xh_venv_table_*)
against the per-row chain in the same process -- 64 bins, 2-D, [128,128], at
32768 and 1 M envs, on the builtin item set and on examples/venv_ppo.py's:

  step    one rollout step: PolicyNet.forward(OBS) + act(write_obs) against
          act_table; the table's own forward (once per window) separately
  act     act_table alone against xh_venv_act on a resident row of logits
  epoch   one epoch over the T = 4 recorded steps in minibatches: record_obs
          + forward + policy_loss + backward against table_logits +
          policy_loss + table_grad, and one backward on the table

    python tools/venv_table_time.py
    python tools/venv_table_time.py --envs 32768 --out profiles/venv_table_time.jsonl

Every array stays on the device (the C ABI is called with device pointers).
Each figure is the mean over --launches calls between two stream
synchronisations (host clock), after --warmup calls, repeated --reps times:
median [min .. max].  One JSON line per figure goes to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_SET = dict(items=[[5, 1], [2, 3], [3, 3], [1, 1]],
                   weights=[0.3, 0.3, 0.2, 0.2], capacity=[10, 6])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 1 << 20])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--widths", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--minibatch", type=int, default=32768)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--epoch-launches", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "venv_table_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    from dependence_free_rl_amd import (VENV_POLICY, Context, PolicyNet,
                                        VecEnv, _lib, init_policy)
    lib = _lib.lib
    ctx = Context(device=0)
    B, D, T = a.bins, 2, a.steps
    widths = tuple(a.widths)

    def dev(nfloats):
        p = C.c_void_p()
        _lib.check(_lib.tensor_alloc(ctx.h, nfloats, C.byref(p)))
        return p.value

    def timed(call, launches):
        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        per = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(launches):
                call()
            ctx.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / launches)
        return float(np.median(per)), min(per), max(per)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def report(what, chain, N, set_name, t, **extra):
        key = "ratio" if what == "ratio" else "ms"
        row = dict(what=what, chain=chain, envs=N, bins=B, dims=D,
                   widths=list(widths), steps=T, set=set_name, **{key: t[0]},
                   **extra)
        if what != "ratio":
            row.update(ms_min=t[1], ms_max=t[2])
        out.write(json.dumps(row) + "\n")
        out.flush()
        print("%-6s %-24s %8d envs %-8s %9.4f %s [%.4f .. %.4f] %s"
              % (what, chain, N, set_name, t[0], "x " if what == "ratio"
                 else "ms", t[1], t[2],
                 " ".join("%s=%s" % kv for kv in extra.items())), flush=True)
        return t[0]

    for N in a.envs:
        for set_name, kw in (("builtin", {}), ("example", EXAMPLE_SET)):
            venv = VecEnv(ctx, N, bins=B, dims=D, rng_state=3, **kw)
            pol = PolicyNet(ctx, B, D, widths)
            pol.params = init_policy(D, widths[0], widths[1], seed=1)
            info = venv.table_info()
            E, R = info["entries"], info["rows"]
            venv.set_record(T)
            venv.observe()
            total = T * N
            mb = min(a.minibatch, total)
            tobs, table, G = dev(R * B * 2 * D), dev(R * B), dev(R * B)
            obs_mb, logits_mb, adv = dev(mb * B * 2 * D), dev(mb * B), dev(total)
            # (a name for the host array: it must outlive the copy)
            adv_host = np.random.default_rng(1).standard_normal(
                total).astype(np.float32)
            _lib.check(_lib.tensor_copy(ctx.h, adv, adv_host.ctypes.data,
                                        total, _lib.COPY_H2D))
            venv.table_obs(out=tobs)
            policy = venv.device_ptr(VENV_POLICY)

            def table_forward():
                pol.forward(tobs, rows=R, out=table)

            # ---- one rollout step ------------------------------------------
            def step_rows():
                venv.rewind()
                pol.forward(venv, out=policy)
                venv.act(None, kind="logits", write_obs=True, fetch=False)

            def step_table():
                venv.rewind()
                venv.act_table(table)

            def act_rows():
                venv.rewind()
                venv.act(None, kind="logits", fetch=False)

            table_forward()
            t_rows = report("step", "per-row", N, set_name,
                            timed(step_rows, a.launches))
            t_tab = report("step", "table", N, set_name,
                           timed(step_table, a.launches), entries=E)
            t_fwd = report("step", "table-forward", N, set_name,
                           timed(table_forward, a.launches), rows=R)
            t_act = report("act", "resident-row", N, set_name,
                           timed(act_rows, a.launches))
            report("ratio", "step per-row / table", N, set_name,
                   (t_rows / t_tab,) * 3,
                   with_forward_over_T=t_rows / (t_tab + t_fwd / T))
            report("ratio", "act_table / act", N, set_name,
                   (t_tab / t_act,) * 3)

            # ---- one epoch over the window -----------------------------------
            venv.rewind()
            for _ in range(T):
                venv.act_table(table)
            venv.synchronize()

            def loss(first, count):
                p = _lib.VenvLoss()
                p.policy, p.grad = logits_mb, logits_mb  # in place
                p.kind, p.loss = _lib.ACT_LOGITS, _lib.LOSS_CLIPPED
                p.first, p.count, p.total = first, count, total
                p.adv, p.eps, p.scale = adv, 0.2, 1.0 / total
                _lib.check(lib.xh_venv_policy_loss(venv.h, C.byref(p)))

            def epoch_rows():
                for first in range(0, total, mb):
                    count = min(mb, total - first)
                    venv.record_obs("state", first=first, count=count,
                                    out=obs_mb)
                    pol.forward(obs_mb, rows=count, out=logits_mb)
                    loss(first, count)
                    pol.backward(obs_mb, logits_mb, rows=count,
                                 accumulate=first > 0)

            def epoch_table():
                table_forward()
                for first in range(0, total, mb):
                    count = min(mb, total - first)
                    venv.table_logits(table, first=first, count=count,
                                      out=logits_mb)
                    loss(first, count)
                    venv.table_grad(logits_mb, first=first, count=count,
                                    accumulate=first > 0, out=G)
                pol.backward(tobs, G, rows=R)

            e_rows = report("epoch", "per-row", N, set_name,
                            timed(epoch_rows, a.epoch_launches),
                            minibatch=mb)
            e_tab = report("epoch", "table", N, set_name,
                           timed(epoch_table, a.epoch_launches), minibatch=mb)
            report("ratio", "epoch per-row / table", N, set_name,
                   (e_rows / e_tab,) * 3)
            venv.synchronize()
            for p in (tobs, table, G, obs_mb, logits_mb, adv):
                _lib.check(_lib.tensor_free(ctx.h, p))
            pol.close()
            venv.close()
    ctx.close()
    out.close()


if __name__ == "__main__":
    main()
