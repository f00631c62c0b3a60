#!/usr/bin/env python3
"""Time of a venv learner's value net read straight from the record
(xh_net_forward_record / xh_net_backward_record) against the layer path
(xh_venv_record_obs + xh_net_forward / xh_net_backward) in the same process --
64 bins 2-D at 32768 envs and 128 bins 3-D at 4096 envs, T = 4:

  window  the values of a window, (T + 1) N rows of the STATE view
  epoch   one epoch's value work over the T N recorded rows through a shuffled
          index list, in minibatches of 4096 and of 32768 rows: per minibatch
          one forward (for the loss head) and one backward

    python tools/venv_value_time.py
    python tools/venv_value_time.py --out profiles/venv_value_time.jsonl

Every array stays on the device (device pointers throughout).  Each figure is
the mean over --launches calls between two stream synchronisations (host
clock), after --warmup calls, repeated --reps times: median [min .. max].  One
JSON line per figure goes to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE_SETS = {2: dict(items=[[5, 1], [2, 3], [3, 3], [1, 1]],
                        weights=[0.3, 0.3, 0.2, 0.2], capacity=[10, 6]),
                3: dict(items=[[5, 1, 2], [2, 3, 1], [3, 3, 4]],
                        capacity=[10, 6, 7])}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="64x2x32768,128x3x4096",
                    help="bins x dims x envs, comma separated")
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--minibatch", type=int, nargs="+", default=[4096, 32768])
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "venv_value_time.jsonl"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    from dependence_free_rl_amd import Context, ValueNet, VecEnv, _lib
    ctx = Context(device=0)
    T = a.steps

    def dev(nwords):
        p = C.c_void_p()
        _lib.check(_lib.tensor_alloc(ctx.h, nwords, C.byref(p)))
        return p.value

    def put(ptr, arr):  # 4-byte elements
        _lib.check(_lib.tensor_copy(ctx.h, ptr, arr.ctypes.data, arr.size,
                                    _lib.COPY_H2D))

    def timed(call):
        for _ in range(a.warmup):
            call()
        ctx.synchronize()
        per = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(a.launches):
                call()
            ctx.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / a.launches)
        return float(np.median(per)), min(per), max(per)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = open(a.out, "w")

    def report(what, path, shape, t, **extra):
        B, D, N = shape
        key = "ratio" if what == "ratio" else "ms"
        row = dict(what=what, path=path, envs=N, bins=B, dims=D, steps=T,
                   **{key: t[0]}, **extra)
        if what != "ratio":
            row.update(ms_min=t[1], ms_max=t[2])
        out.write(json.dumps(row) + "\n")
        out.flush()
        print("%-6s %-22s %3d bins %d-D %6d envs %9.4f %s [%.4f .. %.4f] %s"
              % (what, path, B, D, N, t[0], "x " if what == "ratio" else "ms",
                 t[1], t[2], " ".join("%s=%s" % kv for kv in extra.items())),
              flush=True)
        return t[0]

    for spec in a.shapes.split(","):
        B, D, N = (int(x) for x in spec.split("x"))
        shape = (B, D, N)
        venv = VecEnv(ctx, N, bins=B, dims=D, rng_state=3, **EXAMPLE_SETS[D])
        val = ValueNet(ctx, B, D)
        val.init(2)
        venv.set_record(T)
        for _ in range(T):
            venv.act_heuristic("random")
        venv.synchronize()
        window, total = (T + 1) * N, T * N
        F = B * 2 * D
        obs, values = dev(window * F), dev(window)
        rng = np.random.default_rng(1)
        # (names for the host arrays: they must outlive the copies)
        perm_host = rng.permutation(total).astype(np.int32)
        dv_host = rng.standard_normal(total).astype(np.float32)
        perm, dv = dev(total), dev(total)
        put(perm, perm_host)
        put(dv, dv_host)

        # ---- the values of a window ------------------------------------------
        def window_layers():
            venv.record_obs("state", first=0, count=window, out=obs)
            val.forward(obs, rows=window, out=values)

        def window_record():
            val.forward_record(venv, "state", first=0, count=window, out=values)

        t_l = report("window", "layers", shape, timed(window_layers), rows=window)
        t_r = report("window", "record", shape, timed(window_record), rows=window)
        report("ratio", "window layers / record", shape, (t_l / t_r,) * 3)

        # ---- one epoch's value work --------------------------------------------
        for mb in sorted({min(m, total) for m in a.minibatch}):
            def epoch_layers():
                for first in range(0, total, mb):
                    count = min(mb, total - first)
                    venv.record_obs("state", rows=perm, first=first,
                                    count=count, out=obs)
                    val.forward(obs, rows=count, out=values)
                    val.backward(obs, dv + 4 * first, rows=count,
                                 accumulate=first > 0)

            def epoch_record():
                for first in range(0, total, mb):
                    count = min(mb, total - first)
                    at = dict(rows=perm, first=first, count=count)
                    val.forward_record(venv, "state", out=values, **at)
                    val.backward_record(venv, dv + 4 * first, "state",
                                        accumulate=first > 0, **at)

            e_l = report("epoch", "layers", shape, timed(epoch_layers),
                         minibatch=mb, rows=total)
            e_r = report("epoch", "record", shape, timed(epoch_record),
                         minibatch=mb, rows=total)
            report("ratio", "epoch layers / record", shape, (e_l / e_r,) * 3,
                   minibatch=mb)
        venv.synchronize()
        for p in (obs, values, perm, dv):
            _lib.check(_lib.tensor_free(ctx.h, p))
        val.close()
        venv.close()
    ctx.close()
    out.close()


if __name__ == "__main__":
    main()
