#!/usr/bin/env python3
"""Kernel time of the learner-side venv kernels, from xh_venv_kernel_time (HIP
events around each launch): venv_gae_kernel (xh_venv_advantages on the
record's window, adv + td_target + lambda_return, with and without v_term)
and venv_record_obs_kernel (xh_venv_record_obs: a run of N rows, and N
shuffled rows of the whole record, STATE and NEXT), beside
venv_observe_kernel (xh_venv_observe) on the same venv.  64 bins, 2-D, with
32768 and 1,048,576 envs and windows of T = 4 and 64 steps.

    python tools/venv_learn_time.py
    python tools/venv_learn_time.py --envs 32768 --steps 4 --json out.json
    python tools/venv_learn_time.py --envs 1048576 --steps 4 --only venv_gae
                        # one case alone, e.g. under a kernel trace

Bytes by the kernels' models: the scan reads 4 (T + 1) + T +
4 T per env (+ 4 T with v_term) and writes 4 T per output; an observation row
reads B D + 4 and writes 8 B D (+ 4 with an index list, + 9 for NEXT);
xh_venv_observe moves the same B D + 4 and 8 B D per env.  Each figure is the
mean over --launches launches, repeated --reps times: median [min .. max].
Every array stays on the device (the venv's record, xh_tensor_alloc blocks);
only the policy rows that drive the recorded steps are uploaded."""
import argparse
import ctypes as C
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
        out.append(ms / launches)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 1048576])
    ap.add_argument("--steps", type=int, nargs="+", default=[4, 64])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", nargs="+", metavar="NAME",
                    help="run these cases alone, by the name printed (for a "
                    "kernel trace of one case)")
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    sys.path.insert(0, REPO)

    from dependence_free_rl_amd import Context, VecEnv, _lib
    lib, check = _lib.lib, _lib.check
    B, D = a.bins, a.dims
    ctx = Context(device=0)

    def dev(nbytes):
        p = C.c_void_p()
        check(_lib.tensor_alloc(ctx.h, (nbytes + 3) // 4, C.byref(p)))
        return p.value

    def put(ptr, arr):
        arr = np.ascontiguousarray(arr)
        check(_lib.tensor_copy(ctx.h, ptr, arr.ctypes.data, arr.nbytes // 4,
                               _lib.COPY_H2D))

    rows_out = []

    def wanted(name):
        return not a.only or name in a.only

    def report(name, N, T, nbytes, per):
        med = float(np.median(per))
        row = {"kernel": name, "envs": N, "steps": T, "bins": B, "dims": D,
               "bytes": nbytes, "ms": med, "ms_min": min(per),
               "ms_max": max(per), "tb_s": nbytes / med / 1e9}
        rows_out.append(row)
        print("%-28s %8d envs T=%-3d %.4f ms [%.4f .. %.4f]  %6.1f MB  "
              "%5.2f TB/s" % (name, N, T, med, min(per), max(per),
                              nbytes / 1e6, row["tb_s"]), flush=True)

    for N in a.envs:
        g = np.random.default_rng(N)
        policy = g.random((N, B), dtype=np.float32) + np.float32(0.01)
        policy[::4, 0] = 50.0  # every fourth env overflows bin 0 and resets
        for T in a.steps:
            env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7)
            env.set(_lib.VENV_POLICY, policy)
            env.set_record(T)
            for _ in range(T):
                env.act(fetch=False)
            env.synchronize()
            blocks = []
            # ---- the scan: values, v_term and the three outputs on the device
            n = T * N
            vals, vterm = dev(4 * (n + N)), dev(4 * n)
            outs = [dev(4 * n) for _ in range(3)]
            blocks += [vals, vterm] + outs
            chunk = g.standard_normal(min(n + N, 1 << 22)).astype(np.float32)
            for off in range(0, n + N, len(chunk)):
                m = min(len(chunk), n + N - off)
                put(vals + 4 * off, chunk[:m])
                if off < n:
                    put(vterm + 4 * off, chunk[:min(m, n - off)])
            for name, vt in (("venv_gae", None), ("venv_gae +v_term", vterm)):
                if not wanted(name):
                    continue
                adv = _lib.VenvAdv()
                adv.steps, adv.values, adv.v_term = 0, vals, vt
                adv.gamma, adv.lambda_ = 0.99, 0.95
                adv.adv, adv.td_target, adv.lambda_return = outs

                def launch():
                    check(lib.xh_venv_advantages(env.h, C.byref(adv)))
                per = measure(env, launch, a.launches, a.reps, a.warmup)
                nbytes = N * (4 * (T + 1) + T + 4 * T + (4 * T if vt else 0)
                              + 3 * 4 * T)
                report(name, N, T, nbytes, per)
            # ---- observations: N rows per launch
            obs = dev(N * B * 2 * D * 4)
            idx_state, idx_next = dev(4 * N), dev(4 * N)
            blocks += [obs, idx_state, idx_next]
            put(idx_state, g.integers(0, (T + 1) * N, N).astype(np.int32))
            put(idx_next, g.integers(0, T * N, N).astype(np.int32))
            row_rw = B * D + 4 + 8 * B * D
            cases = [("record_obs STATE run", _lib.VOBS_STATE, None,
                      (T // 2) * N, row_rw),
                     ("record_obs NEXT run", _lib.VOBS_NEXT, None,
                      (T // 2) * N, row_rw + 9),
                     ("record_obs STATE gather", _lib.VOBS_STATE, idx_state, 0,
                      row_rw + 4),
                     ("record_obs NEXT gather", _lib.VOBS_NEXT, idx_next, 0,
                      row_rw + 13)]
            for name, view, idx, first, per_row in cases:
                if not wanted(name):
                    continue

                def launch():
                    check(lib.xh_venv_record_obs(env.h, view, idx, first, N,
                                                 obs))
                per = measure(env, launch, a.launches, a.reps, a.warmup)
                report(name, N, T, N * per_row, per)

            def launch():
                check(lib.xh_venv_observe(env.h))
            if wanted("venv_observe"):
                per = measure(env, launch, a.launches, a.reps, a.warmup)
                report("venv_observe", N, T, N * row_rw, per)
            env.synchronize()
            env.close()
            for p in blocks:
                check(_lib.tensor_free(ctx.h, p))
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
