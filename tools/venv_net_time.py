#!/usr/bin/env python3
"""Time per call of the device-resident policy net (PolicyNet: the fused
net_policy_fwd_kernel / net_policy_bwd_kernel + slab_reduce) against the same
rows through the layer-by-layer launches (LayerPolicyNet, XH_NET_POLICY_LAYERS:
layer_forward / layer_gradient / layer_backward of dense_kernels.hip, the
launches xh_model_forward / xh_model_gradient run, on device buffers, every
activation materialised) -- at 64 bins, 2-D, [128,128], 8192 and 32768 rows.

    python tools/venv_net_time.py
    python tools/venv_net_time.py --rows 8192 --widths 64 64 --json out.json

Each figure is the mean over --launches calls between two stream
synchronisations (host clock; at these sizes a call is hundreds of
microseconds to milliseconds, the launch gaps a few microseconds), after
--warmup calls, repeated --reps times: median [min .. max].

Bytes by the model of DESIGN.md 3.2, R = rows * bins flat rows, F0 = 2 dims:
fused forward R (4 F0 + 4); fused backward R (4 F0 + 4) + slabs; the layer
launches write and re-read every activation: forward R (4 F0 + 4 (4 H1 + 4 H2)
+ 4) (pre-activation written, read by relu, relu's output written, read by
the next layer), backward that again plus R 4 (3 H1 + 3 H2) of backprop
traffic.  FLOP: forward 2 R (F0 H1 + H1 H2 + H2), backward recomputes the
forward and adds 2 R (2 H1 H2 + F0 H1 + H2)."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_F32_MFMA = 157.3e12  # MI355X f32-input MFMA, FLOP/s


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[8192, 32768])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--widths", type=int, nargs=2, default=[128, 128])
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import ctypes as C

    from dependence_free_rl_amd import Context, PolicyNet, _lib, init_policy
    from dependence_free_rl_amd.nets import LayerPolicyNet
    ctx = Context(device=0)
    B, D, (H1, H2) = a.bins, a.dims, a.widths
    F0 = 2 * D

    def dev(nfloats):
        p = C.c_void_p()
        _lib.check(_lib.tensor_alloc(ctx.h, nfloats, C.byref(p)))
        return p.value

    def put(ptr, arr):
        arr = np.ascontiguousarray(arr, np.float32)
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

    params = init_policy(D, H1, H2, seed=1)
    out_rows = []
    for rows in a.rows:
        R = rows * B
        g = np.random.default_rng(rows)
        obs, logits, dout = dev(R * F0), dev(R), dev(R)
        # eighths like the venv's observations; chunked uploads
        chunk = 1 << 22
        xs = (g.integers(0, 9, min(R * F0, chunk)) / 8.0).astype(np.float32)
        for off in range(0, R * F0, chunk):
            put(obs + 4 * off, xs[:min(chunk, R * F0 - off)])
        ds = g.standard_normal(min(R, chunk)).astype(np.float32)
        for off in range(0, R, chunk):
            put(dout + 4 * off, ds[:min(chunk, R - off)])
        flop_f = 2.0 * R * (F0 * H1 + H1 * H2 + H2)
        flop_b = flop_f + 2.0 * R * (2 * H1 * H2 + F0 * H1 + H2)
        acts = 4 * (4 * H1 + 4 * H2)
        res = {}
        for name, cls in (("fused", PolicyNet), ("layers", LayerPolicyNet)):
            net = cls(ctx, B, D, (H1, H2))
            net.params = params
            f = timed(lambda: net.forward(obs, rows=rows, out=logits))
            b = timed(lambda: net.backward(obs, dout, rows=rows))
            info = net.info()
            if name == "fused":
                by_f = R * (4 * F0 + 4)
                by_b = R * (4 * F0 + 4) + 4 * info["slabs"] * net.num_params
            else:
                by_f = R * (4 * F0 + acts + 4)
                by_b = by_f + R * 4 * (3 * H1 + 3 * H2)
            res[name] = (f, b)
            for what, t, by, fl in (("forward", f, by_f, flop_f),
                                    ("backward", b, by_b, flop_b)):
                row = {"net": name, "call": what, "rows": rows, "bins": B,
                       "dims": D, "widths": [H1, H2], "ms": t[0],
                       "ms_min": t[1], "ms_max": t[2], "bytes": by,
                       "tb_s": by / t[0] / 1e9, "tflops": fl / t[0] / 1e9,
                       "peak_fraction": fl / (t[0] * 1e-3) / PEAK_F32_MFMA,
                       "grid": info["grid"].get(what, 0)}
                out_rows.append(row)
                print("%-6s %-8s %6d rows B=%d D=%d [%d,%d]  %.4f ms [%.4f .. "
                      "%.4f]  %8.1f MB  %5.2f TB/s  %6.2f TF (%.1f %% of peak)"
                      % (name, what, rows, B, D, H1, H2, t[0], t[1], t[2],
                         by / 1e6, row["tb_s"], row["tflops"],
                         100 * row["peak_fraction"]), flush=True)
            net.close()
        for k, what in enumerate(("forward", "backward")):
            print("ratio layers / fused, %s, %d rows: %.2f"
                  % (what, rows, res["layers"][k][0] / res["fused"][k][0]),
                  flush=True)
        ctx.synchronize()
        for p in (obs, logits, dout):
            _lib.check(_lib.tensor_free(ctx.h, p))
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out_rows, f, indent=1)


if __name__ == "__main__":
    main()
