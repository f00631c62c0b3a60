#!/usr/bin/env python3
"""Kernel time of the VecEnv loss head, from xh_venv_kernel_time (HIP events
around the loss launch; the one-wave launch that reduces the statistics is
not timed): venv_policy_loss_kernel (xh_venv_policy_loss) on logits, clipped
loss, a shuffled minibatch gathered through an index list, with the value
head, with and without probs_out and stats -- at 131,072 and 1,048,576 rows
of 64 bins and of 128 bins.  --kl adds the KL-regulated loss on the same
rows (each row's sampling distribution gathered through the index list), alone
and with kl_stats, and kl_stats under the clipped loss.  --mask adds the
masked launch (xh_venv_policy_loss_masked: each row's legal words gathered
through the index list), plain and with probs_out and stats.  --ent adds
xh_venv_policy_loss_ex's arms: the entropy bonus alone, with the clipped value
loss (v_old gathered through the index list) and with ext_stats, and
ext_stats alone (the same instantiation, no logarithm).

    python tools/venv_loss_time.py
    python tools/venv_loss_time.py --kl
    python tools/venv_loss_time.py --mask --rows 32768
    python tools/venv_loss_time.py --ent
    python tools/venv_loss_time.py --package-root build/prev_tree
                        # the parent commit's package, built in its own tree
    python tools/venv_loss_time.py --rows 1048576 --bins 64 --json out.json
    python tools/venv_loss_time.py --torch     # the same loss in torch, alone

Bytes by the kernel's model: per row 4 B read, 4 B written,
4 B more with probs_out, and 28 gathered or scattered (the index, action,
p_old, adv, target, values_new, dvalue); the KL arms gather 4 B more (the
row's distribution), the masked arms 4 W more, W = max(1, B / 32) (the row's
legal words), the value clip 4 more (v_old), the bonus none.  Each figure is the mean over
--launches launches, repeated --reps times: median [min .. max].

--torch times the loss a caller would otherwise write on the device: gather,
softmax, clipped surrogate, value error and backward to the logits, eager
torch ops bracketed by events.  It runs in a process of its own (torch brings
its own HIP runtime) and prints the same kind of row."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_rows(a):
    import torch
    dev = torch.device("cuda:0")
    out = []
    for B in a.bins:
        for n in a.rows:
            g = torch.Generator(device=dev).manual_seed(n + B)
            total = 2 * n
            z = torch.randn(n, B, device=dev, generator=g, requires_grad=True)
            idx = torch.randperm(total, device=dev, generator=g)[:n]
            action = torch.randint(0, B, (total,), device=dev, generator=g)
            p_old = torch.rand(total, device=dev, generator=g) * 0.5 + 0.01
            adv = torch.randn(total, device=dev, generator=g)
            target = torch.randn(total, device=dev, generator=g)
            values = torch.randn(n, device=dev, generator=g, requires_grad=True)

            def step():
                z.grad = values.grad = None
                p = torch.softmax(z, dim=1)
                p_ch = p.gather(1, action[idx].unsqueeze(1)).squeeze(1)
                ratio = p_ch / p_old[idx]
                A = adv[idx]
                surr = torch.minimum(ratio.clamp(0.8, 1.2) * A, ratio * A)
                loss = -surr.sum() + 0.5 * ((values - target[idx]) ** 2).sum()
                loss.backward()
            for _ in range(a.warmup):
                step()
            per = []
            for _ in range(a.reps):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(a.launches):
                    step()
                e1.record()
                torch.cuda.synchronize()
                per.append(e0.elapsed_time(e1) / a.launches)
            med = float(np.median(per))
            out.append({"kernel": "torch eager loss + backward", "rows": n,
                        "bins": B, "ms": med, "ms_min": min(per),
                        "ms_max": max(per)})
            print("%-34s %8d rows B=%-3d %.4f ms [%.4f .. %.4f]"
                  % ("torch eager loss + backward", n, B, med, min(per),
                     max(per)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, nargs="+", default=[131072, 1048576])
    ap.add_argument("--bins", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kl", action="store_true",
                    help="add the KL-regulated loss and kl_stats arms")
    ap.add_argument("--mask", action="store_true",
                    help="add the masked arms (xh_venv_policy_loss_masked)")
    ap.add_argument("--ent", action="store_true",
                    help="add the entropy-bonus / value-clip arms "
                    "(xh_venv_policy_loss_ex)")
    ap.add_argument("--package-root", default=REPO,
                    help="import dependence_free_rl_amd from this tree (a "
                    "checkout of another commit with its library built)")
    ap.add_argument("--torch", action="store_true",
                    help="time the eager torch form instead (own process)")
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    if a.torch:
        rows_out = torch_rows(a)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows_out, f, indent=1)
        return
    sys.path.insert(0, os.path.abspath(a.package_root))

    from dependence_free_rl_amd import Context, VecEnv, _lib
    lib, check = _lib.lib, _lib.check
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
    for B in a.bins:
        env = VecEnv(ctx, num_envs=64, bins=B, dims=1, rng_state=7)
        for n in a.rows:
            g = np.random.default_rng(n + B)
            total = 2 * n
            blocks = {k: dev(4 * n * B) for k in ("z", "grad", "probs")}
            for k in ("idx", "values", "dvalue"):
                blocks[k] = dev(4 * n)
            for k in ("action", "p_old", "adv", "target"):
                blocks[k] = dev(4 * total)
            blocks["stats"] = dev(8 * _lib.VLOSS_COUNT)
            if a.kl:  # any positive rows do: the time does not depend on them
                blocks["distrib"] = dev(4 * total * B)
                blocks["kl_stats"] = dev(8 * _lib.VKL_COUNT)
                qs = (g.random(min(total * B, 1 << 22)) / B).astype(np.float32)
                for off in range(0, total * B, 1 << 22):
                    put(blocks["distrib"] + 4 * off,
                        qs[:min(1 << 22, total * B - off)])
            chunk = 1 << 22
            zs = g.standard_normal(min(n * B, chunk)).astype(np.float32)
            for off in range(0, n * B, chunk):
                put(blocks["z"] + 4 * off, zs[:min(chunk, n * B - off)])
            put(blocks["idx"], g.permutation(total)[:n].astype(np.int32))
            put(blocks["values"], g.standard_normal(n).astype(np.float32))
            action = g.integers(0, B, total).astype(np.int32)
            put(blocks["action"], action)
            if a.mask:  # about half the bins legal, the row's action among them
                W = max(1, B // 32)
                words = g.integers(0, 1 << min(B, 32), (total, W),
                                   dtype=np.uint64).astype(np.uint32)
                words[np.arange(total), action // 32] |= (
                    np.uint32(1) << (action % 32).astype(np.uint32))
                blocks["legal"] = dev(4 * total * W)
                put(blocks["legal"], words)
            if a.ent:
                blocks["v_old"] = dev(4 * total)
                blocks["ext_stats"] = dev(8 * _lib.VEXT_COUNT)
                put(blocks["v_old"],
                    g.standard_normal(total).astype(np.float32))
            put(blocks["p_old"],
                (g.random(total) * 0.5 + 0.01).astype(np.float32))
            put(blocks["adv"], g.standard_normal(total).astype(np.float32))
            put(blocks["target"], g.standard_normal(total).astype(np.float32))
            arms = [("venv_policy_loss", 0, 0),
                    ("venv_policy_loss +probs", 1, 0),
                    ("venv_policy_loss +stats", 0, 1),
                    ("venv_policy_loss +probs +stats", 1, 1),
                    ("venv_policy_loss run (no list)", 0, 0)]
            if a.kl:
                arms += [("venv_policy_loss kl", 0, 0),
                         ("venv_policy_loss kl +kl_stats", 0, 0),
                         ("venv_policy_loss clipped +kl_stats", 0, 0)]
            if a.mask:
                arms += [("venv_policy_loss masked", 0, 0),
                         ("venv_policy_loss masked +probs +stats", 1, 1),
                         ("venv_policy_loss masked run (no list)", 0, 0)]
            if a.ent:
                arms += [("venv_policy_loss ent", 0, 0),
                         ("venv_policy_loss ent +vclip", 0, 0),
                         ("venv_policy_loss ent +ext_stats", 0, 0),
                         # the same instantiation without the logarithms
                         ("venv_policy_loss ext_stats alone", 0, 0)]
            for name, probs, stats in arms:
                v = _lib.VenvLoss()
                v.policy, v.kind = blocks["z"], _lib.ACT_LOGITS
                v.loss = _lib.LOSS_CLIPPED
                # rows idx[j] of the 2 n (a shuffled minibatch), or rows 0 ..
                v.rows_dev = None if "run" in name else blocks["idx"]
                v.first, v.count, v.total = 0, n, total
                v.adv, v.action = blocks["adv"], blocks["action"]
                v.p_old, v.eps, v.scale = blocks["p_old"], 0.2, 1.0 / n
                v.values_new, v.target = blocks["values"], blocks["target"]
                v.value_scale, v.grad = 1.0, blocks["grad"]
                v.dvalue = blocks["dvalue"]
                v.probs_out = blocks["probs"] if probs else None
                v.stats = blocks["stats"] if stats else None
                gathers_q = "kl" in name
                if gathers_q:
                    v.distrib, v.beta = blocks["distrib"], 0.05
                    if " kl" in name:
                        v.loss = _lib.LOSS_KL_REGULATED
                    if "kl_stats" in name:
                        v.kl_stats = blocks["kl_stats"]

                masked = "masked" in name
                x = None
                if " ent" in name or "ext_stats" in name:
                    x = _lib.VenvLossExt()
                    x.ent_coef = 0.01 if " ent" in name else 0.0
                    if "vclip" in name:
                        x.v_old, x.vclip = blocks["v_old"], 0.2
                    if "ext_stats" in name:
                        x.ext_stats = blocks["ext_stats"]

                def launch():
                    if x is not None:
                        check(lib.xh_venv_policy_loss_ex(env.h, C.byref(v),
                                                         C.byref(x)))
                    elif masked:
                        check(lib.xh_venv_policy_loss_masked(
                            env.h, C.byref(v), blocks["legal"]))
                    else:
                        check(lib.xh_venv_policy_loss(env.h, C.byref(v)))
                for _ in range(a.warmup):
                    launch()
                env.synchronize()
                per = []
                for _ in range(a.reps):
                    env.set_timing(True)
                    for _ in range(a.launches):
                        launch()
                    ms, cnt = env.kernel_time()
                    env.set_timing(False)
                    assert cnt == a.launches, (cnt, a.launches)
                    per.append(ms / a.launches)
                med = float(np.median(per))
                nbytes = n * (8 * B + (4 * B if probs else 0) + 28
                              - (0 if v.rows_dev else 4)
                              + (4 * B if gathers_q else 0)
                              + (4 * max(1, B // 32) if masked else 0)
                              + (4 if "vclip" in name else 0))
                rows_out.append({"kernel": name, "rows": n, "bins": B,
                                 "bytes": nbytes, "ms": med,
                                 "ms_min": min(per), "ms_max": max(per),
                                 "tb_s": nbytes / med / 1e9})
                print("%-37s %8d rows B=%-3d %.4f ms [%.4f .. %.4f]  %6.1f MB"
                      "  %5.2f TB/s" % (name, n, B, med, min(per), max(per),
                                        nbytes / 1e6, nbytes / med / 1e9),
                      flush=True)
            env.synchronize()
            for p in blocks.values():
                check(_lib.tensor_free(ctx.h, p))
        env.close()
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows_out, f, indent=1)


if __name__ == "__main__":
    main()
