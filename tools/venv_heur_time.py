#!/usr/bin/env python3
"""Kernel time of xh_venv_act_heuristic per kind, beside xh_venv_act(LOGITS,
ARGMAX) on a resident row and beside that act plus a score-row kernel of the
caller's (best-fit as a torch expression), at 64 bins, 2-D, with 32768 and
1,048,576 envs: ms per launch and the achieved GB/s over the algorithmic
bytes.

    python tools/venv_heur_time.py
    python tools/venv_heur_time.py --envs 32768 --bins 128 --dims 3
    python tools/venv_heur_time.py --no-torch       # without the score-row arm

Bytes per env step: the heuristic launch 2 B D + 13 (bins read
and written, item read and written, stream state read and written, action,
PCHOICE, reward, done); the act launch that plus its policy row, 4 B; the
caller's score kernel reads the bins and the item and writes the row, B D + 4
+ 4 B.  The venv launches are timed by xh_venv_kernel_time (HIP events around
each launch), the torch expression by torch events around the same number of
evaluations, in a child process of its own (torch brings its own HIP runtime)
that runs one repetition each time the parent asks; "act+scores" is the sum of
the two, which cannot be timed as one span.  Every arm runs --launches
launches per repetition and the arms alternate within each of the --reps
repetitions, on one device: median [min .. max] of the repetitions."""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("random", "firstfit", "bestfit", "minwaste")


def timed(env, launch, launches):
    env.set_timing(True)
    for _ in range(launches):
        launch()
    ms, n = env.kernel_time()
    env.set_timing(False)
    assert n == launches, (n, launches)
    return ms / n


def torch_child(N, B, D, launches, warmup):
    """The child process: a caller's best-fit score row as a torch expression
    on bins and items of the venv's shapes (int8 [N][B][D], int8 [N][4]; their
    values do not change its time), f32 [N][B] out.  One repetition per line
    read from stdin, its ms per evaluation printed."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(N)
    bins = torch.randint(0, 9, (N, B, D), device="cuda", generator=g,
                         dtype=torch.int8)
    item = torch.randint(1, 5, (N, 4), device="cuda", generator=g,
                         dtype=torch.int8)[:, :D].contiguous()
    out = torch.empty((N, B), dtype=torch.float32, device="cuda")
    minus = torch.tensor(-1.0, device="cuda")

    def evaluate():
        it = item[:, None, :]
        fits = (bins >= it).all(dim=-1)
        s = (it.float() / bins.float()).sum(dim=-1)
        torch.where(fits, s, minus, out=out)
    for _ in range(warmup):
        evaluate()
    torch.cuda.synchronize()
    print("ready", flush=True)
    for _ in sys.stdin:
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            evaluate()
        e1.record()
        e1.synchronize()
        print(e0.elapsed_time(e1) / launches, flush=True)


class TorchArm:
    """The child process of one N; rep() runs one repetition in it."""

    def __init__(self, N, B, D, launches, warmup):
        import subprocess
        self.p = subprocess.Popen(
            [sys.executable, os.path.abspath(__file__), "--torch-child",
             "--envs", str(N), "--bins", str(B), "--dims", str(D),
             "--launches", str(launches), "--warmup", str(warmup)],
            stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        line = self.p.stdout.readline().strip()
        if line != "ready":
            raise RuntimeError("the torch arm did not start: %r" % line)

    def rep(self):
        self.p.stdin.write("go\n")
        self.p.stdin.flush()
        return float(self.p.stdout.readline())

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=60)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--envs", type=int, nargs="+", default=[32768, 1048576])
    ap.add_argument("--bins", type=int, default=64)
    ap.add_argument("--dims", type=int, default=2)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true",
                    help="leave out the caller's score-row arm")
    ap.add_argument("--torch-child", action="store_true",
                    help=argparse.SUPPRESS)
    ap.add_argument("--json", help="also write the result rows to this file")
    a = ap.parse_args()
    if a.torch_child:
        return torch_child(a.envs[0], a.bins, a.dims, a.launches, a.warmup)
    sys.path.insert(0, REPO)

    from dependence_free_rl_amd import Context, VecEnv, _lib
    B, D = a.bins, a.dims
    ctx = Context(device=0)
    rows = []
    heur_bytes = 2 * B * D + 13
    act_bytes = heur_bytes + 4 * B
    score_bytes = B * D + 4 + 4 * B
    for N in a.envs:
        env = VecEnv(ctx, num_envs=N, bins=B, dims=D, rng_state=7,
                     policy_draws=2)
        g = np.random.default_rng(N)
        env.set(_lib.VENV_POLICY, g.random((N, B), dtype=np.float32))
        arms = {k: (lambda k=k: env.act_heuristic(k)) for k in KINDS}
        arms["act argmax"] = lambda: env.act(kind="logits", mode="argmax",
                                             fetch=False)
        evaluate = None
        if not a.no_torch:
            try:
                evaluate = TorchArm(N, B, D, a.launches, a.warmup)
            except RuntimeError as e:  # reported; the venv arms still run
                print("no score-row arm at %d envs: %s" % (N, e), flush=True)
        for launch in arms.values():
            for _ in range(a.warmup):
                launch()
        env.synchronize()
        per = {name: [] for name in arms}
        per_scores = []
        for _ in range(a.reps):  # the arms alternate within a repetition
            for name, launch in arms.items():
                per[name].append(timed(env, launch, a.launches))
            if evaluate:
                per_scores.append(evaluate.rep())
        if evaluate:
            evaluate.close()
            per["scores (torch)"] = per_scores
            per["act+scores"] = [x + y for x, y in zip(per["act argmax"],
                                                       per_scores)]
        nbytes = {"act argmax": act_bytes, "scores (torch)": score_bytes,
                  "act+scores": act_bytes + score_bytes}
        for name, ms in per.items():
            med = float(np.median(ms))
            nb = nbytes.get(name, heur_bytes)
            row = {"lib": _lib.LIB_PATH, "kernel": name, "envs": N, "bins": B,
                   "dims": D, "bytes_per_env": nb, "ms": med,
                   "ms_min": min(ms), "ms_max": max(ms),
                   "gb_s": N * nb / med / 1e6}
            rows.append(row)
            print("%-15s %8d envs  %.4f ms [%.4f .. %.4f]  %7.1f GB/s  (%d B "
                  "per env step)" % (name, N, med, min(ms), max(ms),
                                     row["gb_s"], nb), flush=True)
        env.close()
    ctx.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
