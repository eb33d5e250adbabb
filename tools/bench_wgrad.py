#!/usr/bin/env python3
"""Times the MLP weight gradient gw = g^T x: tuned GEMM against wgrad_splitk.

Shapes: the seven `_LinearReLU` layers of the flagship DLRM at batch 65536
(g [K, M], x [K, N], gw [M, N]).  The TunableOp selections of `profiles/` are
loaded as `bench.py` loads them, so `g.t().mm(x)` runs the tuned solution.
The two methods alternate inside every round so that drift hits them alike;
each figure is the median over rounds of the mean call time, taken with
device events, with the rounds' min and max.  Two operand-residency modes:

  same    one (g, x) pair, called again and again: what fits stays in the
          256 MiB Infinity Cache
  rotate  a pool of pairs larger than the Infinity Cache, one after another:
          every call reads its operands from HBM

One JSON line per (shape, mode, method).  `tb_s` counts the operand bytes
only (the slab is overhead), `tflop_s` the 2 K M N flops.

  python tools/bench_wgrad.py
  python tools/bench_wgrad.py --shapes 256x512 128x256 --splitk 8 16 32 --tile 0 1
  python tools/bench_wgrad.py --modes rotate --k 32768

--splitk / --tile time the kernel with those settings too (0 / -1: the
plan's own), for choosing the plan.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

# (M, N) = (out, in) features of the bottom and the top MLP
SHAPES = [(512, 13), (256, 512), (128, 256),
          (1024, 512), (1024, 1024), (512, 1024), (256, 512)]
INFINITY_CACHE = 256 << 20


def enable_tunableop():
    import torch.cuda.tunable as tunable
    base = os.path.join(ROOT, "profiles")
    csvs = [os.path.join(base, f) for f in
            ("tunableop_gfx950.csv", "tunableop_gfx950_bs64k.csv")]
    csvs = [c for c in csvs if os.path.exists(c)]
    if csvs:
        tunable.enable(True)
        tunable.tuning_enable(False)
        for c in csvs:
            tunable.read_file(c)
    return [os.path.basename(c) for c in csvs]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--k", type=int, default=65536)
    p.add_argument("--shapes", nargs="+", default=None, metavar="MxN")
    p.add_argument("--modes", nargs="+", default=["same", "rotate"],
                   choices=["same", "rotate"])
    p.add_argument("--splitk", nargs="+", type=int, default=[0])
    p.add_argument("--tile", nargs="+", type=int, default=[-1])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    csvs = enable_tunableop()

    shapes = SHAPES
    if args.shapes:
        shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes]
    k = args.k
    torch.manual_seed(0)
    done = set()
    for m, n in shapes:
        if (m, n) in done:
            continue
        done.add((m, n))
        pair_bytes = k * (m + n) * 2
        variants = [("gemm", 0, -1)]
        for t in args.tile:
            if t == 2 and n > 16 or t in (0, 1) and n % 8 != 0:
                continue
            for s in args.splitk:
                variants.append(("wgrad_splitk", s, t))
        plan = ext.wgrad_splitk_plan(k, m, n)
        for mode in args.modes:
            npairs = 1 if mode == "same" else \
                max(2, -(-3 * INFINITY_CACHE // pair_bytes))
            pool = [(torch.randn(k, m, device="cuda").bfloat16(),
                     torch.randn(k, n, device="cuda").bfloat16())
                    for _ in range(npairs)]

            def call(v, i):
                g, x = pool[i % npairs]
                if v[0] == "gemm":
                    return g.t().mm(x)
                return ext.wgrad_splitk(g, x, v[1], v[2])

            for v in variants:
                for i in range(3):
                    call(v, i)
            torch.cuda.synchronize()
            times = {v: [] for v in variants}
            for _ in range(args.rounds):
                for v in variants:
                    t0 = torch.cuda.Event(enable_timing=True)
                    t1 = torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for i in range(args.iters):
                        call(v, i)
                    t1.record()
                    t1.synchronize()
                    times[v].append(t0.elapsed_time(t1) / args.iters * 1e3)
            for v in variants:
                med = statistics.median(times[v])
                print(json.dumps({
                    "shape": f"{m}x{n}", "k": k, "mode": mode,
                    "pairs": npairs, "method": v[0], "splitk": v[1],
                    "tile": v[2], "plan": list(plan),
                    "us_median": round(med, 1),
                    "us_min": round(min(times[v]), 1),
                    "us_max": round(max(times[v]), 1),
                    "operand_mb": round(pair_bytes / 1e6, 1),
                    "tb_s": round(pair_bytes / med / 1e6, 2),
                    "tflop_s": round(2.0 * k * m * n / med / 1e6, 1),
                    "tunableop": csvs,
                }), flush=True)
            del pool
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
