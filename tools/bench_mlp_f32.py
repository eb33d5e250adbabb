#!/usr/bin/env python3
"""Times the fp32 MLP backward kernels against the plain fp32 torch ops.

  wgrad   gw = g^T x for the seven `Linear` + `ReLU` layers of the flagship
          DLRM (g [K, M], x [K, N]): `g.t().mm(x)` against `wgrad_splitk_f32`
  gemv    the logit layer (M = 1): `g.t().mm(x)` + `g.sum(0)` against
          `wgrad_gemv_f32`
  relu    `threshold_backward` + `sum(0)` against `relu_bwd_bias_grad_f32`

The TunableOp selections of `profiles/` are loaded as `bench.py` loads them.
The methods of one shape alternate inside every round so that drift hits them
alike; each figure is the median over rounds of the mean call time, taken
with device events, with the rounds' min and max.  Operand residency as in
`tools/bench_wgrad.py`: `same` calls one set of operands again and again,
`rotate` walks a pool larger than the 256 MiB Infinity Cache, so every call
reads from HBM.  One JSON line per (shape, mode, method).

  python tools/bench_mlp_f32.py
  python tools/bench_mlp_f32.py --wgrad 256x512 --splitk 0 16 32 --tile -1 1
  python tools/bench_mlp_f32.py --wgrad --relu --gemv 256 --k 8192 65536

--splitk / --tile time `wgrad_splitk_f32` with those settings too (0 / -1:
the plan's own), for choosing the plan.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch

from bench_wgrad import INFINITY_CACHE, SHAPES, enable_tunableop


def time_variants(variants, pool, rounds, iters):
    """variants: {name: fn(operands)}; {name: [us per call, one per round]}"""
    for fn in variants.values():
        for i in range(3):
            fn(pool[i % len(pool)])
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(iters):
                fn(pool[i % len(pool)])
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / iters * 1e3)
    return times


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--k", nargs="+", type=int, default=[65536])
    p.add_argument("--wgrad", nargs="*", default=None, metavar="MxN")
    p.add_argument("--gemv", nargs="*", type=int, default=None, metavar="N")
    p.add_argument("--relu", nargs="*", type=int, default=None, metavar="N")
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
    if args.wgrad is None and args.gemv is None and args.relu is None:
        args.wgrad, args.gemv, args.relu = [], [], []
    wgrad = [tuple(int(v) for v in s.split("x")) for s in args.wgrad or []] \
        or (list(dict.fromkeys(SHAPES)) if args.wgrad is not None else [])
    gemv = args.gemv or ([256] if args.gemv is not None else [])
    relu = args.relu or ([1024, 512] if args.relu is not None else [])
    torch.manual_seed(0)

    jobs = []  # (kind, shape name, operand widths, bytes moved, flops, plan, variants)
    for k in args.k:
        for m, n in wgrad:
            v = {"gemm": lambda o: o[0].t().mm(o[1])}
            for t in args.tile:
                if (t == 2) != (n <= 16) and t >= 0:
                    continue
                for s in args.splitk:
                    v[f"wgrad_splitk_f32 splitk={s} tile={t}"] = \
                        lambda o, s=s, t=t: ext.wgrad_splitk_f32(o[0], o[1], s, t)
            jobs.append(("wgrad", k, f"{m}x{n}", (m, n), k * (m + n) * 4,
                         2.0 * k * m * n, ext.wgrad_splitk_f32_plan(k, m, n), v))
        for n in gemv:
            v = {"gemm+sum": lambda o: (o[0].t().mm(o[1]), o[0].sum(0)),
                 "wgrad_gemv_f32": lambda o: ext.wgrad_gemv_f32(o[0], o[1])}
            jobs.append(("gemv", k, f"1x{n}", (1, n), k * (1 + n) * 4,
                         2.0 * k * n, ext.wgrad_gemv_f32_plan(k, n), v))
        for n in relu:
            def plain(o):
                g = torch.ops.aten.threshold_backward(o[0], o[1], 0)
                return g, g.sum(0)
            v = {"threshold_backward+sum": plain,
                 "relu_bwd_bias_grad_f32":
                     lambda o: ext.relu_bwd_bias_grad_f32(o[0], o[1])}
            # grad_out and y read, grad_in written
            jobs.append(("relu", k, f"{k}x{n}", (n, n), k * n * 12, 0.0, [], v))

    for kind, k, name, widths, nbytes, flops, plan, variants in jobs:
        set_bytes = k * sum(widths) * 4
        for mode in args.modes:
            nsets = 1 if mode == "same" else \
                max(2, -(-3 * INFINITY_CACHE // set_bytes))
            pool = [tuple(torch.randn(k, w, device="cuda") for w in widths)
                    for _ in range(nsets)]
            times = time_variants(variants, pool, args.rounds, args.iters)
            for method, ts in times.items():
                med = statistics.median(ts)
                print(json.dumps({
                    "kind": kind, "shape": name, "k": k, "mode": mode,
                    "sets": nsets, "method": method, "plan": list(plan),
                    "us_median": round(med, 1), "us_min": round(min(ts), 1),
                    "us_max": round(max(ts), 1),
                    "tb_s": round(nbytes / med / 1e6, 2),
                    "tflop_s": round(flops / med / 1e6, 1),
                    "tunableop": csvs,
                }), flush=True)
            del pool
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
