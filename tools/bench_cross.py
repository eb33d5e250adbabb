#!/usr/bin/env python3
"""Micro-benchmark: the low-rank cross interaction's fused backward.

Shape: DLRM-DCNv2 on Criteo (B = 65536, N = 27 * 128 = 3456, r = 512, L = 3)
under bf16 autocast unless --batch / --width / --rank / --layers say
otherwise.  Two things are timed, each as the median over rounds of the mean
call time, taken with device events:

* ``cross_bwd`` (csrc/mlp_ops.hip), first-layer form (init) and accumulating
  form, against the torch composition ``G*x0``, ``.sum(0)``, ``G*u``,
  ``acc.copy_`` / ``acc.add_``;
* ``LowRankCrossNet`` forward + backward, the whole-stack function against
  the plain composition under autograd (``DE_FUSED_CROSS=0``).

  python tools/bench_cross.py --only fused
  python tools/bench_cross.py --only torch

--only runs one variant per process; alternate the two to see the
process-to-process spread.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def timeit(fn, rounds, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(rounds):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / iters * 1e3)
    return statistics.median(times), min(times), max(times)


def report(name, gbytes, stats):
    med, lo, hi = stats
    rate = f"  {gbytes / med * 1e3:5.2f} TB/s" if gbytes else ""
    print(f"{name} : {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}){rate}",
          flush=True)


def bench_op(variant, B, N, rounds, iters):
    from distributed_embeddings_amd.ops import cross as cross_ops
    G, x0, u, acc = (torch.randn(B, N, device="cuda").bfloat16()
                     for _ in range(4))
    # bytes the result needs: G, x0, u (and acc) read, gu and acc written
    passes = {True: 5, False: 6}
    for init in (True, False):
        gb = passes[init] * B * N * 2 / 1e9
        if variant == "fused":
            assert cross_ops._bf16_2d_ok(G, x0, u, acc) and cross_ops._enabled()

        # the accumulating form adds a few hundred unit-variance terms over
        # the run: acc stays finite
        stats = timeit(lambda: cross_ops.cross_bwd(G, x0, u, acc, init),
                       rounds, iters)
        report(f"cross_bwd {variant:5s} init={int(init)}", gb, stats)


def bench_net(variant, B, N, r, layers, rounds, iters):
    from distributed_embeddings_amd.ops.cross import LowRankCrossNet
    net = LowRankCrossNet(N, num_layers=layers, low_rank=r).cuda()
    x0 = torch.randn(B, N, device="cuda").bfloat16().requires_grad_(True)
    gout = torch.randn(B, N, device="cuda").bfloat16()
    params = list(net.parameters())

    def fn():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x0)
        torch.autograd.grad(out, [x0] + params, gout)

    report(f"net fwd+bwd {variant:5s}      ", 0, timeit(fn, rounds, iters))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--only", choices=("all", "fused", "torch"), default="all")
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--width", type=int, default=3456, help="N")
    p.add_argument("--rank", type=int, default=512)
    p.add_argument("--layers", type=int, default=3)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    torch.manual_seed(0)
    print(f"B={args.batch} N={args.width} r={args.rank} L={args.layers}")
    variants = ("fused", "torch") if args.only == "all" else (args.only,)
    for variant in variants:
        os.environ["DE_FUSED_CROSS"] = "1" if variant == "fused" else "0"
        bench_op(variant, args.batch, args.width, args.rounds, args.iters)
        bench_net(variant, args.batch, args.width, args.rank, args.layers,
                  args.rounds, args.iters)


if __name__ == "__main__":
    main()
