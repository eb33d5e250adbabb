#!/usr/bin/env python3
"""Micro-benchmark: the synthetic models' fused concat + average pool.

Shape: the input list of a synthetic model (--model medium | large) at
B = 65536, bf16 inputs, fp32 numerical features, bf16 out, as
``SyntheticModel.forward`` under bf16 autocast hands them over.  Forward and
forward + backward are timed, each as the median over rounds of the mean call
time, taken with device events:

* ``fused``: ``concat_avg_pool`` on the HIP kernels (csrc/concat_pool.hip);
* ``torch``: the lines the model runs with ``DE_FUSED_POOL=0``: ``cat``,
  ``AvgPool1d(ceil_mode=True)``, ``cat`` with the fp32 numerical features
  and the MLP's cast of the promoted row back to bf16.

The rate is bytes needed / time: the inputs read and the output written for
the forward, plus the output's gradient read and the inputs' gradients
written for forward + backward.

  python tools/bench_concat_pool.py --only fused
  python tools/bench_concat_pool.py --only torch

--only runs one variant per process; alternate the two to see the
process-to-process spread.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from bench_cross import report, timeit


def model_widths(name):
    from distributed_embeddings_amd.models.config import synthetic_models
    from distributed_embeddings_amd.models.synthetic import expand_tables
    cfg = synthetic_models[name]
    tables, input_map, _ = expand_tables(cfg)
    return ([tables[t][1] for t in input_map], cfg.num_numerical_features,
            cfg.interact_stride)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--only", choices=("all", "fused", "torch"), default="all")
    p.add_argument("--model", choices=("medium", "large"), default="medium")
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=10)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    torch.manual_seed(0)

    from distributed_embeddings_amd.ops import concat_pool
    widths, nn_cols, stride = model_widths(args.model)
    B, W = args.batch, sum(widths)
    out_w = -(-W // stride) + nn_cols
    print(f"{args.model}: B={B} inputs={len(widths)} W={W} S={stride} "
          f"out={out_w}")
    inputs = [torch.randn(B, w, device="cuda").bfloat16().requires_grad_()
              for w in widths]
    num = torch.rand(B, nn_cols, device="cuda")
    gout = torch.randn(B, out_w, device="cuda").bfloat16()
    pool = torch.nn.AvgPool1d(stride, stride=stride, ceil_mode=True)
    fwd_gb = (B * W * 2 + B * nn_cols * 4 + B * out_w * 2) / 1e9
    both_gb = fwd_gb + (B * out_w * 2 + B * W * 2) / 1e9

    def fused():
        return concat_pool.concat_avg_pool(inputs, num, stride,
                                           out_dtype=torch.bfloat16)

    def composition():
        x = pool(torch.cat(inputs, dim=1).unsqueeze(1)).squeeze(1)
        return torch.cat([x, num], dim=1).to(torch.bfloat16)

    variants = ("fused", "torch") if args.only == "all" else (args.only,)
    for variant in variants:
        if variant == "fused":
            assert concat_pool.fused_ok(inputs, num, stride, torch.bfloat16)
        fn = fused if variant == "fused" else composition
        with torch.no_grad():
            report(f"fwd     {variant:5s}", fwd_gb,
                   timeit(fn, args.rounds, args.iters))
        report(f"fwd+bwd {variant:5s}", both_gb,
               timeit(lambda: torch.autograd.grad(fn(), inputs, gout),
                      args.rounds, args.iters))


if __name__ == "__main__":
    main()
