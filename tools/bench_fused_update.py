#!/usr/bin/env python3
"""Times the in-backward fused update (csr_fused_optimizer_apply) per method.

Shape: the DLRM-bs64k-shaped update of tools/pmc_bw.py (10M x 128 fp32 table,
1.7M hotness-1 ids, bf16 grads), with uniform and with power-law ids (hot
rows take the long-segment path).  Methods alternate inside every round so
that drift hits them alike; each figure is the median over rounds of the mean
call time, taken with device events.  One JSON line per (ids, method).

  python tools/bench_fused_update.py [--methods sgd adagrad rowwise_adagrad]
  python tools/bench_fused_update.py --ext OTHER/_hip_ops*.so --methods sgd adagrad

--ext times another build of the extension (e.g. the parent commit's) on the
same inputs.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

VOCAB, WIDTH, NNZ = 10_000_000, 128, 1_700_000
METHODS = ("sgd", "adagrad", "rowwise_adagrad")


def load_ext(path):
    if path is None:
        from distributed_embeddings_amd.ops import _backend
        return _backend.ops()
    spec = importlib.util.spec_from_file_location("_hip_ops", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def state_for(method):
    if method == "sgd":
        return torch.empty(0, device="cuda")
    shape = (VOCAB, WIDTH) if method == "adagrad" else (VOCAB,)
    return torch.zeros(shape, device="cuda")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", default=None)
    p.add_argument("--methods", nargs="+", default=list(METHODS),
                   choices=METHODS)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    ext = load_ext(args.ext)
    from distributed_embeddings_amd.utils.input_gen import power_law_ids

    torch.manual_seed(0)
    w = torch.randn(VOCAB, WIDTH, device="cuda")
    splits = torch.arange(NNZ + 1, device="cuda")
    grad = torch.randn(NNZ, WIDTH, device="cuda").bfloat16()
    lr = torch.tensor([1e-3], device="cuda")
    id_sets = {
        "uniform": torch.randint(0, VOCAB, (NNZ,), device="cuda"),
        "power_law": power_law_ids(VOCAB, (NNZ,), 1.05).cuda(),
    }
    states = {m: state_for(m) for m in args.methods}

    def call(method, ids):
        ext.csr_fused_optimizer_apply(w, states[method], ids, splits, grad, lr,
                                      False, method != "sgd", 1e-10)

    for name, ids in id_sets.items():
        for m in args.methods:
            for _ in range(3):
                call(m, ids)
        torch.cuda.synchronize()
        times = {m: [] for m in args.methods}
        for _ in range(args.rounds):
            for m in args.methods:
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call(m, ids)
                t1.record()
                t1.synchronize()
                times[m].append(t0.elapsed_time(t1) / args.iters * 1e3)
        for m in args.methods:
            print(json.dumps({
                "ext": args.ext or "in-tree", "ids": name, "method": m,
                "unique_ids": int(torch.unique(ids).numel()),
                "us_median": round(statistics.median(times[m]), 1),
                "us_min": round(min(times[m]), 1),
                "us_max": round(max(times[m]), 1),
                "state_bytes": states[m].numel() * 4,
            }), flush=True)


if __name__ == "__main__":
    main()
