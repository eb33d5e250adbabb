#!/usr/bin/env python3
"""Times the in-backward fused update (csr_fused_optimizer_apply) per method.

Shape: the DLRM-bs64k-shaped update of tools/pmc_bw.py (10M x 128 table, fp32
or with --table-dtype bf16, 1.7M hotness-1 ids, bf16 grads), with uniform and
with power-law ids (hot rows take the long-segment path).  Methods alternate
inside every round so that drift hits them alike; each figure is the median
over rounds of the mean call time, taken with device events.  One JSON line
per (ids, method, rounding).

  python tools/bench_fused_update.py [--methods sgd adagrad rowwise_adagrad]
  python tools/bench_fused_update.py --methods adagrad lazy_adam
  python tools/bench_fused_update.py --ext OTHER/_hip_ops*.so --methods sgd adagrad
  python tools/bench_fused_update.py --table-dtype bf16 --stochastic-rounding
  python tools/bench_fused_update.py --deterministic --id-sets power_law all_equal

--ext times another build of the extension (e.g. the parent commit's) on the
same inputs.  --stochastic-rounding (bf16 tables) times every method twice,
with nearest-even and with stochastic rounding, the two alternating inside
every round like the methods.  lazy_adam needs this tree's build: its state
is the [2, VOCAB, WIDTH] moments (10 GB) and it counts its steps in a device
tensor.

--deterministic times this tree's build in deterministic mode (long segments
through the slab and the fixed-order combine, no float atomics); the line then
carries the slab's size.  --id-sets picks the id distributions: besides the
two defaults, tiny_vocab (8192 ids over a vocabulary of 3) and all_equal (all
1.7M ids the same), the extremes of the long-segment path.
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
METHODS = ("sgd", "adagrad", "rowwise_adagrad", "lazy_adam")
ID_SETS = ("uniform", "power_law", "tiny_vocab", "all_equal")


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
    if method == "lazy_adam":
        return torch.zeros(2, VOCAB, WIDTH, device="cuda")
    shape = (VOCAB, WIDTH) if method == "adagrad" else (VOCAB,)
    return torch.zeros(shape, device="cuda")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", default=None)
    p.add_argument("--methods", nargs="+", default=list(METHODS),
                   choices=METHODS)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--table-dtype", choices=("fp32", "bf16"), default="fp32")
    p.add_argument("--stochastic-rounding", action="store_true",
                   help="also time stochastic rounding (needs bf16 tables)")
    p.add_argument("--deterministic", action="store_true",
                   help="time the deterministic mode (this tree's build only)")
    p.add_argument("--id-sets", nargs="+", default=["uniform", "power_law"],
                   choices=ID_SETS)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    if args.stochastic_rounding and args.table_dtype != "bf16":
        p.error("--stochastic-rounding needs --table-dtype bf16")
    if args.deterministic and args.ext:
        p.error("--deterministic times this tree's build, not --ext")
    ext = load_ext(args.ext)
    from distributed_embeddings_amd.utils.input_gen import power_law_ids

    torch.manual_seed(0)
    w = torch.randn(VOCAB, WIDTH, device="cuda")
    if args.table_dtype == "bf16":
        w = w.bfloat16()
    all_splits = torch.arange(NNZ + 1, device="cuda")
    all_grad = torch.randn(NNZ, WIDTH, device="cuda").bfloat16()
    lr = torch.tensor([1e-3], device="cuda")
    make_ids = {
        "uniform": lambda: torch.randint(0, VOCAB, (NNZ,), device="cuda"),
        "power_law": lambda: power_law_ids(VOCAB, (NNZ,), 1.05).cuda(),
        "tiny_vocab": lambda: torch.randint(0, 3, (8192,), device="cuda"),
        "all_equal": lambda: torch.full((NNZ,), 12345, device="cuda"),
    }
    id_sets = {name: make_ids[name]() for name in args.id_sets}
    # the parent commit's call, argument for argument, unless asked otherwise
    det = {"deterministic": True} if args.deterministic else {}
    states = {m: state_for(m) for m in args.methods}
    sr = torch.tensor([1234, 0], device="cuda")  # {seed, step}
    adam_step = torch.zeros(1, dtype=torch.int64, device="cuda")
    roundings = ("rne", "sr") if args.stochastic_rounding else ("rne",)
    variants = [(m, r) for m in args.methods for r in roundings]

    def call(variant, ids):
        method, rounding = variant
        n = ids.numel()
        splits, grad = all_splits[:n + 1], all_grad[:n]
        # the nearest-even call is the parent commit's, argument for argument
        extra = (None, sr) if rounding == "sr" else ()
        if method == "lazy_adam":
            ext.csr_fused_optimizer_apply(w, states[method], ids, splits, grad,
                                          lr, False, False, 1e-8, *extra,
                                          adam_step=adam_step, **det)
            return
        ext.csr_fused_optimizer_apply(w, states[method], ids, splits, grad, lr,
                                      False, method != "sgd", 1e-10, *extra,
                                      **det)

    for name, ids in id_sets.items():
        for v in variants:
            for _ in range(3):
                call(v, ids)
        torch.cuda.synchronize()
        times = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                t0 = torch.cuda.Event(enable_timing=True)
                t1 = torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    call(v, ids)
                t1.record()
                t1.synchronize()
                times[v].append(t0.elapsed_time(t1) / args.iters * 1e3)
        for v in variants:
            print(json.dumps({
                "ext": args.ext or "in-tree", "ids": name, "method": v[0],
                "table_dtype": args.table_dtype, "rounding": v[1],
                "unique_ids": int(torch.unique(ids).numel()),
                "us_median": round(statistics.median(times[v]), 1),
                "us_min": round(min(times[v]), 1),
                "us_max": round(max(times[v]), 1),
                "state_bytes": states[v[0]].numel() * 4,
                "deterministic": args.deterministic,
                "slab_bytes": ((ids.numel() // 64 + 64) * WIDTH * 4
                               if args.deterministic else 0),
            }), flush=True)


if __name__ == "__main__":
    main()
