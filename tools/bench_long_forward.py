#!/usr/bin/env python3
"""Times the ragged forward (csr_lookup_forward) on bags of power-law length.

Shape: a 10M x 128 fp32 table and 16384 bags whose lengths follow a power law
(1 + power_law_ids(max_len), alpha 1.05: most bags hold a few ids, a few hold
thousands), uniform ids.  With 8192 row-waves the adaptive threshold applies,
so only the outliers -- more than four times the average length -- take the
long-row split.  Variants alternate inside every round; each figure is the
median over rounds of the mean call time, taken with device events.  One JSON
line per (out dtype, mode).

  python tools/bench_long_forward.py
  python tools/bench_long_forward.py --ext OTHER/_hip_ops*.so

--ext times another build of the extension (e.g. the parent commit's) on the
same inputs, in the default mode only.  This tree's build is timed with the
deterministic mode off and on: bf16 out with the mode off reduces every bag
in-register (the long split is disabled), with the mode on it splits the long
bags like fp32 out.
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

VOCAB, WIDTH, BAGS = 10_000_000, 128, 16384


def load_ext(path):
    if path is None:
        from distributed_embeddings_amd.ops import _backend
        return _backend.ops()
    spec = importlib.util.spec_from_file_location("_hip_ops", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", default=None)
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--max-len", type=int, default=20_000)
    args = p.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    ext = load_ext(args.ext)
    from distributed_embeddings_amd.utils.input_gen import power_law_ids

    g = torch.Generator().manual_seed(0)
    w = torch.randn(VOCAB, WIDTH, device="cuda")
    lengths = 1 + power_law_ids(args.max_len, (BAGS,), 1.05, generator=g)
    splits = torch.cat([torch.zeros(1, dtype=torch.long), lengths.cumsum(0)])
    nnz = int(splits[-1])
    ids = torch.randint(0, VOCAB, (nnz,), generator=g).cuda()
    splits = splits.cuda()
    thresh = min(max(4 * (nnz // BAGS), 128), 8192)

    modes = (False,) if args.ext else (False, True)
    variants = [(bf16, det) for bf16 in (False, True) for det in modes]

    def call(variant):
        bf16, det = variant
        # the default call is the parent commit's, argument for argument
        kw = {"deterministic": True} if det else {}
        ext.csr_lookup_forward(w, ids, splits, False, bf16, None, **kw)

    for v in variants:
        for _ in range(3):
            call(v)
    torch.cuda.synchronize()
    times = {v: [] for v in variants}
    for _ in range(args.rounds):
        for v in variants:
            t0 = torch.cuda.Event(enable_timing=True)
            t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.iters):
                call(v)
            t1.record()
            t1.synchronize()
            times[v].append(t0.elapsed_time(t1) / args.iters * 1e3)
    for v in variants:
        print(json.dumps({
            "ext": args.ext or "in-tree", "out": "bf16" if v[0] else "fp32",
            "deterministic": v[1], "bags": BAGS, "nnz": nnz,
            "max_len": int(lengths.max()),
            "bags_over_threshold": int((lengths > thresh).sum()),
            "threshold": thresh,
            "us_median": round(statistics.median(times[v]), 1),
            "us_min": round(min(times[v]), 1),
            "us_max": round(max(times[v]), 1),
            "slab_bytes": (nnz // 64 + 64) * WIDTH * 4 if v[1] else 0,
        }), flush=True)


if __name__ == "__main__":
    main()
