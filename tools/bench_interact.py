#!/usr/bin/env python3
"""Micro-benchmark: interaction kernels, old [B,F,D] vs packed layouts.

Shape: the DLRM-bs64k interaction (B = 65536, P = 26, D = 128, out_w = 512).
Each figure is the median over rounds of the mean call time, taken with
device events.

  python tools/bench_interact.py
  python tools/bench_interact.py --ext OTHER/_hip_ops*.so
  DI_SWEEP=1 python tools/bench_interact.py     # DE_DI_WPB = 2, 4, 8
  python tools/bench_interact.py --only packed --rounds 1 --iters 3  # counter runs

--ext times another build of the extension (e.g. the parent commit's) on the
same inputs; run the two builds in alternating processes.
"""
import argparse
import importlib.util
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def load_ext(path):
    if path is None:
        from distributed_embeddings_amd.ops import _backend
        return _backend.ops()
    spec = importlib.util.spec_from_file_location("_hip_ops", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


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


def sweep_wpb(argv):
    env = dict(os.environ, _DI_WORKER="1")
    for w in (2, 4, 8):
        e = dict(env, DE_DI_WPB=str(w))
        print(f"--- WPB={w} ---", flush=True)
        subprocess.run([sys.executable, __file__] + argv, env=e, check=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", default=None)
    p.add_argument("--only", choices=("all", "packed"), default="all")
    p.add_argument("--sample-major", action="store_true",
                   help="packed block as [B, P, D] (the world==1 layout)")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    if "_DI_WORKER" not in os.environ and os.environ.get("DI_SWEEP") == "1":
        sweep_wpb(sys.argv[1:])
        return
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    ext = load_ext(args.ext)
    torch.manual_seed(0)
    B, P, D = 65536, 26, 128
    F = P + 1
    out_w = 512
    sm = args.sample_major
    packed = torch.randn((B, P, D) if sm else (P, B, D), device="cuda").bfloat16()
    bottom = torch.randn(B, D, device="cuda").bfloat16()
    perm = torch.arange(P, dtype=torch.int32, device="cuda")
    gout = torch.randn(B, out_w, device="cuda").bfloat16()
    tag = "samp-major" if sm else "feat-major"
    runs = [
        (f"fwd  packed {tag}", 0.52,
         lambda: ext.dot_interact_fwd_packed(bottom, packed, perm, out_w, sm)),
        (f"bwd  packed {tag}", 0.97,
         lambda: ext.dot_interact_bwd_packed(gout, bottom, packed, perm, sm)),
    ]
    if args.only == "all":
        feats = torch.randn(B, F, D, device="cuda").bfloat16()
        runs = [
            ("fwd  old [B,F,D]      ", 0.52,
             lambda: ext.dot_interact_fwd(feats, out_w)),
            ("bwd  old [B,F,D]      ", 0.97,
             lambda: ext.dot_interact_bwd(gout, feats)),
        ] + runs
    print(f"ext: {args.ext or 'in-tree'}")
    for name, gbytes, fn in runs:
        med, lo, hi = timeit(fn, args.rounds, args.iters)
        print(f"{name} : {med:7.1f} us  (min {lo:.1f}, max {hi:.1f})  "
              f"{gbytes / med * 1e3:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
