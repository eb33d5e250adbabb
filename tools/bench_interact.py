#!/usr/bin/env python3
"""Micro-benchmark: interaction kernels, old [B,F,D] vs packed layouts.

Shape: the DLRM-bs64k interaction (B = 65536, P = 26, D = 128, out_w = 512)
unless --features / --width say otherwise; out_w is tril + D padded
to a multiple of 64, as the DLRM model pads it.  Each figure is the median
over rounds of the mean call time, taken with device events.

  python tools/bench_interact.py
  python tools/bench_interact.py --ext OTHER/_hip_ops*.so
  DI_SWEEP=1 python tools/bench_interact.py     # DE_DI_WPB = 2, 4, 8 (F > 32: 1, 2, 4)
  python tools/bench_interact.py --only packed --rounds 1 --iters 3  # counter runs
  python tools/bench_interact.py --features 40 --only packed
  python tools/bench_interact.py --features 40 --only torch  # the torch fallback

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


def sweep_wpb(argv, values):
    env = dict(os.environ, _DI_WORKER="1")
    for w in values:
        e = dict(env, DE_DI_WPB=str(w))
        print(f"--- WPB={w} ---", flush=True)
        subprocess.run([sys.executable, __file__] + argv, env=e, check=True)


def torch_runs(packed, bottom, perm, gout, out_w, sm, tag, gb_fwd, gb_bwd):
    """The fallback of ops.dot_interact.dot_interact_packed, forward alone and
    backward alone (autograd over a graph built once)."""
    from distributed_embeddings_amd.ops import dot_interact as di

    def fwd(pk, bt):
        sel = pk.index_select(1, perm.long()) if sm else \
            pk.index_select(0, perm.long()).transpose(0, 1)
        feats = torch.cat([bt.unsqueeze(1), sel], dim=1)
        return di._torch_dot_interact(feats.contiguous(), out_w)

    pk = packed.clone().requires_grad_(True)
    bt = bottom.clone().requires_grad_(True)
    out = fwd(pk, bt)

    def fwd_only():
        with torch.no_grad():
            fwd(packed, bottom)

    return [
        (f"fwd  torch  {tag}", gb_fwd, fwd_only),
        (f"bwd  torch  {tag}", gb_bwd,
         lambda: torch.autograd.grad(out, (pk, bt), gout, retain_graph=True)),
    ]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--ext", default=None)
    p.add_argument("--only", choices=("all", "packed", "torch"), default="all",
                   help="torch: the ops' torch fallback on the packed input "
                        "(what shapes outside the kernels' cap run)")
    p.add_argument("--features", type=int, default=27,
                   help="F, counting the bottom-MLP output")
    p.add_argument("--width", type=int, default=128, help="D")
    p.add_argument("--sample-major", action="store_true",
                   help="packed block as [B, P, D] (the world==1 layout)")
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args()
    if "_DI_WORKER" not in os.environ and os.environ.get("DI_SWEEP") == "1":
        # the 64-row kernels (F > 32) hold 1, 2 or 4 samples per block
        sweep_wpb(sys.argv[1:], (1, 2, 4) if args.features > 32 else (2, 4, 8))
        return
    assert torch.cuda.is_available(), "needs a GPU: no timing without one"
    torch.manual_seed(0)
    B, F, D = 65536, args.features, args.width
    P = F - 1
    out_w = (F * P // 2 + D + 63) // 64 * 64
    # bytes the result needs: features (+ gout) read, out or gradients written
    gb_fwd = B * (F * D + out_w) * 2 / 1e9
    gb_bwd = B * (2 * F * D + out_w) * 2 / 1e9
    sm = args.sample_major
    packed = torch.randn((B, P, D) if sm else (P, B, D), device="cuda").bfloat16()
    bottom = torch.randn(B, D, device="cuda").bfloat16()
    perm = torch.arange(P, dtype=torch.int32, device="cuda")
    gout = torch.randn(B, out_w, device="cuda").bfloat16()
    tag = "samp-major" if sm else "feat-major"
    print(f"B={B} F={F} D={D} out_w={out_w}")
    if args.only == "torch":
        runs = torch_runs(packed, bottom, perm, gout, out_w, sm, tag,
                          gb_fwd, gb_bwd)
        print("ext: none (torch ops)")
    else:
        ext = load_ext(args.ext)
        runs = [
            (f"fwd  packed {tag}", gb_fwd,
             lambda: ext.dot_interact_fwd_packed(bottom, packed, perm, out_w, sm)),
            (f"bwd  packed {tag}", gb_bwd,
             lambda: ext.dot_interact_bwd_packed(gout, bottom, packed, perm, sm)),
        ]
        if args.only == "all":
            feats = torch.randn(B, F, D, device="cuda").bfloat16()
            runs = [
                ("fwd  old [B,F,D]      ", gb_fwd,
                 lambda: ext.dot_interact_fwd(feats, out_w)),
                ("bwd  old [B,F,D]      ", gb_bwd,
                 lambda: ext.dot_interact_bwd(gout, feats)),
            ] + runs
        print(f"ext: {args.ext or 'in-tree'}")
    for name, gbytes, fn in runs:
        med, lo, hi = timeit(fn, args.rounds, args.iters)
        print(f"{name} : {med:7.1f} us  (min {lo:.1f}, max {hi:.1f})  "
              f"{gbytes / med * 1e3:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    main()
