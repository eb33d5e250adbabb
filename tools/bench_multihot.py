#!/usr/bin/env python3
"""Measures the multi-hot id plumbing on one GPU (results: profiles/multihot.md).

Part 1, the id vector of one fused group: the ``pack_ids`` kernel against the
torch composition it replaces (``torch.cat`` + cached offset vector add, with
``multi_hot_expand`` per input in front when bags are expanded), for 26
inputs at the batch size given:

  one-hot        hotness 1 everywhere (the flagship Criteo shape), copy
  one-hot-views  the same, the inputs adjacent views of one flat tensor (as
                 bench.py passes them): the composition's cat is then free
  mlperf-copy    MLPERF_MULTI_HOT_SIZES (214 ids per sample), [b, h] inputs
  mlperf-expand  the same bags expanded from one-hot ids

Part 2, the train step of DLRM (bf16 autocast, fused SGD on the tables, dense
SGD), eager and hipGraph-captured, with ``DE_PACK_IDS`` 1 and 0 (0 is the
code path from before the kernel):

  one-hot        interaction dot, the flagship
  expand         interaction cross, multi-hot, one-hot ids expanded on device
  data           the same model fed the same bags as [b, h] inputs

Every figure is a device-event time over ``--iters`` calls, taken
``--repeats`` times with the variants alternating; median, min and max of the
repeats are printed, one JSON line per figure.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

import distributed_embeddings_amd as de
from distributed_embeddings_amd.models.config import (CRITEO_1TB_TABLE_SIZES,
                                                      MLPERF_MULTI_HOT_SIZES)
from distributed_embeddings_amd.models.dlrm import DLRM
from distributed_embeddings_amd.ops.embedding_lookup import (
    multi_hot_expand_keyed, multi_hot_key, pack_ids)
from distributed_embeddings_amd.parallel.dist_embedding import _cat_or_view
from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer
from distributed_embeddings_amd.utils.input_gen import make_batch

SEED = 1234


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=65536)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--train-iters", type=int, default=20)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--table-size-cap", type=int, default=None,
                   help="cap the Criteo vocabularies (smaller tables)")
    p.add_argument("--embedding-dim", type=int, default=128)
    p.add_argument("--skip-kernel", action="store_true")
    p.add_argument("--skip-train", action="store_true")
    return p.parse_args()


def time_ms(fn, iters):
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def compare(name, variants, iters, repeats, extra=None):
    """Alternates the variants; prints one JSON line each."""
    for fn in variants.values():        # warm every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(time_ms(fn, iters))
    for k, ts in times.items():
        print(json.dumps(dict(extra or {}, what=name, variant=k,
                              median_ms=round(statistics.median(ts), 4),
                              min_ms=round(min(ts), 4),
                              max_ms=round(max(ts), 4), repeats=repeats,
                              iters=iters)), flush=True)


# ------------------------------------------------------------------ part 1

def kernel_part(args, sizes):
    b = args.batch
    g = torch.Generator().manual_seed(SEED)
    one_hot = [x.cuda() for x in make_batch(sizes, [1] * len(sizes), b,
                                            generator=g)]
    offsets, pos = [], 0
    for s in sizes:
        offsets.append(pos)
        pos += s
    specs = [(s, multi_hot_key(SEED, f)) for f, s in enumerate(sizes)]
    hot = MLPERF_MULTI_HOT_SIZES
    bags = [multi_hot_expand_keyed(x, s, h, k).contiguous()
            for x, h, (s, k) in zip(one_hot, hot, specs)]

    def offset_vector(counts):
        return torch.cat([torch.full((n,), off, dtype=torch.long, device="cuda")
                          for off, n in zip(offsets, counts)])

    views = list(torch.split(torch.cat(one_hot), b))
    shapes = {
        "one-hot": ([(x, 1, None, off) for x, off in zip(one_hot, offsets)],
                    offset_vector([b] * len(sizes)), False),
        "one-hot-views": ([(x, 1, None, off) for x, off in zip(views, offsets)],
                          offset_vector([b] * len(sizes)), False),
        "mlperf-copy": ([(x, 1, None, off) for x, off in zip(bags, offsets)],
                        offset_vector([b * h for h in hot]), False),
        "mlperf-expand": ([(x, h, spec, off) for x, h, spec, off
                           in zip(one_hot, hot, specs, offsets)],
                          offset_vector([b * h for h in hot]), True),
    }
    for name, (segs, off_vec, expand) in shapes.items():
        def composition(segs=segs, off_vec=off_vec, expand=expand):
            parts = [multi_hot_expand_keyed(x, e[0], h, e[1]) if expand else x
                     for x, h, e, _ in segs]
            return _cat_or_view(parts) + off_vec

        def kernel(segs=segs):
            return pack_ids([(x.reshape(-1), h, e, off)
                             for x, h, e, off in segs])

        assert torch.equal(kernel(), composition()), name
        n = off_vec.numel()
        compare("pack_ids", {"kernel": kernel, "composition": composition},
                args.iters, args.repeats,
                dict(shape=name, batch=b, ids=n,
                     out_mbytes=round(n * 8 / 1e6, 1)))


# ------------------------------------------------------------------ part 2

def train_part(args, sizes):
    b = args.batch
    g = torch.Generator().manual_seed(SEED + 1)
    one_hot = make_batch(sizes, [1] * len(sizes), b, generator=g)
    num = torch.rand(b, 13, generator=g).cuda()
    labels = torch.randint(0, 2, (b, 1), generator=g).float().cuda()
    hot = MLPERF_MULTI_HOT_SIZES
    bags = [de.multi_hot_expand(x, s, h, SEED, f).cuda()
            for f, (x, s, h) in enumerate(zip(one_hot, sizes, hot))]
    # adjacent views of one flat tensor, as bench.py passes its inputs
    one_hot = list(torch.split(torch.cat(one_hot).cuda(), b))
    loss_sum = torch.nn.BCEWithLogitsLoss(reduction="sum")

    for name, interaction, multi_hot, cats in (
            ("one-hot", "dot", None, one_hot),
            ("expand", "cross", hot, one_hot),
            ("data", "cross", hot, bags)):
        torch.manual_seed(SEED)
        with torch.device("cuda"):
            model = DLRM(sizes, embedding_dim=args.embedding_dim,
                         interaction=interaction, multi_hot_sizes=multi_hot,
                         multi_hot_seed=SEED)
        model.embeddings.enable_fused_sgd(1e-3)
        opt = SparseEmbeddingOptimizer(model.parameters(), lr=1e-3,
                                       method="sgd")

        def step():
            opt.zero_grad(set_to_none=False)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = model(num, cats)
                loss = loss_sum(logits.float(), labels) / b
            loss.backward()
            opt.step()
            return loss

        def with_env(value, fn):
            def run():
                os.environ["DE_PACK_IDS"] = value
                return fn()
            return run

        for _ in range(3):
            step()
        torch.cuda.synchronize()
        variants = {"eager DE_PACK_IDS=1": with_env("1", step),
                    "eager DE_PACK_IDS=0": with_env("0", step)}
        graphs = {}
        for value in ("1", "0"):
            os.environ["DE_PACK_IDS"] = value
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            graphs[value] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[value]):
                step()
            variants[f"graph DE_PACK_IDS={value}"] = graphs[value].replay
        compare("train step", variants, args.train_iters, args.repeats,
                dict(model=name, interaction=interaction, batch=b,
                     ids_per_sample=sum(multi_hot) if multi_hot else len(sizes),
                     table_size_cap=args.table_size_cap))
        os.environ.pop("DE_PACK_IDS", None)
        del graphs, variants, model, opt
        torch.cuda.empty_cache()


def main():
    args = parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_multihot.py measures on a GPU; none is visible")
    sizes = list(CRITEO_1TB_TABLE_SIZES)
    if args.table_size_cap:
        sizes = [min(s, args.table_size_cap) for s in sizes]
    if not args.skip_kernel:
        kernel_part(args, sizes)
    if not args.skip_train:
        train_part(args, sizes)


if __name__ == "__main__":
    main()
