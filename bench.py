#!/usr/bin/env python3
"""Flagship benchmark: DLRM / Criteo-1TB config, hybrid data+model parallel.

Driver contract: `python bench.py --gpus N --steps K --warmup W` runs one
training step per iteration (forward + BCE loss + backward + optimizer step)
on synthetic power-law categorical inputs of the BASELINE.json config
(DLRM Criteo, batch 65536 per GPU — at N=1 this IS the reference's global
bs=64k config; weak scaling as N grows), random-init weights, and prints ONE
JSON line from rank 0.

Launch for N>1: torchrun --nnodes=1 --nproc-per-node N bench.py --gpus N ...
(reads RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the env; RCCL backend).

A plain run only sets up, warms up, times the K steps and prints the result
line.  `--dump-outputs DIR` additionally writes what the last timed step
computed (see dump_outputs) so two builds can be compared output for output;
the inputs depend only on the arguments.  `--full` is where any measurement
beyond the headline figure belongs; there is none today, so it adds nothing.
"""

import argparse
import json
import os
import time

import numpy as np
import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-per-gpu", type=int, default=65536)
    p.add_argument("--model", type=str, default="dlrm-criteo",
                   choices=["dlrm-criteo", "synthetic-tiny", "synthetic-small",
                            "synthetic-medium", "synthetic-large"])
    p.add_argument("--alpha", type=float, default=1.05, help="power-law skew")
    p.add_argument("--pool", type=int, default=8, help="pre-generated batch pool size")
    p.add_argument("--strategy", type=str, default="memory_balanced")
    p.add_argument("--dtype", type=str, default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--table-dtype", type=str, default="fp32",
                   choices=["fp32", "bf16"],
                   help="embedding table storage dtype (fp32 accumulate both)")
    p.add_argument("--fused-sgd", dest="fused_sgd", action="store_true", default=True)
    p.add_argument("--no-fused-sgd", dest="fused_sgd", action="store_false")
    p.add_argument("--graph", dest="graph", action="store_true", default=True,
                   help="capture the train step in a hipGraph (world==1; "
                        "falls back to eager if capture fails)")
    p.add_argument("--no-graph", dest="graph", action="store_false")
    p.add_argument("--table-size-cap", type=int, default=None,
                   help="cap vocab sizes (CPU smoke only — a capped run is "
                        "NOT a valid benchmark measurement)")
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps write the last step's outputs "
                        "(loss, logits, updated parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true", default=False,
                   help="also run the measurements beyond the headline figure "
                        "(none today: a plain run already does only that)")
    return p.parse_args()


def setup_dist(args):
    import torch.distributed as dist
    have_gpu = torch.cuda.is_available()
    if "RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        rank = int(os.environ["RANK"])
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
        if have_gpu:
            torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl" if have_gpu else "gloo")
        return rank, dist.get_world_size(), local_rank
    if have_gpu:
        torch.cuda.set_device(0)
    return 0, 1, 0


def build_model(args, device):
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.models.config import CRITEO_1TB_TABLE_SIZES, synthetic_models
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.models.synthetic import SyntheticModel, expand_tables

    if args.model == "dlrm-criteo":
        tdt = torch.bfloat16 if args.table_dtype == "bf16" else torch.float32
        sizes = CRITEO_1TB_TABLE_SIZES
        if args.table_size_cap:  # CPU smoke only; never a valid measurement
            sizes = [min(s, args.table_size_cap) for s in sizes]
        with device:  # construct tables directly in HBM (96 GB fp32 / 48 GB bf16)
            model = DLRM(sizes, embedding_dim=128,
                         strategy=args.strategy, table_dtype=tdt)
        table_sizes = sizes
        hotness = [1] * len(table_sizes)
        num_numerical = 13
        name = "DLRM-Criteo-1TB"
    else:
        cfg = synthetic_models[args.model.split("-", 1)[1]]
        with device:
            model = SyntheticModel(cfg, strategy=args.strategy)
        tables, input_map, hotness = expand_tables(cfg)
        table_sizes = [tables[t][0] for t in input_map]
        num_numerical = cfg.num_numerical_features
        name = f"synthetic-{cfg.name}"
    keep_hot = args.model != "dlrm-criteo"
    return model, table_sizes, hotness, num_numerical, name, keep_hot


def maybe_enable_tunableop():
    """Load pre-tuned hipBLASLt GEMM algorithm selections (read-only).

    profiles/tunableop_gfx950.csv was produced by a PYTORCH_TUNABLEOP_TUNING=1
    run of this bench on an MI355X; validators (torch/hipblaslt versions) are
    checked by TunableOp itself — on mismatch it silently falls back to
    default algorithm selection.
    """
    try:
        import torch.cuda.tunable as tunable
        if os.environ.get("PYTORCH_TUNABLEOP_TUNING") == "1":
            return  # tuning run: TunableOp env config drives everything
        base = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles")
        csvs = [os.path.join(base, f) for f in
                ("tunableop_gfx950.csv", "tunableop_gfx950_bs64k.csv")]
        csvs = [c for c in csvs if os.path.exists(c)]
        if csvs and torch.cuda.is_available():
            tunable.enable(True)
            tunable.tuning_enable(False)
            for c in csvs:
                tunable.read_file(c)
    except Exception as e:
        print(f"# tunableop unavailable: {e}")


DUMP_FULL_PARAM_ELEMS = 4 * 1024 * 1024   # larger parameters are sampled
DUMP_SAMPLE_ROWS = 2048                   # seeded row sample of a large one
DUMP_TOUCHED_ROWS = 256                   # per table, rows the last step hit
DUMP_MAX_BYTES = 64 * 1024 * 1024


def dump_outputs(out_dir, model, loss, logits, cats, rank, world):
    """Writes what the last timed step handed back as ``<name>.npy`` (fp32).

    A caller of the train step receives the loss, the logits and the updated
    parameters.  Small parameters are written whole.  A parameter above
    DUMP_FULL_PARAM_ELEMS (the fused embedding variables, tens of GB) is
    written as a fixed seeded sample of DUMP_SAMPLE_ROWS rows, and for every
    table inside a fused variable the rows looked up by the first
    DUMP_TOUCHED_ROWS samples of the last batch are written too, so the
    sparse update of that very step is covered.  ``cats`` is that batch.
    """
    arrays = {"loss": loss.detach().reshape(1), "logits": logits.detach()}
    for pname, prm in model.named_parameters():
        w = prm.detach()
        if w.numel() <= DUMP_FULL_PARAM_ELEMS:
            arrays[f"param.{pname}"] = w
            continue
        w2 = w.reshape(w.shape[0], -1)
        g = torch.Generator(device="cpu").manual_seed(4321)
        rows = torch.randint(0, w2.shape[0], (DUMP_SAMPLE_ROWS,), generator=g)
        arrays[f"param_sample.{pname}"] = w2[rows.sort().values.to(w.device)]
    emb = getattr(model, "embeddings", None)
    # only where feature i reads table i (DLRM: no shared tables)
    if emb is not None and world == 1 and \
            list(emb.strategy.input_table_map) == list(range(len(cats))):
        groups = emb.strategy.local_concat_groups(rank)
        for grp, lyr in zip(groups, emb.col_layers):
            for m in grp.members:
                ids = cats[m.table_id].reshape(-1)[:DUMP_TOUCHED_ROWS]
                ids = ids.to(lyr.weight.device) + m.concat_row_offset
                arrays[f"emb_rows.table{m.table_id:02d}"] = lyr.weight.detach()[ids]
    prefix = "" if world == 1 else f"rank{rank}."
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        a = t.float().cpu().numpy().astype(np.float32, copy=False)
        total += a.nbytes
        assert total <= DUMP_MAX_BYTES, f"dump exceeds {DUMP_MAX_BYTES} bytes at {name}"
        np.save(os.path.join(out_dir, f"{prefix}{name}.npy"), a)


def main():
    args = parse_args()
    rank, world, local_rank = setup_dist(args)
    maybe_enable_tunableop()
    device = torch.device("cuda", local_rank) if torch.cuda.is_available() \
        else torch.device("cpu")
    torch.manual_seed(1234 + rank)

    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.utils.input_gen import make_batch

    model, table_sizes, hotness, num_numerical, name, keep_hot = build_model(args, device)
    b = args.batch_per_gpu

    # pre-generated input pool (parity: reference InputGenerator batch pool).
    # cats stored as ONE flat tensor per entry so graph replay needs a single
    # H2H copy; per-feature views are carved out once.
    pool = []
    cat_sizes = None
    for i in range(args.pool):
        g = torch.Generator(device="cpu").manual_seed(1000 + 131 * rank + i)
        cats = [c.to(device) for c in
                make_batch(table_sizes, hotness, b, args.alpha, generator=g,
                           keep_hot_dim=keep_hot)]
        if cat_sizes is None:
            cat_shapes = [c.shape for c in cats]
            cat_sizes = [c.numel() for c in cats]
        flat = torch.cat([c.reshape(-1) for c in cats])
        # dense inputs and labels come from the same per-entry CPU generator,
        # so the inputs depend on the arguments alone (not on how many device
        # random numbers the model's initialisation consumed)
        num = torch.rand(b, num_numerical, generator=g).to(device)
        labels = torch.randint(0, 2, (b, 1), generator=g).float().to(device)
        pool.append((num, flat, labels))

    def carve(flat):
        return [p.view(shape) for p, shape in
                zip(torch.split(flat, cat_sizes), cat_shapes)]

    from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer
    opt = de.DistributedOptimizer(
        SparseEmbeddingOptimizer(model.parameters(), lr=1e-3, method="sgd"),
        average=False)  # loss is normalized by the global batch below
    if args.fused_sgd and hasattr(model, "embeddings"):
        # in-backward fused SGD for the model-parallel tables (same SGD math,
        # applied during backward; optimizer still updates the dense params)
        model.embeddings.enable_fused_sgd(1e-3)
    de.broadcast_parameters(model)
    # per-rank loss normalized by the GLOBAL batch: mp tables get exact
    # global-batch grads, dp params sum to the same (see allreduce_gradients)
    _loss_sum = torch.nn.BCEWithLogitsLoss(reduction="sum")
    global_batch_ = b * world
    loss_fn = lambda logits, labels: _loss_sum(logits, labels) / global_batch_
    use_bf16 = args.dtype == "bf16" and torch.cuda.is_available()

    def run_fwd_bwd_opt(num, cats, labels, set_to_none=True):
        opt.zero_grad(set_to_none=set_to_none)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=use_bf16):
            logits = model(num, cats)
            loss = loss_fn(logits.float(), labels)
        loss.backward()
        opt.step()
        return loss, logits

    graph = None
    graph_ok = torch.cuda.is_available() and (
        world == 1 or os.environ.get("DE_DIST_GRAPH") == "1")
    if args.graph and graph_ok:
        # hipGraph capture: static input buffers (one flat cat copy per step),
        # grads pre-materialized, fused SGD has no host syncs.
        s_num, s_flat, s_labels = (t.clone() for t in pool[0])
        s_cats = carve(s_flat)
        try:
            for i in range(max(args.warmup, 2)):
                run_fwd_bwd_opt(s_num, s_cats, s_labels, set_to_none=False)
            torch.cuda.synchronize()  # graph block runs on GPU only
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                # static outputs: every replay rewrites them in place
                s_out = run_fwd_bwd_opt(s_num, s_cats, s_labels,
                                        set_to_none=False)
            graph = g
        except Exception as e:
            print(f"# graph capture failed ({type(e).__name__}: {e}); eager fallback")
            graph = None

    def step(i):
        num, flat, labels = pool[i % len(pool)]
        if graph is not None:
            s_num.copy_(num)
            s_flat.copy_(flat)
            s_labels.copy_(labels)
            graph.replay()
            return s_out
        return run_fwd_bwd_opt(num, carve(flat), labels)

    for i in range(args.warmup):
        step(i)

    de.comm.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for i in range(args.steps):
        out = step(i)
    de.comm.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    # max over ranks
    t = torch.tensor([elapsed], device=device)
    if world > 1:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs and out is not None:
        last_flat = pool[(args.steps - 1) % len(pool)][1]
        dump_outputs(args.dump_outputs, model, out[0], out[1],
                     carve(last_flat), rank, world)

    global_batch = b * world
    samples_per_sec = global_batch * args.steps / elapsed
    # 8xA100 TF32 DLRM at global batch 65536; synthetic models
    # publish ms/iter, not samples/s — no samples/s baseline for those.
    baseline = 9157869.0 if args.model == "dlrm-criteo" else None
    # metric names the MEASURED config (batch per GPU, weak scaling) — the
    # N=1 default bs/gpu=65536 equals the reference's global bs=64k config.
    metric = f"samples/sec (whole node) {name} bs/gpu={b}"
    if rank == 0:
        print(json.dumps({
            "metric": metric,
            "value": samples_per_sec,
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": (samples_per_sec / baseline) if baseline else None,
            "dtype": "bf16" if use_bf16 else "fp32",
            "data": "synthetic (power-law ids alpha=1.05, random-init weights)",
            "config": {
                "model": name,
                "global_batch": global_batch,
                "batch_per_gpu": b,
                "embedding_dim": 128,
                "parallelism": f"hybrid dp+mp (strategy={args.strategy}) x{world}",
            },
        }))


if __name__ == "__main__":
    main()
