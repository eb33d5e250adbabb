"""Multi-hot expansion on the CPU: the function against its definition, and
DistributedEmbedding / DLRM fed one-hot ids with ``set_multi_hot`` against
the same modules fed the expanded ids.  Ids are integers, so every
comparison of the two feeds is exact."""

import os
import random
import subprocess
import sys

import pytest
import torch

from conftest import run_distributed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


# --- the definition, on Python ints, independent of the package's code -----

def _mix64(k):
    k = (k + 0x9E3779B97F4A7C15) & M64
    k = ((k ^ (k >> 30)) * 0xBF58476D1CE4E5B9) & M64
    k = ((k ^ (k >> 27)) * 0x94D049BB133111EB) & M64
    return k ^ (k >> 31)


def _bag(x, vocab, hotness, seed, feature):
    if not 0 <= x < vocab:
        return [x] * hotness
    key_f = _mix64((seed & M64) ^ _mix64(feature & M64))
    inner = _mix64((key_f + x) & M64)
    return [x] + [_mix64((inner + k) & M64) % vocab
                  for k in range(1, hotness)]


GOLDEN = [
    ((5, 1000, 4, 1234, 0), [5, 667, 890, 726]),
    ((5, 1000, 4, 1234, 1), [5, 875, 183, 771]),
    ((0, 40000000, 3, 0, 25), [0, 1436384, 19127424]),
    ((2**33 + 4, 2**33 + 5, 3, 7, 2), [8589934596, 978949023, 5003538532]),
    ((-1, 1000, 3, 7, 2), [-1, -1, -1]),
    ((1000, 1000, 3, 7, 2), [1000, 1000, 1000]),
]


@pytest.mark.parametrize("args,want", GOLDEN)
def test_golden_values(args, want):
    from distributed_embeddings_amd import multi_hot_expand
    x, vocab, h, seed, feature = args
    assert _bag(*args) == want
    got = multi_hot_expand(torch.tensor([x]), vocab, h, seed, feature)
    assert got.dtype == torch.int64 and got.shape == (1, h)
    assert got[0].tolist() == want


def test_matches_python_int_definition():
    from distributed_embeddings_amd.ops.embedding_lookup import multi_hot_expand
    rng = random.Random(99)
    vocabs = [1, 7, 2**33 + 5]
    for case in range(200):
        vocab = vocabs[case] if case < len(vocabs) else \
            rng.choice([1, 7, 1000, 40_000_000, 2**33 + 5, rng.randrange(1, 2**40)])
        h = rng.randrange(1, 12)
        seed = rng.randrange(-2**63, 2**63)
        feature = rng.randrange(0, 64)
        # ids inside the vocabulary, at its edges and outside it
        xs = [rng.randrange(0, vocab) for _ in range(3)] + \
            [0, vocab - 1, vocab, -1, -rng.randrange(1, 2**62)]
        got = multi_hot_expand(torch.tensor(xs), vocab, h, seed, feature)
        assert got.shape == (len(xs), h)
        for x, row in zip(xs, got.tolist()):
            assert row == _bag(x, vocab, h, seed, feature), \
                (x, vocab, h, seed, feature)


def test_properties():
    from distributed_embeddings_amd import multi_hot_expand
    ids = torch.randint(0, 500, (3, 40), generator=torch.Generator().manual_seed(1))
    one = multi_hot_expand(ids, 500, 1, 11, 3)
    assert torch.equal(one, ids[..., None])
    bags = multi_hot_expand(ids, 500, 9, 11, 3)
    assert bags.shape == (3, 40, 9)
    assert torch.equal(bags[..., 0], ids)                 # slot 0 is the id
    assert int(bags.min()) >= 0 and int(bags.max()) < 500
    # a pure function of (seed, feature, id): equal ids give equal bags
    again = multi_hot_expand(ids.flatten().flip(0), 500, 9, 11, 3).flip(0)
    assert torch.equal(again.view(3, 40, 9), bags)
    # a prefix of a longer bag
    assert torch.equal(multi_hot_expand(ids, 500, 4, 11, 3), bags[..., :4])
    assert not torch.equal(multi_hot_expand(ids, 500, 9, 12, 3), bags)
    assert not torch.equal(multi_hot_expand(ids, 500, 9, 11, 4), bags)
    with pytest.raises(ValueError):
        multi_hot_expand(ids, 0, 3, 1)
    with pytest.raises(ValueError):
        multi_hot_expand(ids, 500, 0, 1)


def test_uniformity_fixed_seed():
    """70 000 hashed slots over vocab 7000: each residue mod 7 between 9 500
    and 10 500 times (the definition gives 9 913 .. 10 061)."""
    from distributed_embeddings_amd import multi_hot_expand
    bags = multi_hot_expand(torch.arange(7000), 7000, 11, 1234, 3)
    counts = torch.bincount((bags[:, 1:] % 7).flatten(), minlength=7).tolist()
    want = [0] * 7
    for x in range(7000):
        for v in _bag(x, 7000, 11, 1234, 3)[1:]:
            want[v % 7] += 1
    assert counts == want
    assert (min(want), max(want)) == (9913, 10061)
    assert all(9500 <= c <= 10500 for c in counts), counts


# --- DistributedEmbedding ---------------------------------------------------

SEED = 77
WIDTH = 8


def _plan(kind):
    """(table configs, input_table_map, hotness, DistributedEmbedding kwargs)"""
    import distributed_embeddings_amd as de
    if kind == "hybrid":
        # table 0 data-parallel, 1 shared by inputs 1 and 4, 2 row-sliced,
        # 3 column-sliced in two, 4 without combiner
        rows = [8, 400, 900, 600, 50]
        comb = ["sum", "sum", "mean", "sum", None]
        tmap = [0, 1, 2, 3, 1, 4]
        hot = [2, 1, 3, 27, 5, 1]
        # round-robin placement: the two slices land on different ranks
        kw = dict(strategy="basic", data_parallel_threshold=8 * WIDTH,
                  row_slice_threshold=900 * WIDTH,
                  column_slice_threshold=4000)
    elif kind == "tp":       # all table-parallel, table 2 column-sliced
        rows = [300, 40, 600, 70]
        comb = ["sum"] * 4
        tmap = [0, 1, 2, 3, 1]
        hot = [1, 2, 27, 3, 5]
        kw = dict(strategy="memory_balanced", column_slice_threshold=4000)
    else:                    # "packed": forward_packed applies
        rows = [300, 40, 100, 70]
        comb = ["sum"] * 4
        tmap = [0, 1, 2, 3]
        hot = [1, 2, 27, 5]
        kw = dict(strategy="memory_balanced")
    tables = [de.TableConfig(r, WIDTH, c) for r, c in zip(rows, comb)]
    return tables, tmap, hot, kw


def _expanded(ids, tables, tmap, hot, gids=None):
    from distributed_embeddings_amd import multi_hot_expand
    gids = range(len(ids)) if gids is None else gids
    return [multi_hot_expand(x, tables[tmap[f]].input_dim, hot[f], SEED, f)
            if hot[f] > 1 else x for f, x in zip(gids, ids)]


def _de_worker(rank, world, kind, dp_input):
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer
    tables, tmap, hot, kw = _plan(kind)
    gw = torch.Generator().manual_seed(3)
    weights = [torch.randn(t.input_dim, WIDTH, generator=gw).numpy()
               for t in tables]

    def make():
        m = de.DistributedEmbedding(tables, dp_input=dp_input,
                                    input_table_map=tmap, **kw)
        m.set_weights(weights)
        m.enable_fused_sgd(0.05)
        opt = de.DistributedOptimizer(
            SparseEmbeddingOptimizer(m.parameters(), lr=0.05), average=False)
        return m, opt

    a, opt_a = make()
    a.set_multi_hot(hot, seed=SEED)
    b, opt_b = make()
    if kind == "hybrid":
        plan = a.strategy
        assert plan.dp_table_ids and plan.row_table_ids
    if kind != "packed" and world > 1:    # a table has one slice per rank at most
        assert a.strategy.sliced_out_ranges
    if kind == "packed":
        assert a.packed_forward_available()

    lb = 4
    B = lb * world
    gi = torch.Generator().manual_seed(5)
    ids = [torch.randint(0, tables[t].input_dim, (B,), generator=gi)
           for t in tmap]
    ids[-1][0] = -1          # out of vocabulary: passes through unhashed
    if dp_input:
        gids = list(range(len(tmap)))
        one_hot = [x[rank * lb:(rank + 1) * lb] for x in ids]
    else:
        gids = a.local_input_ids()
        one_hot = [ids[f] for f in gids]
    # every second one-hot input as [b, 1]
    one_hot = [x[:, None] if i % 2 else x for i, x in enumerate(one_hot)]
    bags = _expanded(one_hot, tables, tmap, hot, gids)
    bags = [x.reshape(x.shape[0], -1) if hot[f] > 1 else x
            for f, x in zip(gids, bags)]

    ok = True
    for _ in range(2):
        outs = []
        for m, opt, inp in ((a, opt_a, one_hot), (b, opt_b, bags)):
            opt.zero_grad(set_to_none=True)
            out = m(inp)
            sum((o * o).sum() for o in out).backward()
            opt.step()
            outs.append(out)
        ok = ok and all(x.shape == y.shape and torch.equal(x, y)
                        for x, y in zip(*outs))
    wa = a.get_weights(all_ranks=True)
    wb = b.get_weights(all_ranks=True)
    ok = ok and all(torch.equal(torch.as_tensor(x), torch.as_tensor(y))
                    for x, y in zip(wa, wb))
    moved = any(not torch.equal(torch.as_tensor(x), torch.as_tensor(w))
                for x, w in zip(wa, weights))
    # a [b, h] input is taken as it is while the mode is on
    mixed = [y if i % 2 else x for i, (x, y) in enumerate(zip(one_hot, bags))]
    with torch.no_grad():
        ok = ok and all(torch.equal(x, y) for x, y in zip(a(mixed), b(bags)))
        if kind == "packed":
            pa, _ = a.forward_packed(one_hot)
            pb, _ = b.forward_packed(bags)
            ok = ok and pa.shape == pb.shape and torch.equal(pa, pb)
    return bool(ok and moved)


@pytest.mark.parametrize("kind,dp_input", [("hybrid", True), ("tp", True),
                                           ("tp", False), ("packed", True)])
def test_dist_embedding_world1(kind, dp_input):
    assert _de_worker(0, 1, kind, dp_input)


@pytest.mark.parametrize("kind,dp_input", [("hybrid", True), ("tp", False),
                                           ("packed", True)])
def test_dist_embedding_world2(kind, dp_input):
    assert all(run_distributed(_de_worker, world=2, args=(kind, dp_input)))


def _async_worker(rank, world):
    """redistribute_async carries the one-hot ids; the expansion follows."""
    import distributed_embeddings_amd as de
    tables, tmap, hot, kw = _plan("tp")
    torch.manual_seed(0)
    a = de.DistributedEmbedding(tables, input_table_map=tmap, **kw)
    de.broadcast_parameters(a)
    a.set_multi_hot(hot, seed=SEED)
    gi = torch.Generator().manual_seed(5)
    ids = [torch.randint(0, tables[t].input_dim, (4 * world,), generator=gi)
           [rank * 4:(rank + 1) * 4] for t in tmap]
    with torch.no_grad():
        handle = a.redistribute_async(ids)
        assert handle is not None
        # one id per sample and local input crosses, not a bag
        assert handle["recv"].numel() == 4 * world * len(handle["my_sizes"])
        got = a(ids, async_handle=handle)
        want = a(_expanded(ids, tables, tmap, hot))
    return all(torch.equal(x, y) for x, y in zip(got, want))


def test_redistribute_async_world2():
    assert all(run_distributed(_async_worker, world=2))


def test_offloaded_table_expands_on_the_host():
    import distributed_embeddings_amd as de
    tables = [de.TableConfig(300, WIDTH, "sum"), de.TableConfig(40, WIDTH, "sum")]
    hot = [5, 2]
    torch.manual_seed(0)
    a = de.DistributedEmbedding(tables, gpu_embedding_size=100)
    assert any(getattr(l, "_cpu_offload", False) for l in a.col_layers)
    ids = [torch.randint(0, 300, (6,)), torch.randint(0, 40, (6,))]
    with torch.no_grad():
        want = a(_expanded(ids, tables, [0, 1], hot))
        a.set_multi_hot(hot, seed=SEED)
        got = a(ids)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_set_multi_hot_errors_and_repr():
    import distributed_embeddings_amd as de
    tables = [de.TableConfig(30, WIDTH, "sum"), de.TableConfig(40, WIDTH)]
    m = de.DistributedEmbedding(tables)
    with pytest.raises(ValueError):
        m.set_multi_hot([2])                  # wrong length
    with pytest.raises(ValueError):
        m.set_multi_hot([0, 1])               # h < 1
    with pytest.raises(ValueError):
        m.set_multi_hot([2, 3])               # h > 1 without a combiner
    assert "multi_hot" not in repr(m)
    m.set_multi_hot([3, 1], seed=9)
    assert "multi_hot=[3, 1]" in repr(m) and "multi_hot_seed=9" in repr(m)
    x = torch.zeros(4, dtype=torch.long)
    for bad in (x.view(2, 2), x.view(4, 1, 1), x.view(1, 4)):
        with pytest.raises(ValueError):
            m([bad, x])                       # neither one-hot nor [b, 3]
        with pytest.raises(ValueError):
            m.forward_packed([bad, x])
    assert m([x, x])[0].shape == (4, WIDTH)
    m.set_multi_hot(None)                     # off again: [2, 2] is a bag of 2
    assert m([x.view(2, 2), x])[0].shape == (2, WIDTH)


@pytest.mark.parametrize("bits", [8, 4])
def test_quantized_serving(bits):
    import distributed_embeddings_amd as de
    tables, tmap, hot, kw = _plan("packed")
    torch.manual_seed(1)
    a = de.DistributedEmbedding(tables, input_table_map=tmap)
    a.set_multi_hot(hot, seed=SEED)
    a.quantize_(bits=bits)
    ids = [torch.randint(0, tables[t].input_dim, (5,)) for t in tmap]
    bags = _expanded(ids, tables, tmap, hot)
    got = a(ids)
    a.set_multi_hot(None)
    want = a(bags)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


# --- DLRM -------------------------------------------------------------------

SIZES = [50, 7, 120, 33, 64, 200]
HOT = [1, 2, 3, 27, 1, 5]


def _dlrm(interaction, multi_hot=True, **kw):
    from distributed_embeddings_amd.models.dlrm import DLRM
    return DLRM(SIZES, embedding_dim=16, bottom_mlp_dims=(32, 16),
                top_mlp_dims=(32, 1), num_numerical=4,
                strategy="memory_balanced", interaction=interaction,
                cross_layers=2, cross_rank=4,
                multi_hot_sizes=HOT if multi_hot else None,
                multi_hot_seed=SEED, **kw)


@pytest.mark.parametrize("interaction", ["dot", "cross"])
def test_dlrm_matches_pre_expanded_inputs(interaction):
    from distributed_embeddings_amd import multi_hot_expand
    torch.manual_seed(0)
    model = _dlrm(interaction)
    assert "combiner=sum" in repr(model.embeddings)
    g = torch.Generator().manual_seed(7)
    cats = [torch.randint(0, s, (8,), generator=g) for s in SIZES]
    num = torch.rand(8, 4, generator=g)
    bags = [multi_hot_expand(x, s, h, SEED, f)
            for f, (x, s, h) in enumerate(zip(cats, SIZES, HOT))]
    assert [b.shape[1] for b in bags] == HOT
    with torch.no_grad():
        assert torch.equal(model(num, cats), model(num, bags))
        # the bags are summed: the plain torch sum of the table rows
        emb = model.embeddings(cats)
        tabs = model.embeddings.get_weights()
        for e, t, b in zip(emb, tabs, bags):
            assert torch.allclose(e, torch.as_tensor(t)[b].sum(1), atol=1e-5)


def test_dlrm_arguments():
    with pytest.raises(ValueError):
        from distributed_embeddings_amd.models.dlrm import DLRM
        DLRM(SIZES, embedding_dim=16, multi_hot_sizes=[1, 2])
    from distributed_embeddings_amd.models.config import MLPERF_MULTI_HOT_SIZES
    assert len(MLPERF_MULTI_HOT_SIZES) == 26
    assert sum(MLPERF_MULTI_HOT_SIZES) == 214
    plain = _dlrm("dot", multi_hot=False)
    assert "combiner=None" in repr(plain.embeddings)
    assert plain.embeddings._mh_hotness is None


def _dlrm_worker(rank, world, interaction):
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer
    torch.manual_seed(0)
    model = _dlrm(interaction)
    gw = torch.Generator().manual_seed(42)
    model.embeddings.set_weights(
        [torch.randn(s, 16, generator=gw).numpy() * 0.3 for s in SIZES])
    for mod in (model.bottom_mlp, model.top_mlp, model.cross):
        for p in (mod.parameters() if mod is not None else ()):
            with torch.no_grad():
                p.copy_(torch.randn(p.shape, generator=gw) * 0.3)
    de.broadcast_parameters(model)
    model.embeddings.enable_fused_sgd(0.05)
    opt = de.DistributedOptimizer(
        SparseEmbeddingOptimizer(model.parameters(), lr=0.05), average=False)
    gi = torch.Generator().manual_seed(7)
    B = 8
    cats = [torch.randint(0, s, (B,), generator=gi) for s in SIZES]
    num = torch.rand(B, 4, generator=gi)
    labels = torch.randint(0, 2, (B, 1), generator=gi).float()
    lb = B // world
    sl = slice(rank * lb, (rank + 1) * lb)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        logits = model(num[sl], [c[sl] for c in cats])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            logits.float(), labels[sl], reduction="sum") / B
        loss.backward()
        opt.step()
    out = model(num[sl], [c[sl] for c in cats]).detach()
    tables = model.embeddings.get_weights(all_ranks=True)
    return {"out": out, "tables": [torch.as_tensor(t) for t in tables]}


@pytest.mark.parametrize("interaction", ["dot", "cross"])
def test_dlrm_world2_matches_world1(interaction):
    r2 = run_distributed(_dlrm_worker, world=2, args=(interaction,))
    r1 = _dlrm_worker(0, 1, interaction)
    for rank in range(2):
        got, ref = r2[rank]["out"], r1["out"][rank * 4:(rank + 1) * 4]
        assert torch.allclose(got, ref, atol=1e-4), \
            f"rank{rank} fwd err {(got - ref).abs().max()}"
    for t in range(len(SIZES)):
        a, b = r2[0]["tables"][t], r1["tables"][t]
        assert torch.allclose(a, b, atol=1e-4), \
            f"table {t} err {(a - b).abs().max()}"


# --- data and example --------------------------------------------------------

def test_synthetic_data_multi_hot():
    from distributed_embeddings_amd.utils.criteo import SyntheticDLRMData
    data = SyntheticDLRMData([100, 200, 30], local_bs=8, num_batches=2,
                             multi_hot_sizes=[1, 4, 27], learnable=True)
    num, cats, labels = next(iter(data))
    assert [tuple(c.shape) for c in cats] == [(8, 1), (8, 4), (8, 27)]
    assert all(int(c.min()) >= 0 and int(c.max()) < s
               for c, s in zip(cats, [100, 200, 30]))
    assert torch.equal(labels, (cats[0][:, 0] % 2).view(-1, 1).float())
    plain = SyntheticDLRMData([100, 200, 30], local_bs=8, num_batches=2)
    assert [tuple(c.shape) for c in next(iter(plain))[1]] == [(8,)] * 3


def _run_example(args):
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "dlrm_main.py")] + args,
        capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert proc.returncode == 0, (
        f"dlrm_main.py failed:\n{proc.stdout[-2000:]}\n{proc.stderr[-2000:]}")
    return proc.stdout


@pytest.mark.parametrize("extra", [
    ["--interaction", "cross", "--cross-rank", "8"],
    ["--multi-hot-source", "data", "--fused-optimizer"]])
def test_dlrm_example_multi_hot(extra):
    out = _run_example(["--multi-hot", "mlperf", "--batch-size", "64",
                        "--num-batches", "2", "--embedding-dim", "16",
                        "--table-size-cap", "1000"] + extra)
    assert "loss" in out
