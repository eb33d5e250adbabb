"""Per-sample weights through DistributedEmbedding, world 2 on gloo.

Every case is compared with the single-process formula of
test_weighted_lookup.py in float64: out[r] = c_r * sum_k w_k * T[i_k].  Bags
hold at most 4 ids of N(0,1) tables with |w| < 1.5, so fp32 stays far inside
the 1e-5 the other distributed tests use (n * eps * max|x| ~ 4 * 6e-8 * 7).
"""

import pytest
import torch

from conftest import run_distributed
from test_weighted_lookup import _dense_grad_ref, _forward_ref

_B = 4  # per-rank batch
_LR = 0.1

# name -> tables (rows, width, combiner), how each input is fed (w: weighted
# Ragged, r: Ragged without weights, d: dense [b, 2]) and the plan arguments
_CASES = {
    # every table model-parallel, one per rank
    "basic": dict(tables=[(50, 8, "sum"), (60, 8, "mean")], feed="ww",
                  kwargs={}),
    # the 50 x 8 table is cut into two column slices
    "column": dict(tables=[(50, 8, "mean"), (30, 4, "sum")], feed="ww",
                   kwargs={"column_slice_threshold": 200}),
    # the 20 x 8 table is replicated
    "dp": dict(tables=[(20, 8, "mean"), (60, 8, "sum")], feed="ww",
               kwargs={"data_parallel_threshold": 20 * 8}),
    # rank 0 serves tables 0 and 2 in one concat group, rank 1 tables 1 and 3:
    # a weighted and an unweighted pair share a fused lookup
    "concat": dict(tables=[(50, 8, "sum"), (60, 8, "sum"), (40, 8, "sum"),
                           (30, 8, "sum")], feed="wwrd", kwargs={}),
    "mp_input": dict(tables=[(50, 8, "sum"), (60, 8, "mean")], feed="wr",
                     kwargs={"dp_input": False}),
}


def _tables(case):
    g = torch.Generator().manual_seed(3)
    return [torch.randn(rows, width, generator=g)
            for rows, width, _ in _CASES[case]["tables"]]


def _global_inputs(case, world):
    """Per input: (ids, splits, weights) of the whole batch; dense inputs are
    [world * _B, 2] ids with weights of ones."""
    g = torch.Generator().manual_seed(17)
    out = []
    for (rows, _, _), kind in zip(_CASES[case]["tables"], _CASES[case]["feed"]):
        n = world * _B
        if kind == "d":
            lengths = torch.full((n,), 2)
        else:
            lengths = torch.randint(0, 5, (n,), generator=g)
            lengths[1] = 0
        splits = torch.cat([torch.zeros(1, dtype=torch.long),
                            lengths.cumsum(0)])
        ids = torch.randint(0, rows, (int(splits[-1]),), generator=g)
        w = torch.rand(ids.numel(), generator=g) * 3 - 1.5
        w[::5] = 0
        if kind != "w":
            w = torch.ones_like(w)
        out.append((ids, splits, w))
    return out


def _slice_input(inp, kind, lo, hi):
    from distributed_embeddings_amd import Ragged
    ids, splits, w = inp
    s, e = int(splits[lo]), int(splits[hi])
    if kind == "d":
        return ids[s:e].view(hi - lo, 2)
    return Ragged(ids[s:e], splits[lo:hi + 1] - s,
                  w[s:e] if kind == "w" else None)


def _worker(rank, world, case, step):
    import distributed_embeddings_amd as de
    spec = _CASES[case]
    model = de.DistributedEmbedding(
        [de.TableConfig(*t) for t in spec["tables"]], strategy="basic",
        **spec["kwargs"])
    plan = model.strategy
    if case == "column":
        assert plan.sliced_out_ranges
    if case == "dp":
        assert plan.dp_table_ids == [0]
    if case == "concat":
        assert any(len(g.members) >= 2
                   for g in plan.local_concat_groups(rank))
    model.set_weights([t.numpy() for t in _tables(case)])
    inputs = _global_inputs(case, world)
    if spec["kwargs"].get("dp_input", True):
        local = [_slice_input(x, k, rank * _B, (rank + 1) * _B)
                 for x, k in zip(inputs, spec["feed"])]
    else:
        local = [_slice_input(inputs[i], spec["feed"][i], 0, world * _B)
                 for i in model.local_input_ids()]
    outs = model(local)
    result = {"outs": [o.detach() for o in outs]}
    if step:
        opt = de.DistributedOptimizer(
            torch.optim.SGD(model.parameters(), lr=_LR))
        sum((o * o).sum() for o in outs).backward()
        opt.step()
        result["weights"] = [torch.as_tensor(w)
                             for w in model.get_weights(all_ranks=True)]
    return result


@pytest.mark.parametrize("case", list(_CASES))
def test_weighted_world2_matches_formula(case):
    world = 2
    step = case == "basic"
    results = run_distributed(_worker, world=world, args=(case, step))
    tables, inputs = _tables(case), _global_inputs(case, world)
    refs = [_forward_ref(t, ids, splits, w, comb)
            for t, (ids, splits, w), (_, _, comb)
            in zip(tables, inputs, _CASES[case]["tables"])]
    for rank in range(world):
        outs = results[rank]["outs"]
        assert len(outs) == len(tables)
        for t, o in enumerate(outs):
            ref = refs[t][rank * _B:(rank + 1) * _B]
            assert o.shape == ref.shape
            assert torch.allclose(o.double(), ref, atol=1e-5), \
                f"rank {rank} table {t}: {(o.double() - ref).abs().max()}"
    # the weights matter: the unweighted result is far away
    ids, splits, w = inputs[0]
    plain = _forward_ref(tables[0], ids, splits, torch.ones_like(w),
                         _CASES[case]["tables"][0][2])
    assert float((plain - refs[0]).abs().max()) > 0.1
    if step:
        # loss = sum(out^2): the table gradient comes back through the
        # output all-to-all; model-parallel tables see the whole batch
        for t, (ids, splits, w) in enumerate(inputs):
            rows, _, comb = _CASES[case]["tables"][t]
            want = tables[t].double() - _LR * _dense_grad_ref(
                2 * refs[t], ids, splits, w, rows, comb)
            assert not torch.allclose(want, tables[t].double(), atol=1e-3)
            for rank in range(world):
                got = results[rank]["weights"][t]
                assert torch.allclose(got.double(), want, atol=1e-5), \
                    f"rank {rank} table {t}"


# the bags of test_dist_embedding._ragged_rowslice_worker, with weights
_ROW_LISTS = [[1, 2, 250], [7], [299, 0], [42, 42, 42, 99],
              [280], [5, 260], [150], [3, 297]]
_ROW_WEIGHTS = [[0.5, -1.25, 2.0], [0.0], [1.5, -0.5], [1.0, -1.0, 0.25, 3.0],
                [-2.0], [0.75, 0.0], [1.25], [-0.25, 0.5]]


def _rowslice_worker(rank, world):
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd import Ragged
    model = de.DistributedEmbedding([de.TableConfig(300, 8, "sum")],
                                    row_slice_threshold=1)
    assert len(model.row_layers) == 1 and not len(model.col_layers)
    g = torch.Generator().manual_seed(3)
    model.set_weights([torch.randn(300, 8, generator=g).numpy()])
    sl = slice(rank * 4, (rank + 1) * 4)
    return model([Ragged.from_lists(_ROW_LISTS[sl],
                                    _ROW_WEIGHTS[sl])])[0].detach()


def test_weighted_row_slice_world2():
    from distributed_embeddings_amd import Ragged
    results = run_distributed(_rowslice_worker, world=2)
    table = torch.randn(300, 8, generator=torch.Generator().manual_seed(3))
    rg = Ragged.from_lists(_ROW_LISTS, _ROW_WEIGHTS)
    ref = _forward_ref(table, rg.values, rg.row_splits, rg.weights, "sum")
    plain = _forward_ref(table, rg.values, rg.row_splits,
                         torch.ones_like(rg.weights), "sum")
    assert float((plain - ref).abs().max()) > 0.1
    for rank in range(2):
        assert torch.allclose(results[rank].double(),
                              ref[rank * 4:(rank + 1) * 4], atol=1e-5)


def test_weighted_cpu_offload_world1():
    """The offloaded group's lookup goes through embedding_lookup on the CPU
    and must take the weights along."""
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd import Ragged
    sizes = [10, 1000, 100]
    model = de.DistributedEmbedding(
        [de.TableConfig(s, 8, "mean") for s in sizes],
        gpu_embedding_size=(10 + 100) * 8)
    assert any(getattr(lyr, "_cpu_offload", False)
               for lyr in model.col_layers)
    g = torch.Generator().manual_seed(8)
    tables = [torch.randn(s, 8, generator=g) for s in sizes]
    model.set_weights([t.numpy() for t in tables])
    inputs = []
    for s in sizes:
        lengths = torch.randint(0, 5, (6,), generator=g)
        ids = torch.randint(0, s, (int(lengths.sum()),), generator=g)
        w = torch.rand(ids.numel(), generator=g) * 3 - 1.5
        inputs.append(Ragged.from_row_lengths(ids, lengths, w))
    for o, x, t in zip(model(inputs), inputs, tables):
        ref = _forward_ref(t, x.values, x.row_splits, x.weights, "mean")
        assert torch.allclose(o.double(), ref, atol=1e-5)


def test_weights_requiring_grad_raise():
    """Weights are data to the distributed wrapper: no silent zero."""
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd import Ragged
    model = de.DistributedEmbedding([de.TableConfig(50, 8, "sum")])
    w = torch.ones(3, requires_grad=True)
    rg = Ragged(torch.tensor([1, 2, 3]), torch.tensor([0, 2, 3]), w)
    with pytest.raises(ValueError, match="Embedding"):
        model([rg])
    out = model([Ragged(rg.values, rg.row_splits, w.detach() * 2)])[0]
    plain = model([Ragged(rg.values, rg.row_splits)])[0]
    assert torch.allclose(out, 2 * plain)
    with pytest.raises(ValueError):  # one weight short
        model([Ragged(rg.values, rg.row_splits, torch.ones(2))])
