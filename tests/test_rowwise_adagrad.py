"""Row-wise Adagrad: one fp32 accumulator per embedding row.

For every unique in-range id r of a step, with G[r] its summed gradient row:

    state[r] += mean_c(G[r, c]^2)
    w[r, c]  -= lr * G[r, c] / (sqrt(state[r]) + eps)

The CPU tests check the Python paths against this formula written out in
float64; the GPU tests check the HIP kernels over every tiling of the shared
gather-reduce helpers, on the case test_gpu.py builds for them.

Tolerances are the per-element bounds derived above ``_HELPER_WIDTHS`` in
test_gpu.py: 1e-4 for sums of <= 7 terms, 1e-3 for up to 300 terms, plus
2**-8 * |ref| where the result is stored as bf16.  The weight moves by
lr * G / (sqrt(state) + eps) with state >= 1 and lr = 0.125, so an error in G
reaches the weight scaled down, never up.  The row state is a mean over the
row of G^2; its error is at most 2 * max|G| * (error in G) plus one fp32
rounding.  In this case |G| < 11 and fp32 summation errs by less than 1/40
of the bound on G, so the fp32 state stays inside the per-element bound
(measured on the CPU: 1/20 of it) and no wider one is needed.  Each GPU test
asserts that first: the same formula in fp32 on the CPU has to stay inside
the bound against float64 before the kernel is held to it.
"""

import pytest
import torch

from conftest import run_distributed
from test_gpu import (_HELPER_VOCAB, _HELPER_WIDTHS, _assert_within,
                      _dense_grad_ref, _helper_case, _helper_dense,
                      _terms_atol)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")

_LR = 0.125
_EPS = float(torch.tensor(1e-10, dtype=torch.float32))


def _rowwise_step(w0, state0, g, lr, eps):
    """The formula in g's precision on a dense [vocab, width] summed grad.
    A row nobody touched has g == 0 and comes back unchanged."""
    st = state0.to(g.dtype) + (g * g).mean(dim=1)
    w = w0.to(g.dtype) - lr * g / (st.sqrt() + eps).unsqueeze(1)
    return w, st


def _dense_grad(up, values, row_splits, vocab, combiner):
    """float64 [vocab, width] summed gradient: duplicates added, mean
    weights applied, out-of-range ids dropped."""
    lengths = row_splits[1:] - row_splits[:-1]
    row_of = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    rows = up.double()[row_of]
    if combiner == "mean":
        rows = rows / lengths.clamp(min=1).double()[row_of].unsqueeze(1)
    valid = (values >= 0) & (values < vocab)
    dense = torch.zeros(vocab, up.shape[1], dtype=torch.float64)
    return dense.index_add_(0, values[valid], rows[valid])


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------

# id 1 three times (twice in one bag), id 3 twice, ids 5 and 7 once; rows
# 0, 2, 4, 6, 8, 9 never
_LISTS_A = [[1, 1, 3], [1, 5], [7, 3]]
# second step: id 3 stays away, so its state has to survive bitwise
_LISTS_B = [[1, 7], [5, 5, 5], [2]]


def _upstream(n, width):
    # all positive, so the square of a sum is far from the sum of squares
    return (torch.arange(1, n + 1).float().unsqueeze(1)
            * torch.linspace(0.5, 1.5, width).unsqueeze(0))


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_fused_layer_cpu_matches_formula(combiner, seed):
    from distributed_embeddings_amd import Embedding, Ragged
    vocab, width, lr, eps = 10, 4, 0.1, 1e-10
    emb = Embedding(vocab, width, combiner=combiner)
    emb.enable_fused_optimizer("rowwise_adagrad", lr, eps)
    w_ref = emb.weight.detach().double().clone()
    st_ref = torch.zeros(vocab, dtype=torch.float64)
    up = _upstream(3, width)
    for lists in (_LISTS_A, _LISTS_B):
        rg = Ragged.from_lists(lists)
        w_before = emb.weight.detach().clone()
        st_before = emb._fused_state.clone()
        emb(rg).backward(up)
        g = _dense_grad(up, rg.values, rg.row_splits, vocab, combiner)
        w_ref, st_ref = _rowwise_step(w_ref, st_ref, g, lr, eps)
        assert emb.weight.grad is None
        assert torch.allclose(emb._fused_state.double(), st_ref, rtol=1e-6,
                              atol=1e-7)
        assert torch.allclose(emb.weight.detach().double(), w_ref, rtol=1e-6,
                              atol=1e-6)
        untouched = torch.ones(vocab, dtype=torch.bool)
        untouched[rg.values] = False
        assert untouched.any()
        assert torch.equal(emb.weight.detach()[untouched],
                           w_before[untouched])
        assert torch.equal(emb._fused_state[untouched], st_before[untouched])
    # the inputs tell the square of the summed row from per-occurrence
    # squares: for id 1 they differ by more than the state of any other row
    rg = Ragged.from_lists(_LISTS_A)
    lengths = rg.row_splits[1:] - rg.row_splits[:-1]
    row_of = torch.repeat_interleave(torch.arange(3), lengths)
    rows = up.double()[row_of]
    if combiner == "mean":
        rows = rows / lengths.double()[row_of].unsqueeze(1)
    per_occurrence = torch.zeros(vocab, dtype=torch.float64).index_add_(
        0, rg.values, (rows * rows).mean(dim=1))
    g = _dense_grad(up, rg.values, rg.row_splits, vocab, combiner)
    assert float((g * g).mean(dim=1)[1] - per_occurrence[1]) > 0.25


def test_sparse_optimizer_cpu_matches_formula(seed):
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    vocab, width, lr, eps = 10, 4, 0.1, 1e-10
    emb = Embedding(vocab, width, combiner="sum")
    dense = torch.nn.Linear(width, 2)
    opt = SparseEmbeddingOptimizer(
        list(emb.parameters()) + list(dense.parameters()), lr=lr,
        method="rowwise_adagrad", eps=eps)
    w_ref = emb.weight.detach().double().clone()
    st_ref = torch.zeros(vocab, dtype=torch.float64)
    d_ref = dense.weight.detach().double().clone()
    d_st = torch.zeros_like(d_ref)
    coef = _upstream(3, 2)
    for lists in (_LISTS_A, _LISTS_B):
        rg = Ragged.from_lists(lists)
        opt.zero_grad()
        out = emb(rg)
        (dense(out) * coef).sum().backward()
        up = coef @ dense.weight.detach()
        d_g = (coef.t() @ out.detach()).double()
        opt.step()
        g = _dense_grad(up, rg.values, rg.row_splits, vocab, "sum")
        w_ref, st_ref = _rowwise_step(w_ref, st_ref, g, lr, eps)
        # dense-grad params keep element-wise Adagrad
        d_st = d_st + d_g * d_g
        d_ref = d_ref - lr * d_g / (d_st.sqrt() + eps)
        assert torch.allclose(emb.weight.detach().double(), w_ref, rtol=1e-5,
                              atol=1e-6)
        assert torch.allclose(dense.weight.detach().double(), d_ref,
                              rtol=1e-5, atol=1e-6)
    state = opt.state[emb.weight]["sum"]
    assert state.shape == (vocab,) and state.dtype == torch.float32
    assert torch.allclose(state.double(), st_ref, rtol=1e-5, atol=1e-7)
    assert opt.state[dense.weight]["sum"].shape == dense.weight.shape


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_state_is_fp32_vocab_vector(dtype, seed):
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    rg = Ragged.from_lists(_LISTS_A)
    emb = Embedding(10, 4, combiner="sum", dtype=dtype)
    emb.enable_fused_optimizer("rowwise_adagrad", 0.1)
    assert emb._fused_state.shape == (10,)
    assert emb._fused_state.dtype == torch.float32
    emb(rg).backward(_upstream(3, 4).to(dtype))
    assert emb._fused_state.shape == (10,)
    assert emb._fused_state.dtype == torch.float32
    assert emb.weight.dtype == dtype
    assert float(emb._fused_state[1]) > 0 and float(emb._fused_state[0]) == 0

    emb2 = Embedding(10, 4, combiner="sum", dtype=dtype)
    opt = SparseEmbeddingOptimizer(emb2.parameters(), lr=0.1,
                                   method="rowwise_adagrad")
    emb2(rg).backward(_upstream(3, 4).to(dtype))
    opt.step()
    state = opt.state[emb2.weight]["sum"]
    assert state.shape == (10,) and state.dtype == torch.float32
    assert emb2.weight.dtype == dtype


def test_reconfigure_replaces_state(seed):
    from distributed_embeddings_amd import Embedding
    emb = Embedding(10, 4, combiner="sum")
    emb.enable_fused_optimizer("adagrad", 0.1)
    assert emb._fused_state.shape == (10, 4)
    emb.enable_fused_optimizer("rowwise_adagrad", 0.1)
    assert emb._fused_state.shape == (10,)
    emb.enable_fused_optimizer("adagrad", 0.1)
    assert emb._fused_state.shape == (10, 4)


def test_out_of_range_ids_ignored(seed):
    from distributed_embeddings_amd.ops.embedding_lookup import (
        csr_lookup_fused_optimizer)
    vocab, width, lr, eps = 10, 4, 0.1, 1e-10
    values = torch.tensor([1, -1, 3, 10, 1, 7, 1 << 40])
    splits = torch.tensor([0, 3, 5, 7])
    up = _upstream(3, width)
    w0 = torch.randn(vocab, width)
    w = w0.clone().requires_grad_(True)
    state = torch.zeros(vocab)
    out = csr_lookup_fused_optimizer(w, values, splits, "mean",
                                     torch.tensor([lr]), state, True, eps)
    out.backward(up)
    g = _dense_grad(up, values, splits, vocab, "mean")
    w_ref, st_ref = _rowwise_step(w0.double(), torch.zeros(vocab).double(), g,
                                  lr, eps)
    assert torch.allclose(state.double(), st_ref, rtol=1e-6, atol=1e-7)
    assert torch.allclose(w.detach().double(), w_ref, rtol=1e-6, atol=1e-6)
    untouched = torch.tensor([0, 2, 4, 5, 6, 8, 9])
    assert torch.equal(w.detach()[untouched], w0[untouched])
    assert bool((state[untouched] == 0).all())


def test_unknown_method_still_raises():
    from distributed_embeddings_amd import Embedding, SparseEmbeddingOptimizer
    emb = Embedding(10, 4, combiner="sum")
    for name in ("rowwise", "row_wise_adagrad", "adam"):
        with pytest.raises(ValueError):
            emb.enable_fused_optimizer(name, 0.1)
        with pytest.raises(ValueError):
            SparseEmbeddingOptimizer(emb.parameters(), method=name)


def _twin_tables(sizes, width, combiners, weights, lr):
    from distributed_embeddings_amd import Embedding
    twins = []
    for size, comb, w in zip(sizes, combiners, weights):
        e = Embedding(size, width, combiner=comb)
        with torch.no_grad():
            e.weight.copy_(w)
        e.enable_fused_optimizer("rowwise_adagrad", lr)
        twins.append(e)
    return twins


def test_distributed_embedding_world1_matches_twin():
    import distributed_embeddings_amd as de
    sizes, width, combiners, lr = [40, 30], 8, ["sum", "mean"], 0.1
    g = torch.Generator().manual_seed(5)
    weights = [torch.randn(s, width, generator=g) for s in sizes]
    model = de.DistributedEmbedding(
        [de.TableConfig(s, width, c) for s, c in zip(sizes, combiners)])
    model.set_weights([w.numpy() for w in weights])
    model.enable_fused_optimizer("rowwise_adagrad", lr)
    fused = [lyr for lyr in list(model.col_layers) + list(model.row_layers)
             if getattr(lyr, "_fused_lr", None) is not None]
    assert fused
    for lyr in fused:
        assert lyr._fused_state.shape == (lyr.weight.shape[0],)
        assert lyr._fused_state.dtype == torch.float32
    twins = _twin_tables(sizes, width, combiners, weights, lr)
    for _ in range(2):
        # few distinct ids: duplicates inside a bag and across bags
        xs = [torch.randint(0, 6, (8, 3), generator=g) for _ in sizes]
        sum((o * o).sum() for o in model(xs)).backward()
        sum(e(x).square().sum() for e, x in zip(twins, xs)).backward()
    for got, e in zip(model.get_weights(), twins):
        assert torch.allclose(torch.as_tensor(got), e.weight.detach(),
                              rtol=1e-5, atol=1e-6)


# each rank's four samples hit rows of both shards, and ids 5 and 700 occur
# on both ranks: the owning shard has to see one summed row
_W2_IDS = [5, 5, 700, 3, 5, 700, 899, 450]


def _rowslice_world2_worker(rank, world):
    import distributed_embeddings_amd as de
    g = torch.Generator().manual_seed(9)
    w0 = torch.randn(900, 8, generator=g)
    model = de.DistributedEmbedding([de.TableConfig(900, 8)],
                                    row_slice_threshold=1)
    assert len(model.row_layers) == 1 and not len(model.col_layers)
    model.set_weights([w0.numpy()])
    model.enable_fused_optimizer("rowwise_adagrad", 0.1)
    assert model.row_layers[0]._fused_state.shape == (450,)
    ids = torch.tensor(_W2_IDS)
    coef = _upstream(len(_W2_IDS), 8)
    sl = slice(rank * 4, (rank + 1) * 4)
    for _ in range(2):
        (model([ids[sl]])[0] * coef[sl]).sum().backward()
    return torch.as_tensor(model.get_weights(all_ranks=True)[0])


def test_row_sliced_world2_matches_twin():
    from distributed_embeddings_amd import Embedding
    results = run_distributed(_rowslice_world2_worker, world=2)
    g = torch.Generator().manual_seed(9)
    w0 = torch.randn(900, 8, generator=g)
    twin = Embedding(900, 8)
    with torch.no_grad():
        twin.weight.copy_(w0)
    twin.enable_fused_optimizer("rowwise_adagrad", 0.1)
    ids = torch.tensor(_W2_IDS)
    for _ in range(2):
        (twin(ids) * _upstream(len(_W2_IDS), 8)).sum().backward()
    assert not torch.equal(twin.weight.detach(), w0)
    for got in results:
        assert torch.allclose(got, twin.weight.detach(), rtol=1e-5, atol=1e-6)


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_fused_update_vs_fp64(combiner):
    """csr_fused_optimizer_apply with a [vocab] state: narrow, wide, wide in
    two column passes, and the 300-long segment through scratch + finalize."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"], case["splits"].cuda()
    lr = torch.tensor([_LR])
    atol = _terms_atol(torch.bincount(ids, minlength=_HELPER_VOCAB))
    ones = torch.ones(_HELPER_VOCAB)
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        for wdt in (torch.float32, torch.bfloat16):
            for gdt in (torch.float32, torch.bfloat16):
                w0, gq = table.to(wdt), grad.to(gdt)
                g64 = _dense_grad_ref(gq, ids, case, combiner, torch.float64)
                g32 = _dense_grad_ref(gq, ids, case, combiner, torch.float32)
                w_ref, st_ref = _rowwise_step(w0, ones, g64, _LR, _EPS)
                w32, st32 = _rowwise_step(w0, ones, g32, _LR, _EPS)
                w_tol = atol + (2.0 ** -8 * w_ref.abs()
                                if wdt == torch.bfloat16 else 0.0)
                tag = f"{combiner} w{width} {wdt} {gdt}"
                _assert_within(f"cpu fp32 weight {tag}", w32, w_ref, w_tol)
                _assert_within(f"cpu fp32 state {tag}", st32.unsqueeze(1),
                               st_ref.unsqueeze(1), atol)
                w = w0.cuda()
                state = ones.cuda()
                ext.csr_fused_optimizer_apply(w, state, ids.cuda(), splits,
                                              gq.cuda(), lr.cuda(),
                                              combiner == "mean", True, _EPS)
                assert state.shape == (_HELPER_VOCAB,)
                _assert_within(f"weight {tag}", w, w_ref, w_tol)
                _assert_within(f"state {tag}", state.unsqueeze(1),
                               st_ref.unsqueeze(1), atol)


@pytest.mark.gpu
@requires_gpu
def test_row_update_vs_fp64():
    """sparse_row_update with a [vocab] state.  The rows handed in are the
    summed gradient itself, so every element is held to the 7-term bound."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    uniq = torch.unique(case["ids_hot"])
    uniq = uniq[torch.randperm(uniq.numel(),
                               generator=torch.Generator().manual_seed(1))]
    atol = torch.full((_HELPER_VOCAB, 1), 1e-4, dtype=torch.float64)
    ones = torch.ones(_HELPER_VOCAB)
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        g32 = _dense_grad_ref(grad, case["ids_hot"], case, "sum",
                              torch.float32)
        rows = g32[uniq].contiguous()
        for wdt in (torch.float32, torch.bfloat16):
            w0 = table.to(wdt)
            w_ref, st_ref = _rowwise_step(w0, ones, g32.double(), _LR, _EPS)
            w32, st32 = _rowwise_step(w0, ones, g32, _LR, _EPS)
            w_tol = atol + (2.0 ** -8 * w_ref.abs()
                            if wdt == torch.bfloat16 else 0.0)
            tag = f"w{width} {wdt}"
            _assert_within(f"cpu fp32 weight {tag}", w32, w_ref, w_tol)
            _assert_within(f"cpu fp32 state {tag}", st32.unsqueeze(1),
                           st_ref.unsqueeze(1), atol)
            w = w0.cuda()
            state = ones.cuda()
            ext.sparse_row_update(w, state, uniq.cuda(), rows.cuda(), _LR,
                                  _EPS, True)
            _assert_within(f"weight {tag}", w, w_ref, w_tol)
            _assert_within(f"state {tag}", state.unsqueeze(1),
                           st_ref.unsqueeze(1), atol)


@pytest.mark.gpu
@requires_gpu
def test_fused_layer_gpu_matches_sparse_optimizer():
    """The in-backward kernels and the optimizer-step kernel agree after two
    steps; ids 0 and 3 occur 2000 times each (long segments)."""
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    torch.manual_seed(31)
    w0 = torch.randn(500, 32)
    ids = torch.cat([torch.randint(0, 500, (4000,)),
                     torch.zeros(2000, dtype=torch.long),
                     torch.full((2000,), 3)]).cuda()
    ids = ids[torch.randperm(8000, device="cuda")]
    splits = torch.arange(0, 8001, 4, device="cuda")
    up = torch.randn(2000, 32, device="cuda")
    e1 = Embedding(500, 32, combiner="mean").cuda()
    e2 = Embedding(500, 32, combiner="mean").cuda()
    with torch.no_grad():
        e1.weight.copy_(w0)
        e2.weight.copy_(w0)
    e1.enable_fused_optimizer("rowwise_adagrad", 0.1)
    o2 = SparseEmbeddingOptimizer(e2.parameters(), lr=0.1,
                                  method="rowwise_adagrad")
    for _ in range(2):
        o2.zero_grad()
        e1(Ragged(ids, splits)).backward(up)
        e2(Ragged(ids, splits)).backward(up)
        o2.step()
    s1, s2 = e1._fused_state, o2.state[e2.weight]["sum"]
    assert s1.shape == s2.shape == (500,)
    print("weight diff",
          float((e1.weight - e2.weight).detach().abs().max()),
          "state diff", float((s1 - s2).abs().max()))
    assert not torch.equal(e1.weight.detach().cpu(), w0)
    assert torch.allclose(e1.weight, e2.weight, atol=1e-3)
    assert torch.allclose(s1, s2, atol=1e-3)


@pytest.mark.gpu
@requires_gpu
def test_graph_capture_rowwise_train_step():
    """One captured train step replays to what eager computes.  256 ids over
    300 rows keep every segment on the in-register path, whose summation
    order is fixed, so the two agree bitwise."""
    from distributed_embeddings_amd import Embedding
    torch.manual_seed(23)
    w0 = torch.randn(300, 64)
    ids = torch.randint(0, 300, (256,), device="cuda")

    def make():
        e = Embedding(300, 64).cuda()
        with torch.no_grad():
            e.weight.copy_(w0)
        e.enable_fused_optimizer("rowwise_adagrad", 0.05)
        return e

    def step(e):
        e(ids).float().square().sum().backward()

    e_graph, e_eager = make(), make()
    for _ in range(3):
        step(e_graph)
        step(e_eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step(e_graph)
    assert torch.equal(e_graph.weight, e_eager.weight), "capture ran the step"
    g.replay()
    step(e_eager)
    torch.cuda.synchronize()
    assert not torch.equal(e_eager.weight.detach().cpu(), w0)
    assert torch.equal(e_graph._fused_state, e_eager._fused_state)
    assert torch.equal(e_graph.weight, e_eager.weight)


@pytest.mark.gpu
@requires_gpu
def test_rowwise_state_isolation():
    """SGD leaves a [vocab] state alone; row-wise Adagrad changes the state
    of touched rows only."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"].cuda(), case["splits"].cuda()
    touched = torch.bincount(case["ids_hot"], minlength=_HELPER_VOCAB) > 0
    assert touched.any() and not touched.all()
    lr = torch.tensor([_LR], device="cuda")
    uniq = torch.unique(case["ids_hot"])
    for width in (33, 68):
        table, grad = _helper_dense(width)
        rows = _dense_grad_ref(grad, case["ids_hot"], case, "sum",
                               torch.float32)[uniq].contiguous().cuda()
        state = torch.ones(_HELPER_VOCAB, device="cuda")
        ext.csr_fused_optimizer_apply(table.cuda(), state, ids, splits,
                                      grad.cuda(), lr, False, False, _EPS)
        ext.sparse_row_update(table.cuda(), state, uniq.cuda(), rows, _LR,
                              _EPS, False)
        assert bool((state == 1.0).all()), "SGD touched the state"
        for call in ("fused", "rows"):
            w = table.cuda()
            state = torch.ones(_HELPER_VOCAB, device="cuda")
            if call == "fused":
                ext.csr_fused_optimizer_apply(w, state, ids, splits,
                                              grad.cuda(), lr, False, True,
                                              _EPS)
            else:
                ext.sparse_row_update(w, state, uniq.cuda(), rows, _LR, _EPS,
                                      True)
            state, w = state.cpu(), w.cpu()
            assert bool((state[~touched] == 1.0).all())
            assert bool((state[touched] > 1.0).all())
            assert torch.equal(w[~touched], table[~touched])
