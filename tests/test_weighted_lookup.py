"""Per-sample weights on the embedding lookups, kernels to layers.

With bag r holding positions k in [s_r, e_r), id i_k, weight w_k,
c_r = 1 for sum and 1/len_r for mean (len_r counts every position of the bag),
valid_k = 0 <= i_k < vocab, table T and upstream gradient g:

    out[r] = c_r * sum_{k in r, valid_k} w_k * T[i_k]
    dT[i]  = sum_{k: i_k = i} c_r(k) * w_k * g[r(k)]
    dw_k   = c_r(k) * <g[r(k)], T[i_k]>  if valid_k, else exactly 0

The references below are these formulas written out in float64.

The GPU kernel tests run on the case test_gpu.py builds for the shared
gather-reduce helpers (37 rows, vocab 50, lengths 0..7 plus one row of 300,
widths 3..260, out-of-range ids in short rows and in all three long chunks)
with the weights of ``_case_weights``: |w| < 1.5, mixed signs, 40 exact
zeros.  Tolerances are the per-element bounds derived above
``_HELPER_WIDTHS`` in test_gpu.py: 1e-4 for sums of <= 7 terms, 1e-3 for up
to 300, plus 2**-8 * |ref| where the result is stored as bf16.  A weight
below 1.5 in magnitude scales a term by at most 1.5, which the tenfold margin
of n * eps * max|x| covers.  For dw the bound is the standard dot-product one,

    tol_k = 2 * (width + 2) * 2**-24 * c_r * sum_c |g[r, c] * T[i_k, c]|,

evaluated in float64; it holds for any summation order and for FMA.  Each GPU
test first asserts that the same formula in fp32 on the CPU stays inside the
bound against float64, then holds the kernel to it.
"""

import os
import subprocess
import sys

import pytest
import torch

from test_gpu import (_HELPER_VOCAB, _HELPER_WIDTHS, _assert_within,
                      _helper_case, _helper_dense, _terms_atol)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_LR = 0.125
_EPS = float(torch.tensor(1e-10, dtype=torch.float32))


def _case_weights():
    nnz = int(_helper_case()["splits"][-1])
    g = torch.Generator().manual_seed(4242)
    w = torch.rand(nnz, generator=g) * 3 - 1.5
    w[::11] = 0
    assert nnz == 436 and int((w == 0).sum()) == 40
    return w


# --------------------------------------------------------------------------
# The formulas, in `dtype`
# --------------------------------------------------------------------------

def _geometry(ids, splits, vocab):
    lengths = splits[1:] - splits[:-1]
    row_of = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    valid = (ids >= 0) & (ids < vocab)
    return lengths, row_of, valid


def _c(lengths, row_of, combiner, dtype):
    """c_r per position."""
    if combiner == "mean":
        return 1.0 / lengths.to(dtype)[row_of]
    return torch.ones(row_of.numel(), dtype=dtype)


def _forward_ref(table, ids, splits, w, combiner, dtype=torch.float64):
    lengths, row_of, valid = _geometry(ids, splits, table.shape[0])
    rows = table.to(dtype)[ids.clamp(0, table.shape[0] - 1)]
    scale = w.to(dtype) * valid * _c(lengths, row_of, combiner, dtype)
    out = torch.zeros(lengths.numel(), table.shape[1], dtype=dtype)
    return out.index_add_(0, row_of, rows * scale.unsqueeze(1))


def _dense_grad_ref(grad, ids, splits, w, vocab, combiner,
                    dtype=torch.float64):
    """[vocab, width] weighted summed gradient."""
    lengths, row_of, valid = _geometry(ids, splits, vocab)
    scale = w.to(dtype) * _c(lengths, row_of, combiner, dtype)
    rows = grad.to(dtype)[row_of] * scale.unsqueeze(1)
    dense = torch.zeros(vocab, grad.shape[1], dtype=dtype)
    return dense.index_add_(0, ids[valid], rows[valid])


def _dw_ref(grad, table, ids, splits, combiner, dtype=torch.float64):
    """(dw, tol): dw in `dtype`, tol_k always in float64."""
    lengths, row_of, valid = _geometry(ids, splits, table.shape[0])
    safe = ids.clamp(0, table.shape[0] - 1)
    c = _c(lengths, row_of, combiner, dtype)
    dw = (grad.to(dtype)[row_of] * table.to(dtype)[safe]).sum(dim=1) * c
    dw = torch.where(valid, dw, torch.zeros_like(dw))
    mag = (grad.double()[row_of] * table.double()[safe]).abs().sum(dim=1)
    tol = (2.0 * (table.shape[1] + 2) * 2.0 ** -24
           * _c(lengths, row_of, combiner, torch.float64) * mag)
    return dw, torch.where(valid, tol, torch.zeros_like(tol))


def _assert_dw(what, got, ref, tol):
    _assert_within(what, got.unsqueeze(1), ref.unsqueeze(1),
                   tol.unsqueeze(1).clamp(min=1e-300))


# --------------------------------------------------------------------------
# GPU, kernel level
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_kernel_forward(combiner):
    from distributed_embeddings_amd.ops import _backend
    from distributed_embeddings_amd.ops.embedding_lookup import _csr_lookup_ref
    ext = _backend.ops()
    case = _helper_case()
    ids, splits, w = case["ids_oob"], case["splits"], _case_weights()
    atol = _terms_atol(case["lengths"])
    nonempty = case["lengths"] > 0
    for width in _HELPER_WIDTHS:
        for tdt in (torch.float32, torch.bfloat16):
            table = _helper_dense(width)[0].to(tdt)
            ref = _forward_ref(table, ids, splits, w, combiner)
            plain = _forward_ref(table, ids, splits, torch.ones_like(w),
                                 combiner)
            # a kernel that ignores the weights cannot pass: on every
            # non-empty row the two references differ by far more than the
            # widest tolerance used below
            gap = (ref - plain).abs().max(dim=1).values
            widest = (atol + 2.0 ** -8 * ref.abs()).max(dim=1).values
            assert bool((gap[nonempty] > 10 * widest[nonempty]).all())
            _assert_within(f"cpu fp32 w{width} {tdt}",
                           _csr_lookup_ref(table, ids, splits, combiner, w),
                           ref, atol)
            for out_bf16 in (False, True):
                out = ext.csr_lookup_forward(table.cuda(), ids.cuda(),
                                             splits.cuda(), combiner == "mean",
                                             out_bf16, w.cuda())
                assert out.dtype == (torch.bfloat16 if out_bf16
                                     else torch.float32)
                tol = atol + (2.0 ** -8 * ref.abs() if out_bf16 else 0.0)
                _assert_within(f"fwd w{width} {tdt} out_bf16={out_bf16}",
                               out, ref, tol)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_kernel_sparse_backward(combiner):
    """ids_hot puts one id 300 times: the weighted long path."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    splits, w = case["splits"], _case_weights()
    for which in ("ids_rand", "ids_hot"):
        ids = case[which]
        uniq, counts = torch.unique(ids, return_counts=True)
        atol = _terms_atol(counts)
        for width in _HELPER_WIDTHS:
            for gdt in (torch.float32, torch.bfloat16):
                grad = _helper_dense(width)[1].to(gdt)
                ref = _dense_grad_ref(grad, ids, splits, w, _HELPER_VOCAB,
                                      combiner)[uniq]
                ref32 = _dense_grad_ref(grad, ids, splits, w, _HELPER_VOCAB,
                                        combiner, torch.float32)[uniq]
                _assert_within(f"cpu fp32 {which} w{width} {gdt}", ref32, ref,
                               atol)
                u, g = ext.csr_lookup_backward(grad.cuda(), ids.cuda(),
                                               splits.cuda(), _HELPER_VOCAB,
                                               combiner == "mean", w.cuda())
                assert torch.equal(u.cpu(), uniq)
                assert g.dtype == torch.float32
                _assert_within(f"bwd {which} w{width} {gdt}", g, ref, atol)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_kernel_weight_grad(combiner):
    from distributed_embeddings_amd.ops import _backend
    from distributed_embeddings_amd.ops.embedding_lookup import (
        _csr_weight_grad_ref)
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_oob"], case["splits"]
    oob = (ids < 0) | (ids >= _HELPER_VOCAB)
    assert int(oob.sum()) == 5
    for width in _HELPER_WIDTHS:
        for tdt in (torch.float32, torch.bfloat16):
            for gdt in (torch.float32, torch.bfloat16):
                table = _helper_dense(width)[0].to(tdt)
                grad = _helper_dense(width)[1].to(gdt)
                ref, tol = _dw_ref(grad, table, ids, splits, combiner)
                tag = f"{combiner} w{width} {tdt} {gdt}"
                cpu = _csr_weight_grad_ref(grad, table, ids, splits, combiner)
                assert cpu.dtype == torch.float32
                _assert_dw(f"cpu fp32 dw {tag}", cpu, ref, tol)
                args = (grad.cuda(), table.cuda(), ids.cuda(), splits.cuda(),
                        combiner == "mean")
                dw = ext.csr_lookup_weight_grad(*args)
                assert dw.dtype == torch.float32 and dw.shape == ids.shape
                _assert_dw(f"dw {tag}", dw, ref, tol)
                assert bool((dw.cpu()[oob] == 0).all())
                assert torch.equal(dw, ext.csr_lookup_weight_grad(*args))


def _adagrad_step(w0, g, lr, eps, adagrad):
    st = 1.0 + g * g
    d = g / (st.sqrt() + eps) if adagrad else g
    return w0.to(g.dtype) - lr * d, st


def _rowwise_step(w0, g, lr, eps):
    st = 1.0 + (g * g).mean(dim=1)
    return w0.to(g.dtype) - lr * g / (st.sqrt() + eps).unsqueeze(1), st


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("method", ["sgd", "adagrad", "rowwise_adagrad"])
def test_kernel_fused_update(method, combiner):
    """Same structure and bounds as test_shared_helpers_fused_update and the
    row-wise GPU test, with the weighted dense gradient as the reference.
    The state starts at 1, so an error in the gradient reaches the weight
    scaled down; max|G| here is 9.5, below the 11 the row-wise state bound
    assumes."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits, w = case["ids_hot"], case["splits"], _case_weights()
    rowwise = method == "rowwise_adagrad"
    lr = torch.tensor([_LR])
    atol = _terms_atol(torch.bincount(ids, minlength=_HELPER_VOCAB))
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        for wdt in (torch.float32, torch.bfloat16):
            for gdt in (torch.float32, torch.bfloat16):
                w0, gq = table.to(wdt), grad.to(gdt)
                g64 = _dense_grad_ref(gq, ids, splits, w, _HELPER_VOCAB,
                                      combiner)
                g32 = _dense_grad_ref(gq, ids, splits, w, _HELPER_VOCAB,
                                      combiner, torch.float32)
                assert float(g64.abs().max()) < 11

                def step(g):
                    if rowwise:
                        wn, st = _rowwise_step(w0, g, _LR, _EPS)
                        return wn, st.unsqueeze(1)
                    return _adagrad_step(w0, g, _LR, _EPS, method != "sgd")

                w_ref, st_ref = step(g64)
                w32, st32 = step(g32)
                w_tol = atol + (2.0 ** -8 * w_ref.abs()
                                if wdt == torch.bfloat16 else 0.0)
                tag = f"{method} {combiner} w{width} {wdt} {gdt}"
                _assert_within(f"cpu fp32 weight {tag}", w32, w_ref, w_tol)
                wt = w0.cuda()
                state = torch.ones(
                    (_HELPER_VOCAB,) if rowwise else (_HELPER_VOCAB, width),
                    device="cuda")
                ext.csr_fused_optimizer_apply(
                    wt, state, ids.cuda(), splits.cuda(), gq.cuda(), lr.cuda(),
                    combiner == "mean", method != "sgd", _EPS, w.cuda())
                _assert_within(f"weight {tag}", wt, w_ref, w_tol)
                if method == "sgd":
                    assert bool((state == 1.0).all()), "SGD touched the state"
                else:
                    _assert_within(f"cpu fp32 state {tag}", st32, st_ref, atol)
                    _assert_within(f"state {tag}", state.reshape(st_ref.shape),
                                   st_ref, atol)


# --------------------------------------------------------------------------
# Layer level: GPU and CPU
# --------------------------------------------------------------------------

_on_gpu = pytest.param("cuda", marks=[pytest.mark.gpu, requires_gpu])


def _layer_case(width=33, rows=24, vocab=40):
    """Bags of 0..7 ids over 40 rows, an empty bag, two out-of-range ids."""
    g = torch.Generator().manual_seed(77)
    lengths = torch.randint(0, 8, (rows,), generator=g)
    lengths[2], lengths[5] = 0, 7
    splits = torch.cat([torch.zeros(1, dtype=torch.long), lengths.cumsum(0)])
    nnz = int(splits[-1])
    ids = torch.randint(0, vocab, (nnz,), generator=g)
    ids[1], ids[nnz - 1] = -3, vocab
    w = torch.rand(nnz, generator=g) * 3 - 1.5
    w[::7] = 0
    table = torch.randn(vocab, width, generator=g)
    up = torch.randn(rows, width, generator=g)
    return dict(ids=ids, splits=splits, w=w, table=table, up=up, vocab=vocab)


def _make_layer(table, combiner, device, dtype=torch.float32):
    from distributed_embeddings_amd import Embedding
    emb = Embedding(table.shape[0], table.shape[1], combiner=combiner,
                    dtype=dtype)
    with torch.no_grad():
        emb.weight.copy_(table)
    return emb.to(device)


@pytest.mark.parametrize("device", ["cpu", _on_gpu])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_layer_autograd_ragged(combiner, device):
    """Embedding on the GPU and its own CPU path, both held to the formulas:
    output, coalesced sparse table gradient, weights.grad."""
    from distributed_embeddings_amd import Ragged
    c = _layer_case()
    emb = _make_layer(c["table"], combiner, device)
    w = c["w"].to(device).requires_grad_(True)
    out = emb(Ragged(c["ids"].to(device), c["splits"].to(device), w))
    out.backward(c["up"].to(device))
    lengths = c["splits"][1:] - c["splits"][:-1]
    _assert_within("out", out.detach(),
                   _forward_ref(c["table"], c["ids"], c["splits"], c["w"],
                                combiner), _terms_atol(lengths))
    g = emb.weight.grad
    assert g.layout == torch.sparse_coo
    valid = (c["ids"] >= 0) & (c["ids"] < c["vocab"])
    uniq, counts = torch.unique(c["ids"][valid], return_counts=True)
    # autograd accumulation may drop the coalesced flag; the content is
    # unique sorted ids all the same
    assert torch.equal(g._indices()[0].cpu(), uniq)
    ref = _dense_grad_ref(c["up"], c["ids"], c["splits"], c["w"], c["vocab"],
                          combiner)[uniq]
    _assert_within("table grad", g._values(), ref, _terms_atol(counts))
    dw_ref, tol = _dw_ref(c["up"], c["table"], c["ids"], c["splits"], combiner)
    assert w.grad.dtype == w.dtype and w.grad.shape == w.shape
    _assert_dw("weights.grad", w.grad, dw_ref, tol)
    assert bool((w.grad.cpu()[~valid] == 0).all())


@pytest.mark.parametrize("device", ["cpu", _on_gpu])
def test_layer_autograd_dense(device):
    """Dense [b, h] ids with per_sample_weights, float64 weights: the
    gradient comes back as float64 and N-D ids reshape alongside."""
    g = torch.Generator().manual_seed(5)
    vocab, width, b, h = 30, 16, 6, 4
    table = torch.randn(vocab, width, generator=g)
    ids = torch.randint(0, vocab, (b, h), generator=g)
    w = (torch.rand(b, h, generator=g, dtype=torch.float64) * 3 - 1.5)
    up = torch.randn(b, width, generator=g)
    splits = torch.arange(b + 1) * h
    emb = _make_layer(table, "mean", device)
    wd = w.to(device).requires_grad_(True)
    out = emb(ids.to(device), wd)
    out.backward(up.to(device))
    _assert_within("out", out.detach(),
                   _forward_ref(table, ids.reshape(-1), splits,
                                w.reshape(-1), "mean"),
                   torch.full((b, 1), 1e-4, dtype=torch.float64))
    dw_ref, tol = _dw_ref(up, table, ids.reshape(-1), splits, "mean")
    assert wd.grad.dtype == torch.float64 and wd.grad.shape == (b, h)
    _assert_dw("weights.grad", wd.grad.reshape(-1), dw_ref, tol)
    # [2, 3, h] ids: same numbers, leading shape restored
    out3 = emb(ids.to(device).view(2, 3, h), wd.detach().view(2, 3, h))
    assert out3.shape == (2, 3, width)
    assert torch.equal(out3.reshape(b, width), out.detach())


@pytest.mark.parametrize("device", ["cpu", _on_gpu])
def test_fused_sgd_weight_grad_reads_prestep_table(device):
    """Fused SGD updates the table during backward; weights.grad has to come
    from the table as the forward read it."""
    from distributed_embeddings_amd import Ragged
    c = _layer_case()
    lr = 0.5
    emb = _make_layer(c["table"], "sum", device)
    emb.enable_fused_optimizer("sgd", lr)
    w = c["w"].to(device).requires_grad_(True)
    emb(Ragged(c["ids"].to(device), c["splits"].to(device), w)).backward(
        c["up"].to(device))
    pre, tol = _dw_ref(c["up"], c["table"], c["ids"], c["splits"], "sum")
    stepped = c["table"].double() - lr * _dense_grad_ref(
        c["up"], c["ids"], c["splits"], c["w"], c["vocab"], "sum")
    post, _ = _dw_ref(c["up"], stepped, c["ids"], c["splits"], "sum")
    # the check can tell the two apart
    assert bool(((pre - post).abs() > tol).any())
    assert emb.weight.grad is None
    valid = (c["ids"] >= 0) & (c["ids"] < c["vocab"])
    _assert_within("stepped table", emb.weight.detach(), stepped,
                   _terms_atol(torch.bincount(c["ids"][valid],
                                              minlength=c["vocab"])))
    _assert_dw("weights.grad", w.grad, pre, tol)


@pytest.mark.gpu
@requires_gpu
def test_hipgraph_capture_weighted_train_step():
    """Weighted fixed-shape Ragged inputs through DistributedEmbedding with
    bf16 outputs and fused SGD: the step captures and replays, and the
    world-1 output (bf16 direct store with per-id weights) matches the
    formula."""
    import distributed_embeddings_amd as de
    torch.manual_seed(23)
    sizes, widths, combiners = [500, 300], [64, 16], ["sum", "mean"]
    with torch.device("cuda"):
        model = de.DistributedEmbedding(
            [de.TableConfig(s, d, c)
             for s, d, c in zip(sizes, widths, combiners)])
    g = torch.Generator().manual_seed(3)
    inputs, cpu_inputs = [], []
    for s in sizes:
        lengths = torch.randint(0, 8, (64,), generator=g)
        ids = torch.randint(0, s, (int(lengths.sum()),), generator=g)
        w = torch.rand(ids.numel(), generator=g) * 3 - 1.5
        rg = de.Ragged.from_row_lengths(ids, lengths, w)
        cpu_inputs.append(rg)
        inputs.append(rg.to("cuda"))
    tables = [torch.as_tensor(t) for t in model.get_weights()]
    with torch.no_grad():
        outs = model(inputs, output_dtype=torch.bfloat16)
    for o, rg, t, comb in zip(outs, cpu_inputs, tables, combiners):
        assert o.dtype == torch.bfloat16
        ref = _forward_ref(t, rg.values, rg.row_splits, rg.weights, comb)
        _assert_within("bf16 weighted output", o, ref,
                       1e-4 + 2.0 ** -8 * ref.abs())
    model.enable_fused_optimizer("sgd", 0.01)

    def step():
        outs = model(inputs, output_dtype=torch.bfloat16)
        loss = sum(o.float().square().sum() for o in outs)
        loss.backward()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    before = [lyr.weight.detach().clone() for lyr in model.col_layers]
    graph.replay()
    torch.cuda.synchronize()
    for b, lyr in zip(before, model.col_layers):
        assert not torch.equal(b, lyr.weight), "replay did not update weights"


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------

# id 1 twice in bag 0, an empty bag, out-of-range ids 11 and -1, a zero and
# a negative weight
_LISTS = [[1, 1, 3], [], [11, 4, 1], [2, -1, 5, 2]]
_WLISTS = [[1.0, -2.0, 0.5], [], [3.0, 0.0, 0.25], [-0.75, 2.0, 1.5, 1.25]]
_VOCAB, _WIDTH = 10, 4


def _hand_case(dtype=torch.float32):
    from distributed_embeddings_amd import Ragged
    g = torch.Generator().manual_seed(11)
    table = torch.randn(_VOCAB, _WIDTH, generator=g).to(dtype)
    up = (torch.arange(1, 5).float().unsqueeze(1)
          * torch.linspace(0.5, 1.5, _WIDTH).unsqueeze(0))
    return table, up, Ragged.from_lists(_LISTS, _WLISTS)


def _close(got, ref, bf16=False, bf16_update=None):
    """fp32 arithmetic on a handful of O(1) terms: 1e-6 + 1e-5 * |ref|.  A
    result stored as bf16 adds one RNE rounding, 2**-8 * |ref| with margin.
    The CPU path of a fused step on a bf16 table rounds the update to bf16
    before it adds it: one more rounding, of the size of the update."""
    ref = ref.double()
    tol = 1e-6 + 1e-5 * ref.abs() + (2.0 ** -8 * ref.abs() if bf16 else 0.0)
    if bf16_update is not None:
        tol = tol + 2.0 ** -8 * bf16_update.abs()
    assert bool(((got.double() - ref).abs() <= tol).all()), (got, ref)


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_cpu_ops_and_layer_match_formulas(combiner, tdt):
    from distributed_embeddings_amd import Ragged, embedding_lookup
    table, up, rg = _hand_case(tdt)
    ref = _forward_ref(table, rg.values, rg.row_splits, rg.weights, combiner)
    assert bool((ref[1] == 0).all())
    g_ref = _dense_grad_ref(up, rg.values, rg.row_splits, rg.weights, _VOCAB,
                            combiner)
    dw_ref, _ = _dw_ref(up, table, rg.values, rg.row_splits, combiner)
    assert float(dw_ref[3]) == 0 and float(dw_ref[7]) == 0  # ids 11 and -1
    for via in ("op", "layer"):
        w = rg.weights.clone().requires_grad_(True)
        x = Ragged(rg.values, rg.row_splits, w)
        if via == "op":
            t = table.clone().requires_grad_(True)
            out = embedding_lookup(t, x, combiner)
        else:
            emb = _make_layer(table, combiner, "cpu", tdt)
            t = emb.weight
            out = emb(x)
        assert out.dtype == torch.float32  # fp32 accumulation and output
        _close(out.detach(), ref)
        out.backward(up.float())
        _close(t.grad.to_dense(), g_ref, bf16=tdt == torch.bfloat16)
        _close(w.grad, dw_ref)
        assert float(w.grad[3]) == 0 and float(w.grad[7]) == 0


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("method", ["sgd", "adagrad", "rowwise_adagrad"])
def test_cpu_fused_optimizers_match_formulas(method, combiner, tdt):
    from distributed_embeddings_amd import Ragged
    table, up, rg = _hand_case(tdt)
    lr, eps = 0.1, 1e-10
    emb = _make_layer(table, combiner, "cpu", tdt)
    emb.enable_fused_optimizer(method, lr, eps)
    w = rg.weights.clone().requires_grad_(True)
    emb(Ragged(rg.values, rg.row_splits, w)).backward(up)
    g = _dense_grad_ref(up, rg.values, rg.row_splits, rg.weights, _VOCAB,
                        combiner)
    if method == "sgd":
        w_ref = table.double() - lr * g
    elif method == "adagrad":
        st = g * g
        w_ref = table.double() - lr * g / (st.sqrt() + eps)
        _close(emb._fused_state, st)
    else:
        st = (g * g).mean(dim=1)
        w_ref = table.double() - lr * g / (st.sqrt() + eps).unsqueeze(1)
        _close(emb._fused_state, st)
    bf16 = tdt == torch.bfloat16
    _close(emb.weight.detach(), w_ref, bf16=bf16,
           bf16_update=w_ref - table.double() if bf16 else None)
    dw_ref, _ = _dw_ref(up, table, rg.values, rg.row_splits, combiner)
    _close(w.grad, dw_ref)  # from the table before the step
    untouched = torch.tensor([0, 6, 7, 8, 9])
    assert torch.equal(emb.weight.detach()[untouched], table[untouched])


def test_ragged_api():
    from distributed_embeddings_amd import Ragged
    v, s = torch.tensor([3, 1, 2]), torch.tensor([0, 2, 3])
    r = Ragged(v, s)
    assert r.weights is None and r.nrows == 2
    assert Ragged.from_row_lengths(v, torch.tensor([2, 1])).weights is None
    assert Ragged.from_lists([[3, 1], [2]]).weights is None
    r = Ragged.from_lists(_LISTS, _WLISTS)
    assert r.weights.dtype == torch.float32
    assert torch.equal(r.weights,
                       torch.tensor([x for row in _WLISTS for x in row]))
    assert torch.equal(r.row_splits, torch.tensor([0, 3, 3, 6, 10]))
    with pytest.raises(ValueError):
        Ragged.from_lists([[1, 2], [3]], [[1.0], [1.0]])
    w = torch.tensor([0.5, 1.5, 2.5], dtype=torch.float64)
    r = Ragged.from_row_lengths(v, torch.tensor([2, 1]), w)
    assert r.weights is w
    ids2d = torch.tensor([[4, 5, 6], [7, 8, 9]])
    w2d = torch.arange(6, dtype=torch.bfloat16).view(2, 3)
    r = Ragged.from_dense(ids2d, w2d)
    assert torch.equal(r.values, ids2d.reshape(-1))
    assert torch.equal(r.row_splits, torch.tensor([0, 3, 6]))
    assert torch.equal(r.weights, w2d.reshape(-1))
    assert Ragged.from_dense(ids2d).weights is None
    with pytest.raises(ValueError):
        Ragged.from_dense(ids2d, w2d[:, :2])
    with pytest.raises(ValueError):
        Ragged.from_dense(ids2d.reshape(-1))
    # .to() moves the weights' device but never their dtype
    moved = r.to(torch.int32)
    assert moved.values.dtype == torch.int32
    assert moved.weights.dtype == torch.bfloat16
    moved = r.to("cpu")
    assert moved.weights.dtype == torch.bfloat16
    assert moved.weights.device == moved.values.device
    assert Ragged(v, s).to("cpu").weights is None


def test_value_errors():
    from distributed_embeddings_amd import Embedding, Ragged, embedding_lookup
    table = torch.randn(_VOCAB, _WIDTH)
    rg = Ragged.from_lists(_LISTS, _WLISTS)
    ones = torch.ones(rg.values.numel())
    with pytest.raises(ValueError):       # both places at once
        embedding_lookup(table, rg, "sum", per_sample_weights=ones)
    with pytest.raises(ValueError):
        Embedding(_VOCAB, _WIDTH, combiner="sum")(rg, ones)
    with pytest.raises(ValueError):       # length mismatch
        embedding_lookup(table, Ragged(rg.values, rg.row_splits, ones[:-1]),
                         "sum")
    with pytest.raises(ValueError):
        Embedding(_VOCAB, _WIDTH, combiner="sum")(
            Ragged(rg.values, rg.row_splits, ones[:-1]))
    ids = torch.tensor([[1, 2], [3, 4]])
    with pytest.raises(ValueError):       # weights without a combiner
        embedding_lookup(table, ids, None, per_sample_weights=torch.ones(2, 2))
    with pytest.raises(ValueError):
        Embedding(_VOCAB, _WIDTH)(ids, torch.ones(2, 2))
    with pytest.raises(ValueError):       # dense shape mismatch
        embedding_lookup(table, ids, "sum", per_sample_weights=torch.ones(2, 3))
    with pytest.raises(ValueError):
        Embedding(_VOCAB, _WIDTH, combiner="sum")(ids, torch.ones(4))
    with pytest.raises(ValueError):       # not a floating tensor
        embedding_lookup(table, ids, "sum",
                         per_sample_weights=torch.ones(2, 2, dtype=torch.long))
    sp = torch.sparse_coo_tensor(torch.tensor([[0, 0, 2], [0, 1, 0]]),
                                 torch.tensor([4, 7, 9]), (3, 2))
    with pytest.raises(ValueError):       # sparse: nnz mismatch
        embedding_lookup(table, sp, "sum", per_sample_weights=torch.ones(2))
    with pytest.raises(ValueError):       # sparse: shape mismatch
        embedding_lookup(table, sp, "sum",
                         per_sample_weights=torch.sparse_coo_tensor(
                             torch.tensor([[0, 0, 2], [0, 1, 0]]),
                             torch.ones(3), (3, 3)))


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_sparse_ids_with_weights_equal_ragged(combiner):
    from distributed_embeddings_amd import Embedding, Ragged, embedding_lookup
    table = torch.randn(_VOCAB, _WIDTH,
                        generator=torch.Generator().manual_seed(2))
    index = torch.tensor([[0, 0, 2, 3, 3, 3], [0, 1, 0, 0, 1, 2]])
    ids = torch.tensor([4, 7, 9, 1, 1, 12])
    w = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.5, 3.0])
    sp = torch.sparse_coo_tensor(index, ids, (4, 3))
    rg = Ragged.from_lists([[4, 7], [], [9], [1, 1, 12]],
                           [[0.5, -1.0], [], [2.0], [0.0, 1.5, 3.0]])
    want = embedding_lookup(table, rg, combiner)
    _close(want, _forward_ref(table, rg.values, rg.row_splits, rg.weights,
                              combiner))
    for weights in (w, torch.sparse_coo_tensor(index, w, (4, 3))):
        assert torch.equal(embedding_lookup(table, sp, combiner, weights),
                           want)
    emb = _make_layer(table, combiner, "cpu")
    assert torch.equal(emb(sp, w), want)
    # the gradient reaches a 1-D weights tensor
    w1 = w.clone().requires_grad_(True)
    embedding_lookup(table, sp, combiner, w1).sum().backward()
    w2 = w.clone().requires_grad_(True)
    embedding_lookup(table, Ragged(rg.values, rg.row_splits, w2),
                     combiner).sum().backward()
    assert torch.equal(w1.grad, w2.grad) and float(w1.grad[5]) == 0


def test_lookup_benchmark_weighted_smoke():
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "lookup_benchmark.py"),
         "--vocab", "2000", "--batch", "64", "--width", "16",
         "--max-hotness", "5", "--weighted"],
        capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert proc.returncode == 0, proc.stdout[-2000:] + proc.stderr[-2000:]
    for line in ("custom fwd", "weighted fwd ", "weighted fwd+grad",
                 "weighted fwd+g+SGD"):
        assert line in proc.stdout
