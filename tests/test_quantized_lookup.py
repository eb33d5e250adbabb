"""int8 row-wise quantized embedding tables: quantizer, lookups, layers.

Storage (fixed): uint8 ``[vocab, width + 8]``; row i holds width bytes
q[i, c], then fp32 scale[i], then fp32 bias[i], and stands for
``scale[i] * q[i, c] + bias[i]`` — the bytes that
``torch.ops.quantized.embedding_bag_byte_prepack`` writes, which is the oracle
here: the forward tests read tables packed by torch, not by this project.

Forward bound (derived, not tuned).  The reference is float64 over the same
packed bytes, ``ref[r, c] = c_r * sum_k w_k * (scale_k * q_kc + bias_k)`` with
scale and bias widened from their stored fp32, c_r = 1 (sum) or 1/len_r
(mean), ids outside [0, vocab) skipped.  Per output element

    tol = 2 * (len_r + 3) * 2**-24 * c_r * sum_k |w_k| * (scale_k * q_kc + |bias_k|)

evaluated in float64: the standard summation bound, valid for any order, with
or without FMA, and whether the kernel dequantizes per term or factors the
bias out of the column sum.  A bf16 result adds ``2**-8 * |ref|`` (one RNE
rounding).  Where tol == 0 (empty bags, bags of only out-of-range ids) the
result must be exactly 0.  ``_terms_atol`` of test_gpu.py is not valid for
the factored form and is not used.  Measured worst error / bound on these
shapes: 0.18 for the CPU fp32 path, 0.15 for the kernel (fp32 out).

Quantizer conditions, per row: bias is bitwise the row minimum; scale is
within 1 ulp of fp32 ``(max - min) / 255``; ``|scale * q + bias - x| <=
(0.5 + 2**-10) * scale`` (0.5 from round-to-nearest, the rest covers the fp32
rounding of ``(x - min) * (255 / range)``); the row maximum maps to 255 and
the minimum to 0; a constant row dequantizes exactly.  torch's prepack is held
to the same conditions.

The kernel tests run on the case test_gpu.py builds for the shared
gather-reduce helpers: 37 bags over vocab 50, lengths 0..7 plus one of 300
(the long path, three chunks), out-of-range ids in short bags and in every
chunk of the long one.  Widths 4..64 are lane tiles of 1..16, 68 the first
non-power-of-two tile, 132 is 33 lanes in a 64-lane tile, 260 the column loop.
"""

import copy
import functools
import os
import subprocess
import sys

import pytest
import torch

from conftest import run_distributed
from test_gpu import (_HELPER_LONG_ROW, _HELPER_VOCAB, _assert_within,
                      _helper_case, _helper_dense)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_WIDTHS = [4, 16, 32, 64, 68, 128, 132, 260]
_U = 2.0 ** -24


# --------------------------------------------------------------------------
# Packed tables and the float64 reference
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _packed(width):
    """The N(0,1) [50, width] table of test_gpu.py, packed by torch."""
    return torch.ops.quantized.embedding_bag_byte_prepack(
        _helper_dense(width)[0])


def _unpack(packed):
    """(q, scale, bias): float64 [n, width], [n, 1], [n, 1]."""
    width = packed.shape[1] - 8
    tail = packed[:, width:].contiguous().view(torch.float32).double()
    return packed[:, :width].double(), tail[:, 0:1], tail[:, 1:2]


def _case_weights():
    """|w| < 1.5, mixed signs, exact zeros (as in test_weighted_lookup.py)."""
    nnz = int(_helper_case()["splits"][-1])
    g = torch.Generator().manual_seed(4242)
    w = torch.rand(nnz, generator=g) * 3 - 1.5
    w[::11] = 0
    return w


def _ref_tol(packed, ids, splits, combiner, w=None, zero_bias=False,
             unit_scale=False):
    """float64 reference and per-element bound of the module docstring."""
    q, scale, bias = _unpack(packed)
    if zero_bias:
        bias = torch.zeros_like(bias)
    if unit_scale:
        scale = torch.ones_like(scale)
    lengths = splits[1:] - splits[:-1]
    n = lengths.numel()
    valid = ((ids >= 0) & (ids < packed.shape[0])).double().unsqueeze(1)
    safe = ids.clamp(0, packed.shape[0] - 1)
    wk = (torch.ones(ids.numel()) if w is None else w).double().unsqueeze(1)
    sq, b = (scale * q)[safe], bias[safe]
    seg = torch.repeat_interleave(torch.arange(n), lengths)
    ref = torch.zeros(n, q.shape[1], dtype=torch.float64)
    ref.index_add_(0, seg, valid * wk * (sq + b))
    mag = torch.zeros_like(ref)
    mag.index_add_(0, seg, valid * wk.abs() * (sq + b.abs()))
    c = torch.ones(n, 1, dtype=torch.float64)
    if combiner == "mean":
        c = 1.0 / lengths.clamp(min=1).double().unsqueeze(1)
    tol = 2 * (lengths.double().unsqueeze(1) + 3) * _U * c * mag
    return c * ref, tol


def _assert_bound(what, got, ref, tol):
    zero = tol.expand_as(ref) == 0
    err = (got.double().cpu() - ref).abs()
    if not bool(zero.all()):
        print(f"{what}: worst err/bound where the bound is not 0: "
              f"{float((err / tol)[~zero].max()):.3f}")
    _assert_within(what, got, ref, tol)
    assert bool((got.double().cpu()[zero] == 0).all()), f"{what}: exact zeros"


def _ragged_case(weighted):
    case = _helper_case()
    return case["ids_oob"], case["splits"], (_case_weights() if weighted
                                             else None)


# --------------------------------------------------------------------------
# 1-2. Quantizer and byte layout (CPU)
# --------------------------------------------------------------------------

def _check_quantizer(what, x, packed):
    """The quantizer conditions of the module docstring; x is fp32."""
    n, width = x.shape
    assert packed.dtype == torch.uint8 and packed.shape == (n, width + 8)
    packed = packed.cpu()
    q, scale, bias = _unpack(packed)
    tail = packed[:, width:].contiguous().view(torch.float32)
    lo = x.min(dim=1).values
    hi = x.max(dim=1).values
    assert torch.equal(tail[:, 1].view(torch.int32), lo.view(torch.int32)), \
        f"{what}: bias is the row minimum, bitwise"
    want = (hi - lo) / 255
    ulp = torch.nextafter(want, torch.full_like(want, float("inf"))) - want
    assert bool(((tail[:, 0] - want).abs() <= ulp).all()), \
        f"{what}: scale within 1 ulp"
    err = (scale * q + bias - x.double()).abs()
    bound = (0.5 + 2.0 ** -10) * scale
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"{what}: worst |deq - x| / scale {ratio * (0.5 + 2.0 ** -10):.5f}")
    assert bool((err <= bound).all()), f"{what}: rounding bound"
    rows = torch.arange(n)
    spread = hi > lo                  # a constant row stores q = 0 throughout
    assert bool((q[rows, x.argmax(dim=1)][spread] == 255).all()), \
        f"{what}: max -> 255"
    assert bool((q[rows, x.argmin(dim=1)] == 0).all()), f"{what}: min -> 0"


def _compare_to_torch(what, x, packed):
    """scale and bias are torch's bits; q bytes differ by at most 1."""
    width = x.shape[1]
    theirs = torch.ops.quantized.embedding_bag_byte_prepack(x)
    packed = packed.cpu()
    assert torch.equal(packed[:, width:], theirs[:, width:]), \
        f"{what}: scale and bias bytes equal torch's"
    d = (packed[:, :width].int() - theirs[:, :width].int()).abs()
    print(f"{what}: {int((d != 0).sum())} of {d.numel()} q bytes differ from "
          f"torch's")
    assert int(d.max()) <= 1


@pytest.mark.parametrize("width", _WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantizer_properties_cpu(dtype, width):
    from distributed_embeddings_amd import quantize_rowwise_int8
    src = _helper_dense(width)[0].to(dtype)
    x = src.float()
    packed = quantize_rowwise_int8(src)
    _check_quantizer(f"ours {dtype} w{width}", x, packed)
    _compare_to_torch(f"ours {dtype} w{width}", x, packed)
    _check_quantizer(f"torch {dtype} w{width}", x,
                     torch.ops.quantized.embedding_bag_byte_prepack(x))
    # chunked conversion writes the same bytes
    assert torch.equal(quantize_rowwise_int8(src, chunk_rows=7), packed)


def test_quantizer_constant_row_and_bad_width_cpu():
    from distributed_embeddings_amd import (dequantize_rowwise_int8,
                                            quantize_rowwise_int8)
    x = _helper_dense(16)[0].clone()
    x[5] = 1.2345
    x[9] = -7.0
    x[11] = 0.0
    packed = quantize_rowwise_int8(x)
    deq = dequantize_rowwise_int8(packed)
    for r in (5, 9, 11):
        assert bool((packed[r, :16] == 0).all())
        assert torch.equal(deq[r], x[r])
        assert bool(torch.isfinite(packed[r, 16:20].view(torch.float32)).all())
    with pytest.raises(ValueError, match="6"):
        quantize_rowwise_int8(torch.zeros(3, 6))


@pytest.mark.parametrize("width", _WIDTHS)
def test_layout_matches_torch_unpack_cpu(width):
    from distributed_embeddings_amd import dequantize_rowwise_int8
    packed = _packed(width)
    ours = dequantize_rowwise_int8(packed)
    theirs = torch.ops.quantized.embedding_bag_byte_unpack(packed)
    assert ours.dtype == torch.float32 and ours.shape == theirs.shape
    inf = torch.full_like(theirs, float("inf"))
    ulp = torch.maximum(torch.nextafter(theirs, inf) - theirs,
                        theirs - torch.nextafter(theirs, -inf))
    assert bool(((ours - theirs).abs() <= ulp).all())


# --------------------------------------------------------------------------
# 3. The op on the CPU, every input kind
# --------------------------------------------------------------------------

def _dense_case(weighted):
    """[9, 5] ids with out-of-range entries, same-shape weights."""
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(0, _HELPER_VOCAB, (9, 5), generator=g)
    ids[0, 0], ids[4, 2], ids[8, 4] = -1, _HELPER_VOCAB, _HELPER_VOCAB + 7
    ids[6] = -3                      # a bag of only out-of-range ids
    w = torch.rand(9, 5, generator=g) * 3 - 1.5 if weighted else None
    return ids, w


@pytest.mark.parametrize("width", _WIDTHS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_quantized_lookup_cpu(combiner, weighted, width):
    from distributed_embeddings_amd import Ragged, quantized_embedding_lookup
    packed = _packed(width)
    tag = f"{combiner} w={weighted} width {width}"

    ids, splits, w = _ragged_case(weighted)
    ref, tol = _ref_tol(packed, ids, splits, combiner, w)
    out = quantized_embedding_lookup(packed, Ragged(ids, splits, w), combiner)
    assert out.dtype == torch.float32 and not out.requires_grad
    _assert_bound(f"ragged {tag}", out, ref, tol)
    if w is not None:   # the weights may come either way
        out2 = quantized_embedding_lookup(packed, Ragged(ids, splits),
                                          combiner, per_sample_weights=w)
        assert torch.equal(out, out2)

    dids, dw = _dense_case(weighted)
    dsplits = torch.arange(10) * 5
    ref, tol = _ref_tol(packed, dids.reshape(-1), dsplits, combiner,
                        None if dw is None else dw.reshape(-1))
    out = quantized_embedding_lookup(packed, dids, combiner,
                                     per_sample_weights=dw)
    _assert_bound(f"dense {tag}", out, ref, tol)
    assert bool((out[6] == 0).all())
    outb = quantized_embedding_lookup(packed, dids, combiner,
                                      per_sample_weights=dw,
                                      out_dtype=torch.bfloat16)
    assert outb.dtype == torch.bfloat16
    _assert_bound(f"dense bf16 {tag}", outb, ref, tol + 2.0 ** -8 * ref.abs())

    # sparse COO: the ragged case as (row, position) coordinates
    lengths = splits[1:] - splits[:-1]
    row_of = _helper_case()["row_of"]
    pos = torch.arange(ids.numel()) - splits[:-1][row_of]
    coords = torch.stack([row_of, pos])
    shape = (lengths.numel(), int(lengths.max()))
    sp = torch.sparse_coo_tensor(coords, ids, shape)
    spw = None if w is None else torch.sparse_coo_tensor(coords, w, shape)
    ref, tol = _ref_tol(packed, ids, splits, combiner, w)
    out = quantized_embedding_lookup(packed, sp, combiner,
                                     per_sample_weights=spw)
    _assert_bound(f"sparse {tag}", out, ref, tol)


def test_all_ids_out_of_range_cpu():
    """A call in which no id is valid: what a row shard sees when the whole
    batch belongs to the other ranks.  Exact zeros, as from the fp32 table."""
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            embedding_lookup,
                                            quantize_rowwise_int8,
                                            quantized_embedding_lookup)
    table = _helper_dense(16)[0][:10].contiguous()
    packed = quantize_rowwise_int8(table)
    ids = torch.tensor([[-1, 10], [11, 12]])
    w = torch.tensor([[0.5, -1.0], [2.0, 1.0]])
    for combiner in ("sum", "mean"):
        want = embedding_lookup(table, ids, combiner)
        assert bool((want == 0).all())
        for weights in (None, w):
            out = quantized_embedding_lookup(packed, ids, combiner,
                                             per_sample_weights=weights)
            assert out.shape == (2, 16) and bool((out == 0).all())
    out = quantized_embedding_lookup(
        packed, Ragged.from_lists([[10, -1, 99], [], [10]]), "sum")
    assert out.shape == (3, 16) and bool((out == 0).all())
    out = quantized_embedding_lookup(packed, torch.tensor([10, -4]))
    assert out.shape == (2, 16) and bool((out == 0).all())
    # a row shard's layer: ids arrive shifted by the shard's row offset
    for combiner in (None, "sum"):
        layer = Embedding.from_quantized(packed, combiner)
        layer._oob_zero = True
        shifted = ids - 100
        out = layer(shifted)
        want_shape = (2, 2, 16) if combiner is None else (2, 16)
        assert out.shape == want_shape and bool((out == 0).all())
    out = layer.csr_lookup(torch.tensor([10, 11, -1]),
                           torch.tensor([0, 2, 3]), "mean")
    assert out.shape == (2, 16) and bool((out == 0).all())


@pytest.mark.parametrize("width", _WIDTHS)
def test_quantized_lookup_no_combiner_cpu(width):
    from distributed_embeddings_amd import quantized_embedding_lookup
    packed = _packed(width)
    ids = _dense_case(False)[0]
    flat = ids.reshape(-1)
    ref, tol = _ref_tol(packed, flat, torch.arange(flat.numel() + 1), "sum")
    out = quantized_embedding_lookup(packed, ids)
    assert out.shape == (9, 5, width) and not out.requires_grad
    _assert_bound(f"no combiner width {width}", out.reshape(-1, width), ref,
                  tol)
    with pytest.raises(ValueError):
        quantized_embedding_lookup(packed, ids, None,
                                   per_sample_weights=torch.ones(9, 5))


# --------------------------------------------------------------------------
# 4. Layer (CPU)
# --------------------------------------------------------------------------

def test_quantized_layer_cpu():
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            quantize_rowwise_int8,
                                            quantized_embedding_lookup)
    width = 68
    table = _helper_dense(width)[0]
    layer = Embedding(_HELPER_VOCAB, width, combiner="mean")
    with torch.no_grad():
        layer.weight.copy_(table)
    assert layer.quantize_() is layer and layer.quantized
    assert "weight" not in dict(layer.named_parameters())
    assert not hasattr(layer, "weight")
    assert layer.qweight.dtype == torch.uint8
    assert layer.qweight.shape == (_HELPER_VOCAB, width + 8)
    assert torch.equal(layer.qweight, quantize_rowwise_int8(table))
    assert "quantized=int8" in repr(layer)
    deq = layer.dequantized_weight()
    assert deq.dtype == torch.float32 and deq.shape == (_HELPER_VOCAB, width)

    ids, splits, w = _ragged_case(True)
    for ragged in (Ragged(ids, splits), Ragged(ids, splits, w)):
        out = layer(ragged)
        assert not out.requires_grad
        assert torch.equal(out, quantized_embedding_lookup(
            layer.qweight, ragged, "mean"))
    dids, dw = _dense_case(True)
    assert torch.equal(layer(dids, dw), quantized_embedding_lookup(
        layer.qweight, dids, "mean", per_sample_weights=dw))
    # N-D ids keep their leading shape
    assert layer(dids.view(3, 3, 5)).shape == (3, 3, width)
    outb = layer.csr_lookup(ids, splits, "sum", out_dtype=torch.bfloat16)
    assert outb.dtype == torch.bfloat16

    state = layer.state_dict()
    assert "qweight" in state and "weight" not in state
    other = Embedding.from_quantized(torch.zeros_like(layer.qweight), "mean")
    other.load_state_dict(state)
    assert torch.equal(other.qweight, layer.qweight)
    assert torch.equal(other(Ragged(ids, splits)), layer(Ragged(ids, splits)))
    plain = Embedding.from_quantized(layer.qweight)
    assert plain(dids).shape == (9, 5, width)

    for fn in (lambda: layer.enable_fused_optimizer("sgd", 0.1),
               lambda: layer.set_fused_lr(0.1)):
        with pytest.raises(RuntimeError):
            fn()
    training = Embedding(8, 4, combiner="sum").enable_fused_optimizer(
        "sgd", 0.1)
    with pytest.raises(RuntimeError):
        training.quantize_()
    with pytest.raises(ValueError, match="6"):
        Embedding(8, 6).quantize_()


# --------------------------------------------------------------------------
# 5. DistributedEmbedding: a dp, a column-sliced and a row-sliced table
# --------------------------------------------------------------------------

_DIST_SIZES, _DIST_WIDTH, _DIST_HOT, _DIST_BATCH = [40, 130, 259], 16, 3, 4
_DIST_PLAN = dict(data_parallel_threshold=40 * 16,
                  column_slice_threshold=130 * 16 // 2 + 1,
                  row_slice_threshold=259 * 16)


def _local_layers(model):
    return (list(model.dp_layers) + list(model.col_layers)
            + list(model.row_layers))


def _dist_quantized_worker(rank, world):
    """Worst err / bound of the quantized model against its fp32 twin.

    The twin holds dequantized_weight() of every quantized layer; a second
    twin holds scale * q + |bias|, so its output is the bound's sum.  Both
    run in fp32; 2**-20 covers the rounding of the bound itself."""
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.ops.embedding_lookup import \
        dequantize_rowwise_int8
    torch.manual_seed(7)
    g = torch.Generator().manual_seed(3)
    tables = [de.Embedding(s, _DIST_WIDTH, "sum") for s in _DIST_SIZES]
    with torch.no_grad():
        for t in tables:
            t.weight.copy_(torch.randn(t.weight.shape, generator=g))
    model = de.DistributedEmbedding(tables, **_DIST_PLAN)
    plan = model.strategy
    assert plan.dp_table_ids == [0] and plan.row_table_ids == [2]
    if world > 1:
        assert len(plan.table_slices[1]) == 2
    twin, mag = copy.deepcopy(model), copy.deepcopy(model)
    assert model.quantize_() is model and model.quantized
    with torch.no_grad():
        for lq, lt, lm in zip(_local_layers(model), _local_layers(twin),
                              _local_layers(mag)):
            assert lq.quantized and lq.qweight.dtype == torch.uint8
            assert not list(lq.parameters())
            lt.weight.copy_(lq.dequantized_weight())
            bias = lq.qweight[:, -4:].contiguous().view(torch.float32)
            zero_bias = lq.qweight.clone()
            zero_bias[:, -4:] = 0
            lm.weight.copy_(dequantize_rowwise_int8(zero_bias) + bias.abs())
    g = torch.Generator().manual_seed(11)
    inputs = [torch.randint(0, s, (world * _DIST_BATCH, _DIST_HOT),
                            generator=g) for s in _DIST_SIZES]
    local = [x[rank * _DIST_BATCH:(rank + 1) * _DIST_BATCH] for x in inputs]
    with torch.no_grad():
        outs, refs, mags = model(local), twin(local), mag(local)
    worst = 0.0
    for o, r, m in zip(outs, refs, mags):
        assert o.shape == (_DIST_BATCH, _DIST_WIDTH) and not o.requires_grad
        tol = 2 * (_DIST_HOT + 3) * _U * m.double() * (1 + 2.0 ** -20)
        err = (o.double() - r.double()).abs()
        assert bool((err <= tol).all())
        worst = max(worst, float((err / tol).max()))
    raised = 0
    for fn in (lambda: model.get_weights(),
               lambda: model.set_weights([None] * 3)):
        try:
            fn()
        except RuntimeError as e:
            raised += "quantized" in str(e)
    return {"worst": worst, "raised": raised}


def test_dist_quantized_world1():
    res = _dist_quantized_worker(0, 1)
    print(f"world 1: worst err/bound {res['worst']:.3f}")
    assert res["raised"] == 2


def test_dist_quantize_is_all_or_nothing():
    """A fused optimizer on a later table refuses the conversion before the
    first table is touched."""
    import distributed_embeddings_amd as de
    model = de.DistributedEmbedding(
        [de.TableConfig(s, _DIST_WIDTH, "sum") for s in _DIST_SIZES],
        **_DIST_PLAN)
    model.enable_fused_optimizer("sgd", 0.1)     # col and row tables, not dp
    with pytest.raises(RuntimeError):
        model.quantize_()
    assert not model.quantized
    assert not any(lyr.quantized for lyr in _local_layers(model))
    assert all(hasattr(lyr, "weight") for lyr in _local_layers(model))


def test_dist_quantized_world2():
    results = run_distributed(_dist_quantized_worker, world=2)
    for rank, res in enumerate(results):
        print(f"rank {rank}: worst err/bound {res['worst']:.3f}")
        assert res["raised"] == 2


# --------------------------------------------------------------------------
# 6-8. Kernels and layer on the device
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_q8_kernel_forward(combiner, weighted):
    from distributed_embeddings_amd import Ragged, quantized_embedding_lookup
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    ids, splits, w = _ragged_case(weighted)
    lengths = splits[1:] - splits[:-1]
    short = torch.arange(lengths.numel()) != _HELPER_LONG_ROW
    ids_d, splits_d = ids.cuda(), splits.cuda()
    w_d = None if w is None else w.cuda()
    for width in _WIDTHS:
        packed = _packed(width)
        ref, tol = _ref_tol(packed, ids, splits, combiner, w)
        tol_bf16 = tol + 2.0 ** -8 * ref.abs()
        # guard: a kernel that drops the bias or the scale cannot pass.  Per
        # non-empty bag the unweighted reference moves by more than 10x the
        # bag's widest tolerance (bf16 out included) when either is dropped.
        uref, utol = _ref_tol(packed, ids, splits, combiner)
        widest = (utol + 2.0 ** -8 * uref.abs()).max(dim=1).values
        for kw in (dict(zero_bias=True), dict(unit_scale=True)):
            alt = _ref_tol(packed, ids, splits, combiner, **kw)[0]
            moved = (alt - uref).abs().max(dim=1).values
            assert bool((moved > 10 * widest)[lengths > 0].all()), (width, kw)
        # The weighted reference under test as well.  Dropping the bias moves
        # a bag by c_r * |sum_k w_k * bias_k| in every column, which mixed
        # signs and the exact zeros of _case_weights can cancel, so the guard
        # is asserted on the bags where that sum keeps at least a quarter of
        # sum_k |w_k * bias_k| — and at least ten of them must remain for the
        # weighted instantiations to be told apart.  (The 300 mixed-sign terms
        # of the long bag cancel below that line; its bias is held by the
        # forward bound alone.)
        if w is not None:
            _, _, bias = _unpack(packed)
            ok = ((ids >= 0) & (ids < _HELPER_VOCAB)).double()
            wb = ok * w.double() * bias[ids.clamp(0, _HELPER_VOCAB - 1), 0]
            net = torch.zeros(lengths.numel(), dtype=torch.float64)
            net.index_add_(0, _helper_case()["row_of"], wb)
            gross = torch.zeros_like(net).index_add_(
                0, _helper_case()["row_of"], wb.abs())
            sel = (gross > 0) & (net.abs() >= 0.25 * gross)
            assert int(sel.sum()) >= 10, (width, int(sel.sum()))
            widest = tol_bf16.max(dim=1).values
            for kw in (dict(zero_bias=True), dict(unit_scale=True)):
                alt = _ref_tol(packed, ids, splits, combiner, w, **kw)[0]
                moved = (alt - ref).abs().max(dim=1).values
                assert bool((moved > 10 * widest)[sel].all()), (width, kw)
        _assert_bound(f"cpu fp32 w{width}", quantized_embedding_lookup(
            packed, Ragged(ids, splits, w), combiner), ref, tol)
        packed_d = packed.cuda()
        for out_bf16 in (False, True):
            out = ext.csr_lookup_forward_q8(packed_d, ids_d, splits_d,
                                            combiner == "mean", out_bf16, w_d)
            assert out.dtype == (torch.bfloat16 if out_bf16
                                 else torch.float32)
            assert out.shape == (lengths.numel(), width)
            _assert_bound(f"q8 fwd w{width} out_bf16={out_bf16}", out, ref,
                          tol_bf16 if out_bf16 else tol)
            again = ext.csr_lookup_forward_q8(packed_d, ids_d, splits_d,
                                              combiner == "mean", out_bf16,
                                              w_d)
            # the long bag's atomic combine is order-dependent in fp32 out;
            # bf16 out reduces every bag in registers
            rows = slice(None) if out_bf16 else short
            assert torch.equal(out.cpu()[rows], again.cpu()[rows])


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q8_quantize_dequantize_kernels(dtype):
    from distributed_embeddings_amd import (dequantize_rowwise_int8,
                                            quantize_rowwise_int8)
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    for width in _WIDTHS:
        src = _helper_dense(width)[0].clone()
        src[7] = -0.75                      # a constant row
        src = src.to(dtype)
        x = src.float()
        what = f"device {dtype} w{width}"
        packed = ext.quantize_rows_q8(src.cuda())
        _check_quantizer(what, x, packed)
        _compare_to_torch(what, x, packed)
        cpu = quantize_rowwise_int8(src)
        assert torch.equal(packed.cpu()[:, width:], cpu[:, width:]), \
            f"{what}: scale and bias bitwise those of the CPU op"
        assert torch.equal(quantize_rowwise_int8(src.cuda(), chunk_rows=13),
                           packed)
        deq = ext.dequantize_rows_q8(packed)
        assert deq.dtype == torch.float32
        assert torch.equal(deq.cpu(), dequantize_rowwise_int8(packed.cpu()))
        assert torch.equal(deq.cpu()[7], x[7])


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("width", [32, 132])
def test_q8_layer_on_device(width):
    from distributed_embeddings_amd import Embedding, Ragged
    packed = _packed(width)
    cpu = Embedding.from_quantized(packed, "mean")
    dev = Embedding.from_quantized(packed, "mean").cuda()
    assert dev.qweight.is_cuda
    ids, splits, w = _ragged_case(True)
    _, tol = _ref_tol(packed, ids, splits, "mean", w)
    ragged = Ragged(ids, splits, w)
    _assert_bound(f"layer ragged w{width}", dev(ragged.to("cuda")),
                  cpu(ragged), tol)
    dids, _ = _dense_case(False)
    _, tol = _ref_tol(packed, dids.reshape(-1), torch.arange(10) * 5, "mean")
    dids_d = dids.cuda()
    eager = dev(dids_d)
    assert not eager.requires_grad
    _assert_bound(f"layer dense w{width}", eager, cpu(dids), tol)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev(dids_d)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = dev(dids_d)
    captured.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, eager)


# --------------------------------------------------------------------------
# 9. The serving example, in a fresh process (GPU when present, else CPU)
# --------------------------------------------------------------------------

def test_serving_example_int8():
    res = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "serving.py"),
         "--table-dtype", "int8", "--table-size-cap", "1000",
         "--batch-size", "64", "--iters", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0
    assert "int8 row-wise" in res.stdout and "candidates/s" in res.stdout
