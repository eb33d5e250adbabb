"""int4 row-wise quantized embedding tables: quantizer, lookups, layers.

Storage (fixed): uint8 ``[vocab, width / 2 + 4]``; row i holds width / 2
bytes of nibbles (column 2j in the low nibble of byte j, column 2j + 1 in the
high one), then fp16 scale[i], then fp16 bias[i], and stands for
``scale[i] * q[i, c] + bias[i]`` — the bytes that
``torch.ops.quantized.embedding_bag_4bit_prepack`` writes, which is the oracle
here: the forward tests read tables packed by torch, not by this project.

Forward bound: the derived one of test_quantized_lookup.py, unchanged.  The
reference is float64 over the same packed bytes, ``ref[r, c] = c_r * sum_k
w_k * (scale_k * q_kc + bias_k)`` with scale and bias widened from their
stored fp16, c_r = 1 (sum) or 1/len_r (mean), ids outside [0, vocab) skipped,
and per output element

    tol = 2 * (len_r + 3) * 2**-24 * c_r * sum_k |w_k| * (scale_k * q_kc + |bias_k|)

in float64, valid for any summation order and for the factored form; a bf16
result adds ``2**-8 * |ref|``.  Where tol == 0 (empty bags, bags of only
out-of-range ids) the result must be exactly 0.  Measured worst error / bound
on these shapes: 0.16 for the kernel with fp32 out, 0.996 with bf16 out (2**-8
is exactly bf16's unit roundoff), 0.07 for the CPU path on dense ids.

Quantizer conditions, per row, with s and b the stored scale and bias: the
four tail bytes are torch's, bit for bit; nibbles differ from torch's by at
most 1; ``|s * q + b - x| <= 0.5 * s + 2**-10 * (|b| + 16 * s)`` in float64
(0.5 from round-to-nearest, the rest covers the fp16 rounding of b and s and
the clamps they cause); on rows with max > min the maximum maps to 15 and the
minimum to 0; a constant row (of an fp16-representable value, so that the
range is 0) is all-zero nibbles with scale 1.0.  torch's prepack is held to
the same conditions.  Measured: torch's bytes, the CPU path and the kernel all
reach 0.96 of the rounding bound, and no nibble differs from torch's.

The kernel tests run on the case test_gpu.py builds for the shared
gather-reduce helpers: 37 bags over vocab 50, lengths 0..7 plus one of 300
(the long path, three chunks), out-of-range ids in short bags and in every
chunk of the long one.  Widths 8..128 are lane tiles of 1..16, 136 is 17
lanes in a 32-lane tile, 264 is 33 lanes in a 64-lane tile, 512 a full
64-lane tile, 520 the column loop.
"""

import copy
import functools
import os
import re
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

_WIDTHS = [8, 16, 32, 64, 128, 136, 264, 512, 520]
_U = 2.0 ** -24
_CONST_ROW, _MIN_ROW, _SHIFT_ROW = 7, 12, 21
_FP16_ONE = torch.tensor([0x00, 0x3C], dtype=torch.uint8)


def _prepack(x):
    return torch.ops.quantized.embedding_bag_4bit_prepack(x)


# --------------------------------------------------------------------------
# Packed tables and the float64 reference
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _packed(width):
    """The N(0,1) [50, width] table of test_gpu.py, packed by torch."""
    return _prepack(_helper_dense(width)[0])


def _unpack(packed):
    """(q, scale, bias): float64 [n, width], [n, 1], [n, 1]."""
    half = packed.shape[1] - 4
    nib = packed[:, :half]
    q = torch.stack([nib & 0xF, nib >> 4], dim=2).reshape(-1, 2 * half)
    tail = packed[:, half:].contiguous().view(torch.float16).double()
    return q.double(), tail[:, 0:1], tail[:, 1:2]


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


def _dense_case(weighted):
    """[9, 5] ids with out-of-range entries, same-shape weights."""
    g = torch.Generator().manual_seed(99)
    ids = torch.randint(0, _HELPER_VOCAB, (9, 5), generator=g)
    ids[0, 0], ids[4, 2], ids[8, 4] = -1, _HELPER_VOCAB, _HELPER_VOCAB + 7
    ids[6] = -3                      # a bag of only out-of-range ids
    w = torch.rand(9, 5, generator=g) * 3 - 1.5 if weighted else None
    return ids, w


# --------------------------------------------------------------------------
# 1. Quantizer
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _quantizer_input(width):
    """N(0,1) [50, width] with a constant row, a row whose minimum is not
    fp16-representable and a row shifted to mean -40."""
    x = _helper_dense(width)[0].clone()
    x[_CONST_ROW] = -0.75                   # fp16-representable: range == 0
    x[_MIN_ROW].clamp_(min=-0.9)
    x[_MIN_ROW, 3] = -(1 + 2.0 ** -12)      # fp16 keeps 10 fraction bits
    x[_SHIFT_ROW] -= 40
    assert float(x[_MIN_ROW].min().half().float()) != float(x[_MIN_ROW].min())
    return x


def _check_quantizer(what, x, packed):
    """The quantizer conditions of the module docstring; x is fp32."""
    n, width = x.shape
    assert packed.dtype == torch.uint8 and packed.shape == (n, width // 2 + 4)
    packed = packed.cpu()
    q, scale, bias = _unpack(packed)
    err = (scale * q + bias - x.double()).abs()
    bound = 0.5 * scale + 2.0 ** -10 * (bias.abs() + 16 * scale)
    print(f"{what}: worst |deq - x| / bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all()), f"{what}: rounding bound"
    lo, hi = x.min(dim=1).values, x.max(dim=1).values
    rows = torch.arange(n)
    spread = hi > lo
    assert bool((q[rows, x.argmax(dim=1)][spread] == 15).all()), \
        f"{what}: max -> 15"
    assert bool((q[rows, x.argmin(dim=1)][spread] == 0).all()), \
        f"{what}: min -> 0"
    for r in rows[~spread].tolist():
        assert bool((packed[r, :width // 2] == 0).all()), \
            f"{what}: constant row {r} stores zero nibbles"
        assert torch.equal(packed[r, width // 2:width // 2 + 2], _FP16_ONE), \
            f"{what}: constant row {r} stores scale 1.0"


def _compare_to_torch(what, x, packed):
    """scale and bias are torch's bits; nibbles differ by at most 1."""
    half = x.shape[1] // 2
    theirs = _prepack(x)
    packed = packed.cpu()
    assert torch.equal(packed[:, half:], theirs[:, half:]), \
        f"{what}: scale and bias bytes equal torch's"
    d = (_unpack(packed)[0] - _unpack(theirs)[0]).abs()
    print(f"{what}: {int((d != 0).sum())} of {d.numel()} nibbles differ from "
          f"torch's")
    assert int(d.max()) <= 1


@pytest.mark.parametrize("width", _WIDTHS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quantizer_properties_cpu(dtype, width):
    from distributed_embeddings_amd import quantize_rowwise_int4
    src = _quantizer_input(width).to(dtype)
    x = src.float()
    assert bool((x[_CONST_ROW] == x[_CONST_ROW, 0]).all())
    packed = quantize_rowwise_int4(src)
    _check_quantizer(f"ours {dtype} w{width}", x, packed)
    _compare_to_torch(f"ours {dtype} w{width}", x, packed)
    _check_quantizer(f"torch {dtype} w{width}", x, _prepack(x))
    # chunked conversion writes the same bytes
    assert torch.equal(quantize_rowwise_int4(src, chunk_rows=7), packed)


def test_quantizer_rejects_bad_input_cpu():
    from distributed_embeddings_amd import quantize_rowwise_int4
    for width in (4, 12, 0):
        with pytest.raises(ValueError, match="multiple of 8"):
            quantize_rowwise_int4(torch.zeros(3, width))
    with pytest.raises(ValueError, match="fp32 or bf16"):
        quantize_rowwise_int4(torch.zeros(3, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        quantize_rowwise_int4(torch.zeros(16))
    assert quantize_rowwise_int4(torch.zeros(0, 16)).shape == (0, 12)


# --------------------------------------------------------------------------
# 2. Layout
# --------------------------------------------------------------------------

@pytest.mark.parametrize("width", _WIDTHS)
def test_layout_matches_torch_unpack_cpu(width):
    from distributed_embeddings_amd import dequantize_rowwise_int4
    packed = _packed(width)
    ours = dequantize_rowwise_int4(packed)
    theirs = torch.ops.quantized.embedding_bag_4bit_unpack(packed)
    assert ours.dtype == torch.float32 and ours.shape == theirs.shape
    inf = torch.full_like(theirs, float("inf"))
    ulp = torch.maximum(torch.nextafter(theirs, inf) - theirs,
                        theirs - torch.nextafter(theirs, -inf))
    assert bool(((ours - theirs).abs() <= ulp).all())
    # Constant rows.  An fp16-representable value has range == 0 and comes
    # back exactly; any other value x leaves range = x - fp16(x) != 0 (of
    # either sign) and takes the general path, in torch as here.
    from distributed_embeddings_amd import quantize_rowwise_int4
    x = torch.stack([torch.full((width,), v) for v in (-0.75, 1.2345, 0.37)])
    ours = quantize_rowwise_int4(x)
    assert torch.equal(ours, _prepack(x))
    assert torch.equal(dequantize_rowwise_int4(ours)[0], x[0])


# --------------------------------------------------------------------------
# 3. The op on the CPU, every input kind
# --------------------------------------------------------------------------

@pytest.mark.parametrize("width", _WIDTHS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_int4_lookup_cpu(combiner, weighted, width):
    from distributed_embeddings_amd import Ragged, quantized_embedding_lookup
    packed = _packed(width)
    tag = f"{combiner} w={weighted} width {width}"

    ids, splits, w = _ragged_case(weighted)
    ref, tol = _ref_tol(packed, ids, splits, combiner, w)
    out = quantized_embedding_lookup(packed, Ragged(ids, splits, w), combiner,
                                     bits=4)
    assert out.dtype == torch.float32 and not out.requires_grad
    assert out.shape == (splits.numel() - 1, width)
    _assert_bound(f"ragged {tag}", out, ref, tol)

    dids, dw = _dense_case(weighted)
    dsplits = torch.arange(10) * 5
    ref, tol = _ref_tol(packed, dids.reshape(-1), dsplits, combiner,
                        None if dw is None else dw.reshape(-1))
    out = quantized_embedding_lookup(packed, dids, combiner,
                                     per_sample_weights=dw, bits=4)
    _assert_bound(f"dense {tag}", out, ref, tol)
    assert bool((out[6] == 0).all())
    outb = quantized_embedding_lookup(packed, dids, combiner,
                                      per_sample_weights=dw,
                                      out_dtype=torch.bfloat16, bits=4)
    assert outb.dtype == torch.bfloat16
    _assert_bound(f"dense bf16 {tag}", outb, ref, tol + 2.0 ** -8 * ref.abs())


@pytest.mark.parametrize("width", _WIDTHS)
def test_int4_lookup_no_combiner_cpu(width):
    from distributed_embeddings_amd import quantized_embedding_lookup
    packed = _packed(width)
    ids = _dense_case(False)[0]
    flat = ids.reshape(-1)
    ref, tol = _ref_tol(packed, flat, torch.arange(flat.numel() + 1), "sum")
    out = quantized_embedding_lookup(packed, ids, bits=4)
    assert out.shape == (9, 5, width) and not out.requires_grad
    _assert_bound(f"no combiner width {width}", out.reshape(-1, width), ref,
                  tol)


def test_bits_is_explicit_cpu():
    """An int4 table of width 24 has the shape of an int8 table of width 8:
    only ``bits`` tells them apart, and only 4 and 8 exist."""
    from distributed_embeddings_amd import quantized_embedding_lookup
    packed = _prepack(_helper_dense(24)[0])
    assert packed.shape == (_HELPER_VOCAB, 16)
    ids = torch.tensor([[1, 2]])
    assert quantized_embedding_lookup(packed, ids, "sum", bits=4).shape == (1, 24)
    assert quantized_embedding_lookup(packed, ids, "sum").shape == (1, 8)
    for bits in (2, 16, None):
        with pytest.raises(ValueError, match="bits"):
            quantized_embedding_lookup(packed, ids, "sum", bits=bits)
    with pytest.raises(ValueError, match="multiple of 8"):
        quantized_embedding_lookup(packed[:, :10], ids, "sum", bits=4)


def test_all_ids_out_of_range_cpu():
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            quantize_rowwise_int4,
                                            quantized_embedding_lookup)
    packed = quantize_rowwise_int4(_helper_dense(16)[0][:10].contiguous())
    ids = torch.tensor([[-1, 10], [11, 12]])
    w = torch.tensor([[0.5, -1.0], [2.0, 1.0]])
    for combiner in ("sum", "mean"):
        for weights in (None, w):
            out = quantized_embedding_lookup(packed, ids, combiner,
                                             per_sample_weights=weights,
                                             bits=4)
            assert out.shape == (2, 16) and bool((out == 0).all())
    out = quantized_embedding_lookup(
        packed, Ragged.from_lists([[10, -1, 99], [], [10]]), "sum", bits=4)
    assert out.shape == (3, 16) and bool((out == 0).all())
    out = quantized_embedding_lookup(packed, torch.tensor([10, -4]), bits=4)
    assert out.shape == (2, 16) and bool((out == 0).all())
    layer = Embedding.from_quantized(packed, "mean", bits=4)
    out = layer.csr_lookup(torch.tensor([10, 11, -1]),
                           torch.tensor([0, 2, 3]), "mean")
    assert out.shape == (2, 16) and bool((out == 0).all())


# --------------------------------------------------------------------------
# 4. Layer
# --------------------------------------------------------------------------

def _lookup_over(table, ids, splits, combiner, w):
    """float64 lookup over a dense table: ids outside the table skipped."""
    lengths = splits[1:] - splits[:-1]
    valid = ((ids >= 0) & (ids < table.shape[0])).double().unsqueeze(1)
    rows = table.double()[ids.clamp(0, table.shape[0] - 1)] * valid
    if w is not None:
        rows = rows * w.double().unsqueeze(1)
    seg = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    out = torch.zeros(lengths.numel(), table.shape[1], dtype=torch.float64)
    out.index_add_(0, seg, rows)
    if combiner == "mean":
        out = out / lengths.clamp(min=1).double().unsqueeze(1)
    return out


def _check_quantized_layer(width, device):
    """quantize_(bits=4) on `device`: storage, and the output against the
    float64 lookup over dequantized_weight() within the forward bound."""
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            quantize_rowwise_int4)
    table = _helper_dense(width)[0]
    layer = Embedding(_HELPER_VOCAB, width, combiner="mean").to(device)
    with torch.no_grad():
        layer.weight.copy_(table)
    assert layer.quantize_(bits=4) is layer and layer.quantized
    assert layer.quantized_bits == 4
    assert "weight" not in dict(layer.named_parameters())
    assert not hasattr(layer, "weight")
    assert layer.qweight.dtype == torch.uint8
    assert layer.qweight.device.type == torch.device(device).type
    assert layer.qweight.shape == (_HELPER_VOCAB, width // 2 + 4)
    assert torch.equal(layer.qweight,
                       quantize_rowwise_int4(table.to(device)))
    assert "quantized=int4" in repr(layer)
    assert layer.quantize_(bits=4) is layer         # same format: a no-op
    with pytest.raises(RuntimeError, match="int4"):
        layer.quantize_(bits=8)
    deq = layer.dequantized_weight()
    assert deq.dtype == torch.float32 and deq.shape == (_HELPER_VOCAB, width)
    packed = layer.qweight.cpu()

    ids, splits, w = _ragged_case(True)
    for weights in (None, w):
        _, tol = _ref_tol(packed, ids, splits, "mean", weights)
        ref = _lookup_over(deq.cpu(), ids, splits, "mean", weights)
        out = layer(Ragged(ids, splits, weights).to(device))
        assert not out.requires_grad
        _assert_bound(f"layer ragged w{width} {device}", out, ref, tol)
    dids, dw = _dense_case(True)
    dsplits = torch.arange(10) * 5
    _, tol = _ref_tol(packed, dids.reshape(-1), dsplits, "mean",
                      dw.reshape(-1))
    ref = _lookup_over(deq.cpu(), dids.reshape(-1), dsplits, "mean",
                       dw.reshape(-1))
    _assert_bound(f"layer dense w{width} {device}",
                  layer(dids.to(device), dw.to(device)), ref, tol)
    assert layer(dids.view(3, 3, 5).to(device)).shape == (3, 3, width)
    outb = layer.csr_lookup(ids.to(device), splits.to(device), "sum",
                            out_dtype=torch.bfloat16)
    assert outb.dtype == torch.bfloat16
    return layer


@pytest.mark.parametrize("width", [32, 136])
def test_int4_layer_cpu(width):
    from distributed_embeddings_amd import Embedding, Ragged
    layer = _check_quantized_layer(width, "cpu")
    ids, splits, _ = _ragged_case(False)
    dids = _dense_case(False)[0]

    state = layer.state_dict()
    assert "qweight" in state and "weight" not in state
    other = Embedding.from_quantized(torch.zeros_like(layer.qweight), "mean",
                                     bits=4)
    assert other.output_dim == width and other.quantized_bits == 4
    other.load_state_dict(state)
    assert torch.equal(other.qweight, layer.qweight)
    assert torch.equal(other(Ragged(ids, splits)), layer(Ragged(ids, splits)))
    plain = Embedding.from_quantized(layer.qweight, bits=4)
    assert plain(dids).shape == (9, 5, width)

    for fn in (lambda: layer.enable_fused_optimizer("sgd", 0.1),
               lambda: layer.set_fused_lr(0.1)):
        with pytest.raises(RuntimeError, match="int4"):
            fn()
    training = Embedding(8, 8, combiner="sum").enable_fused_optimizer(
        "sgd", 0.1)
    with pytest.raises(RuntimeError):
        training.quantize_(bits=4)
    with pytest.raises(ValueError, match="multiple of 8"):
        Embedding(8, 12).quantize_(bits=4)
    with pytest.raises(ValueError, match="bits"):
        Embedding(8, 8).quantize_(bits=2)
    with pytest.raises(ValueError, match="multiple of 8"):
        Embedding.from_quantized(torch.zeros(5, 10, dtype=torch.uint8),
                                 bits=4)


# --------------------------------------------------------------------------
# 5. DistributedEmbedding: a dp, a column-sliced, a row-sliced and a
#    CPU-offloaded table
# --------------------------------------------------------------------------

# Table 1 is cut into two width-8 column slices at world 2; with 60 x 16 and
# one 130 x 8 slice (or, at world 1, the whole 130 x 16) on a rank the budget
# of 1040 elements offloads the larger of the two.
_DIST_SIZES, _DIST_WIDTH, _DIST_HOT, _DIST_BATCH = [40, 130, 60, 259], 16, 3, 4
_DIST_PLAN = dict(data_parallel_threshold=40 * 16,
                  column_slice_threshold=130 * 16 // 2 + 1,
                  row_slice_threshold=259 * 16,
                  gpu_embedding_size=130 * 8)


def _local_layers(model):
    return (list(model.dp_layers) + list(model.col_layers)
            + list(model.row_layers))


def _dist_int4_worker(rank, world):
    """Worst err / bound of the int4 model against its fp32 twin.

    The twin holds dequantized_weight() of every quantized layer; a second
    twin holds scale * q + |bias|, so its output is the bound's sum.  Both
    run in fp32; 2**-20 covers the rounding of the bound itself."""
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.ops.embedding_lookup import \
        dequantize_rowwise_int4
    torch.manual_seed(7)
    g = torch.Generator().manual_seed(3)
    tables = [de.Embedding(s, _DIST_WIDTH, "sum") for s in _DIST_SIZES]
    with torch.no_grad():
        for t in tables:
            t.weight.copy_(torch.randn(t.weight.shape, generator=g))
    model = de.DistributedEmbedding(tables, **_DIST_PLAN)
    plan = model.strategy
    assert plan.dp_table_ids == [0] and plan.row_table_ids == [3]
    if world > 1:
        assert len(plan.table_slices[1]) == 2
    twin, mag = copy.deepcopy(model), copy.deepcopy(model)
    assert model.quantize_(bits=4) is model and model.quantized
    offloaded = 0
    with torch.no_grad():
        for lq, lt, lm in zip(_local_layers(model), _local_layers(twin),
                              _local_layers(mag)):
            assert lq.quantized and lq.quantized_bits == 4
            assert lq.qweight.dtype == torch.uint8
            assert lq.qweight.shape[1] == lq.output_dim // 2 + 4
            assert not list(lq.parameters())
            if getattr(lq, "_cpu_offload", False):
                offloaded += 1
                assert lq.qweight.device.type == "cpu"
            lt.weight.copy_(lq.dequantized_weight())
            bias = lq.qweight[:, -2:].contiguous().view(torch.float16).float()
            zero_bias = lq.qweight.clone()
            zero_bias[:, -2:] = 0
            lm.weight.copy_(dequantize_rowwise_int4(zero_bias) + bias.abs())
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
               lambda: model.set_weights([None] * 4)):
        try:
            fn()
        except RuntimeError as e:
            raised += "quantized" in str(e)
    return {"worst": worst, "raised": raised, "offloaded": offloaded}


def test_dist_int4_world1():
    res = _dist_int4_worker(0, 1)
    print(f"world 1: worst err/bound {res['worst']:.3f}")
    assert res["raised"] == 2 and res["offloaded"] == 1


def test_dist_int4_world2():
    results = run_distributed(_dist_int4_worker, world=2)
    for rank, res in enumerate(results):
        print(f"rank {rank}: worst err/bound {res['worst']:.3f}, "
              f"{res['offloaded']} offloaded")
        assert res["raised"] == 2
    assert sum(res["offloaded"] for res in results) >= 1


def test_dist_int4_is_all_or_nothing():
    """A width that int4 cannot hold on a later table refuses the conversion
    before the first table is touched; int8 still takes the model."""
    import distributed_embeddings_amd as de
    model = de.DistributedEmbedding(
        [de.TableConfig(40, 16, "sum"), de.TableConfig(130, 12, "sum")],
        data_parallel_threshold=40 * 16)
    with pytest.raises(ValueError, match="multiple of 8"):
        model.quantize_(bits=4)
    assert not model.quantized
    assert not any(lyr.quantized for lyr in _local_layers(model))
    assert all(hasattr(lyr, "weight") for lyr in _local_layers(model))
    with pytest.raises(ValueError, match="bits"):
        model.quantize_(bits=3)
    model.quantize_()
    assert all(lyr.quantized_bits == 8 for lyr in _local_layers(model))
    with pytest.raises(RuntimeError):
        model.quantize_(bits=4)


# --------------------------------------------------------------------------
# 6-8. Kernels and layer on the device
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_q4_kernel_forward(combiner, weighted):
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
        packed_d = packed.cuda()
        for out_bf16 in (False, True):
            out = ext.csr_lookup_forward_q4(packed_d, ids_d, splits_d,
                                            combiner == "mean", out_bf16, w_d)
            assert out.dtype == (torch.bfloat16 if out_bf16
                                 else torch.float32)
            assert out.shape == (lengths.numel(), width)
            _assert_bound(f"q4 fwd w{width} out_bf16={out_bf16}", out, ref,
                          tol_bf16 if out_bf16 else tol)
            again = ext.csr_lookup_forward_q4(packed_d, ids_d, splits_d,
                                              combiner == "mean", out_bf16,
                                              w_d)
            # the long bag's atomic combine is order-dependent in fp32 out;
            # bf16 out reduces every bag in registers
            rows = slice(None) if out_bf16 else short
            assert torch.equal(out.cpu()[rows], again.cpu()[rows])


@pytest.mark.gpu
@requires_gpu
def test_q4_kernel_input_kinds():
    """Dense, no-combiner, all-out-of-range and empty-table calls through
    the public op on the device."""
    from distributed_embeddings_amd import Ragged, quantized_embedding_lookup
    for width in (8, 136, 520):
        packed = _packed(width)
        packed_d = packed.cuda()
        for weighted in (False, True):
            dids, dw = _dense_case(weighted)
            ref, tol = _ref_tol(packed, dids.reshape(-1), torch.arange(10) * 5,
                                "sum", None if dw is None else dw.reshape(-1))
            out = quantized_embedding_lookup(
                packed_d, dids.cuda(), "sum", bits=4,
                per_sample_weights=None if dw is None else dw.cuda())
            assert out.is_cuda and not out.requires_grad
            _assert_bound(f"dense w{width} weighted={weighted}", out, ref, tol)
        flat = dids.reshape(-1)
        ref, tol = _ref_tol(packed, flat, torch.arange(flat.numel() + 1),
                            "sum")
        out = quantized_embedding_lookup(packed_d, dids.cuda(), bits=4)
        assert out.shape == (9, 5, width)
        _assert_bound(f"no combiner w{width}", out.reshape(-1, width), ref,
                      tol)
        oob = torch.tensor([[-1, _HELPER_VOCAB], [_HELPER_VOCAB + 1, -7]])
        for combiner in ("sum", "mean"):
            out = quantized_embedding_lookup(packed_d, oob.cuda(), combiner,
                                             bits=4)
            assert out.shape == (2, width) and bool((out == 0).all())
        empty = packed_d[:0].contiguous()
        for out_dtype in (None, torch.bfloat16):
            out = quantized_embedding_lookup(
                empty, Ragged.from_lists([[0, 1], [], [3]]).to("cuda"), "sum",
                out_dtype=out_dtype, bits=4)
            assert out.shape == (3, width) and bool((out == 0).all())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_q4_quantize_dequantize_kernels(dtype):
    from distributed_embeddings_amd import (dequantize_rowwise_int4,
                                            quantize_rowwise_int4)
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    for width in _WIDTHS:
        src = _quantizer_input(width).to(dtype)
        x = src.float()
        what = f"device {dtype} w{width}"
        packed = ext.quantize_rows_q4(src.cuda())
        _check_quantizer(what, x, packed)
        _compare_to_torch(what, x, packed)
        assert torch.equal(quantize_rowwise_int4(src.cuda(), chunk_rows=13),
                           packed)
        deq = ext.dequantize_rows_q4(packed)
        assert deq.dtype == torch.float32
        assert torch.equal(deq.cpu(), dequantize_rowwise_int4(packed.cpu()))
        theirs = _packed(width)
        assert torch.equal(ext.dequantize_rows_q4(theirs.cuda()).cpu(),
                           dequantize_rowwise_int4(theirs))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.quantize_rows_q4(torch.zeros(3, 12, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.dequantize_rows_q4(torch.zeros(3, 10, dtype=torch.uint8,
                                           device="cuda"))
    assert ext.quantize_rows_q4(torch.zeros(0, 16, device="cuda")).shape == \
        (0, 12)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("width", [32, 136])
def test_int4_layer_on_device(width):
    _check_quantized_layer(width, "cuda")


@pytest.mark.gpu
@requires_gpu
def test_int4_lookup_graph_replay():
    """The int4 lookup captured in a graph replays to the eager result."""
    from distributed_embeddings_amd import Embedding
    dev = Embedding.from_quantized(_packed(136), "mean", bits=4).cuda()
    dids_d = _dense_case(False)[0].cuda()
    eager = dev(dids_d)
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

def test_serving_example_int4():
    from distributed_embeddings_amd.models.config import \
        CRITEO_1TB_TABLE_SIZES
    res = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "serving.py"),
         "--table-dtype", "int4", "--table-size-cap", "1000",
         "--batch-size", "64", "--iters", "3", "--warmup", "1"],
        capture_output=True, text=True, timeout=600)
    print(res.stdout, res.stderr[-2000:])
    assert res.returncode == 0
    assert "candidates/s" in res.stdout
    m = re.search(r"-> ([0-9.]+) MiB int4 row-wise", res.stdout)
    assert m, "the byte report names the format"
    rows = sum(min(s, 1000) for s in CRITEO_1TB_TABLE_SIZES)
    assert abs(float(m.group(1)) - rows * 68 / 2 ** 20) < 0.06
    assert float(m.group(1)) < rows * 136 / 2 ** 20
