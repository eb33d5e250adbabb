"""Embedding lookup ops: dispatcher, CSR/ragged/sparse handling, autograd.

MI355X-native equivalent of the reference's op layer
(``/root/reference/distributed_embeddings/python/ops/embedding_lookup_ops.py:37-122``):
the same input-type routing (dense / ragged / sparse / fixed-hotness) and
combiner semantics, re-designed for PyTorch + hand-written HIP kernels.

The hot path is a CSR (values, row_splits) segmented gather-reduce.  On GPU it
runs a hand-written CDNA4 kernel (``csrc/embedding_ops.hip``); on CPU a pure
PyTorch reference implementation with identical numerics is used (it is also
the comparison oracle for the GPU numerics tests).

Gradient contract (parity with reference ``embedding_lookup_ops.py:105-122``,
which emits ``tf.IndexedSlices(unique_grad, unique_ids)``): the backward
produces a **coalesced** ``torch.sparse_coo_tensor`` — unique, sorted ids and
their summed gradient rows — so sparse-capable optimizers (SGD/Adagrad/
SparseAdam) apply O(nnz) updates.
"""

import contextlib
import os
from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _backend


# ---------------------------------------------------------------------------
# Deterministic mode
# ---------------------------------------------------------------------------
#
# The HIP kernels split a segment of more than 128 ids -- a long bag of the
# forward, a hot id of the sparse backward and of the fused optimizers -- into
# 128-id chunks.  By default the chunk partials meet in fp32 atomics, whose
# order, and with it the last bits of the sum, changes from run to run.  In
# deterministic mode each partial goes to a slab row of its own and the rows
# are added in a fixed order (docs/KERNELS.md, "Deterministic mode"), so the
# lookup forward, the sparse backward and the fused optimizers issue no float
# atomic and repeat bit for bit.  The initial value comes from
# DE_DETERMINISTIC=1.  The mode is independent of
# torch.use_deterministic_algorithms.

_deterministic = os.environ.get("DE_DETERMINISTIC", "0") == "1"


def set_deterministic(flag: bool) -> None:
    """Turns the deterministic mode of the lookup kernels on or off.

    With the mode on, long segments (more than 128 ids) are combined in a
    fixed order and the lookup forward (fp32, bf16, int8 and int4 tables),
    the sparse backward and the fused optimizers issue no float atomic: equal
    inputs give equal bits on every run.  bf16-out forwards then split long
    bags like fp32-out ones.  A forward reads the flag when it runs; its
    backward uses the mode its forward saw.

    On the CPU the flag is accepted and changes nothing: those paths already
    add in a fixed order.  Not covered: the value a new key draws in
    ``IntegerLookup``, the reduction order inside collectives, and torch's
    own ops.
    """
    global _deterministic
    _deterministic = bool(flag)


def is_deterministic() -> bool:
    """Whether the deterministic mode is on (see :func:`set_deterministic`)."""
    return _deterministic


@contextlib.contextmanager
def deterministic(flag: bool = True):
    """Context manager: the deterministic mode set to ``flag`` inside the
    block and back to its previous value after it."""
    previous = is_deterministic()
    set_deterministic(flag)
    try:
        yield
    finally:
        set_deterministic(previous)


class Ragged(NamedTuple):
    """A batch of variable-hotness (ragged) id lists in CSR form.

    ``values``: 1-D int tensor of ids, ``row_splits``: int tensor of shape
    ``[num_rows + 1]``; row ``i`` owns ``values[row_splits[i]:row_splits[i+1]]``.

    Equivalent of ``tf.RaggedTensor`` in the reference API (rank-2 only, which
    is all the reference supports — ``embedding.py:129-131``).

    ``weights``: optional 1-D floating tensor aligned with ``values``, one
    weight per id (``per_sample_weights`` of ``torch.nn.EmbeddingBag``,
    ``sp_weights`` of ``tf.nn.embedding_lookup_sparse``).  A lookup computes
    ``c_r * sum_k weights[k] * table[values[k]]`` per row, with ``c_r = 1`` for
    ``sum`` and ``1 / len(row)`` for ``mean`` (the count mean, not a division
    by the weight sum).
    """

    values: torch.Tensor
    row_splits: torch.Tensor
    weights: Optional[torch.Tensor] = None

    @property
    def nrows(self) -> int:
        return self.row_splits.numel() - 1

    @staticmethod
    def from_row_lengths(values: torch.Tensor, row_lengths: torch.Tensor,
                         weights: Optional[torch.Tensor] = None) -> "Ragged":
        zero = torch.zeros(1, dtype=torch.long, device=row_lengths.device)
        splits = torch.cat([zero, row_lengths.cumsum(0)])
        return Ragged(values, splits, weights)

    def row_lengths(self) -> torch.Tensor:
        return self.row_splits[1:] - self.row_splits[:-1]

    @staticmethod
    def from_lists(lists: Sequence[Sequence[int]],
                   weights: Optional[Sequence[Sequence[float]]] = None,
                   device=None) -> "Ragged":
        flat = [i for row in lists for i in row]
        lengths = torch.tensor([len(row) for row in lists], dtype=torch.long, device=device)
        values = torch.tensor(flat, dtype=torch.long, device=device)
        w = None
        if weights is not None:
            if [len(row) for row in weights] != [len(row) for row in lists]:
                raise ValueError("weights must be nested lists of the same "
                                 "shape as the ids")
            w = torch.tensor([x for row in weights for x in row],
                             dtype=torch.float32, device=device)
        return Ragged.from_row_lengths(values, lengths, w)

    @staticmethod
    def from_dense(ids: torch.Tensor,
                   weights: Optional[torch.Tensor] = None) -> "Ragged":
        """Fixed-hotness ``[b, h]`` ids (and same-shape weights) as CSR."""
        if ids.dim() != 2:
            raise ValueError(f"from_dense needs 2-D ids, got {ids.dim()}-D")
        if weights is not None and weights.shape != ids.shape:
            raise ValueError(f"weights shape {tuple(weights.shape)} does not "
                             f"match ids shape {tuple(ids.shape)}")
        b, h = ids.shape
        splits = torch.arange(b + 1, device=ids.device, dtype=torch.long) * h
        return Ragged(ids.reshape(-1), splits,
                      None if weights is None else weights.reshape(-1))

    def to(self, *args, **kwargs) -> "Ragged":
        values = self.values.to(*args, **kwargs)
        w = self.weights
        if w is not None:
            # ids follow the call; weights only change device, never dtype
            w = w.to(values.device)
        return Ragged(values, self.row_splits.to(*args, **kwargs), w)


def row_to_split(indices: torch.Tensor, num_rows: int) -> torch.Tensor:
    """COO (row, pos) index pairs -> CSR row_splits.

    Equivalent of the reference ``RowToSplit`` op (``cc/kernels/
    embedding_lookup_kernels.cu:337-356``: per-output-row binary search).
    ``indices``: ``[nnz, 2]`` with sorted row coordinates in column 0.
    """
    rows = indices[:, 0].contiguous()
    if rows.is_cuda:
        return _backend.ops().row_to_split(rows, num_rows)
    return torch.searchsorted(
        rows, torch.arange(num_rows + 1, device=rows.device, dtype=rows.dtype), side="left"
    )


def _csr_lookup_ref(
    weight: torch.Tensor,
    values: torch.Tensor,
    row_splits: torch.Tensor,
    combiner: str,
    per_id_w: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Pure-PyTorch CSR segmented gather-reduce (fp32 oracle + CPU path).

    Accumulates in fp32 and returns fp32 regardless of the table storage
    dtype (fp32 or bf16) — matching the HIP kernels.  ``per_id_w`` scales
    each gathered row before the sum.
    """
    num_rows = row_splits.numel() - 1
    lengths = row_splits[1:] - row_splits[:-1]
    # OOB ids contribute zero rows (needed by the row-slice parallel path,
    # mirroring reference `_call_row_slice` reliance on OOB-gather-zeros,
    # dist_model_parallel.py:889-904).
    valid = (values >= 0) & (values < weight.shape[0])
    safe = torch.where(valid, values, torch.zeros_like(values))
    rows = weight.index_select(0, safe).float()
    rows = rows * valid.unsqueeze(1).to(rows.dtype)
    if per_id_w is not None:
        rows = rows * per_id_w.to(rows.dtype).unsqueeze(1)
    seg_ids = torch.repeat_interleave(
        torch.arange(num_rows, device=values.device), lengths
    )
    out = torch.zeros(num_rows, weight.shape[1], dtype=rows.dtype, device=rows.device)
    out.index_add_(0, seg_ids, rows)
    if combiner == "mean":
        denom = lengths.clamp(min=1).to(out.dtype).unsqueeze(1)
        out = out / denom
    return out


class _CsrLookup(torch.autograd.Function):
    """CSR segmented gather-reduce with sparse (IndexedSlices-style) grad.

    Forward parity: reference kernels K1-K3 (``embedding_lookup_kernels.cu:
    33-336``).  Backward parity: the sort->unique->segmented-sum pipeline
    (``.cu:603-775``) producing unique ids + summed grad rows.

    ``per_id_w`` (optional, one floating weight per id) scales each row
    before the reduce; its gradient ``dw[k] = c_r * <grad_out[r(k)],
    weight[values[k]]>`` is computed only when autograd asks for it.
    """

    @staticmethod
    def forward(ctx, weight, values, row_splits, combiner, out_dtype=None,
                per_id_w=None):
        w32 = _kernel_weights(per_id_w)
        need_dw = per_id_w is not None and ctx.needs_input_grad[5]
        ctx.save_for_backward(values, row_splits, w32,
                              weight if need_dw else None)
        ctx.combiner = combiner
        ctx.vocab = weight.shape[0]
        ctx.width = weight.shape[1]
        ctx.wdtype = weight.dtype
        ctx.dw_dtype = per_id_w.dtype if need_dw else None
        # the backward runs in the mode the forward saw
        ctx.deterministic = is_deterministic()
        if weight.is_cuda:
            # bf16 out is stored directly by the kernel (no cast kernel);
            # the backward consumes bf16 grads natively too
            return _backend.ops().csr_lookup_forward(
                weight, values, row_splits, combiner == "mean",
                out_dtype == torch.bfloat16, w32,
                deterministic=ctx.deterministic)
        out = _csr_lookup_ref(weight, values, row_splits, combiner, w32)
        return out.to(out_dtype) if out_dtype is not None else out

    @staticmethod
    def backward(ctx, grad_out):
        values, row_splits, w32, weight = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        if grad_out.is_cuda:
            unique_ids, unique_grad = _backend.ops().csr_lookup_backward(
                grad_out, values, row_splits, ctx.vocab,
                ctx.combiner == "mean", w32,
                deterministic=ctx.deterministic
            )
        else:
            unique_ids, unique_grad = _csr_lookup_backward_ref(
                grad_out, values, row_splits, ctx.vocab, ctx.combiner, w32
            )
        grad_weight = torch.sparse_coo_tensor(
            unique_ids.unsqueeze(0),
            unique_grad.to(ctx.wdtype),  # autograd: grad dtype == param dtype
            size=(ctx.vocab, ctx.width),
            is_coalesced=True,
        )
        dw = None
        if ctx.dw_dtype is not None:
            dw = _csr_weight_grad(grad_out, weight.detach(), values,
                                  row_splits, ctx.combiner).to(ctx.dw_dtype)
        return grad_weight, None, None, None, None, dw


def _kernel_weights(per_id_w):
    """The contiguous fp32 [nnz] tensor the kernels take (None stays None)."""
    if per_id_w is None:
        return None
    return per_id_w.detach().to(torch.float32).contiguous()


def _csr_weight_grad(grad_out, weight, values, row_splits, combiner):
    """fp32 [nnz] gradient of the per-id weights, HIP kernel or CPU path."""
    if grad_out.is_cuda:
        return _backend.ops().csr_lookup_weight_grad(
            grad_out, weight, values, row_splits, combiner == "mean")
    return _csr_weight_grad_ref(grad_out, weight, values, row_splits, combiner)


def _csr_weight_grad_ref(grad_out, weight, values, row_splits, combiner):
    """CPU reference: dw[k] = c_r * <grad_out[r(k)], weight[values[k]]> in
    fp32, exactly 0 for an out-of-range id."""
    num_rows = row_splits.numel() - 1
    lengths = (row_splits[1:] - row_splits[:-1]).to(torch.long)
    seg_ids = torch.repeat_interleave(torch.arange(num_rows, device=values.device), lengths)
    valid = (values >= 0) & (values < weight.shape[0])
    safe = torch.where(valid, values, torch.zeros_like(values))
    rows = weight.index_select(0, safe).float()
    dot = (grad_out.float().index_select(0, seg_ids) * rows).sum(dim=1)
    if combiner == "mean":
        dot = dot / lengths.clamp(min=1).to(dot.dtype).index_select(0, seg_ids)
    return torch.where(valid, dot, torch.zeros_like(dot))


def _csr_lookup_backward_ref(grad_out, values, row_splits, vocab, combiner,
                             per_id_w=None):
    """CPU reference backward: unique ids + per-unique summed grad rows."""
    num_rows = row_splits.numel() - 1
    lengths = (row_splits[1:] - row_splits[:-1]).to(torch.long)
    seg_ids = torch.repeat_interleave(torch.arange(num_rows, device=values.device), lengths)
    g = grad_out.index_select(0, seg_ids)  # [nnz, width]
    if combiner == "mean":
        w = 1.0 / lengths.clamp(min=1).to(grad_out.dtype)
        g = g * w.index_select(0, seg_ids).unsqueeze(1)
    if per_id_w is not None:
        g = g * per_id_w.to(g.dtype).unsqueeze(1)
    valid = (values >= 0) & (values < vocab)
    vals = values[valid]
    g = g[valid]
    unique_ids, inverse = torch.unique(vals, sorted=True, return_inverse=True)
    unique_grad = torch.zeros(unique_ids.numel(), grad_out.shape[1],
                              dtype=torch.float32, device=grad_out.device)
    unique_grad.index_add_(0, inverse, g.float())
    return unique_ids, unique_grad


# ---------------------------------------------------------------------------
# Stochastic rounding of optimizer writes to bf16 tables
# ---------------------------------------------------------------------------
#
# A finite fp32 x with bit pattern u is stored as the bf16 ``(u + r) >> 16``
# with 16 random bits r: away from zero with probability low16(u) / 65536,
# unbiased, and a bf16-representable x never moves.  A value above the largest
# finite bf16 may become +-inf, as with round-to-nearest-even.  Inf and NaN
# round to nearest-even.  r depends on (seed, step, o) alone, o being the
# element's offset ``row * width + col`` in the local table:
#
#     key = mix64(seed ^ mix64(step))
#     h   = mix64(key + (o >> 2))
#     r   = (h >> (16 * (o & 3))) & 0xFFFF
#
# with mix64 the splitmix64 finalizer of csrc/embedding_ops.hip.  The numpy
# code below is the definition the HIP kernels are tested against, bit for
# bit, and the CPU path of the feature.

_U64 = (1 << 64) - 1


def mix64_int(k: int) -> int:
    """``mix64`` of csrc/embedding_ops.hip on a Python int (mod 2**64)."""
    k = (k + 0x9E3779B97F4A7C15) & _U64
    k = ((k ^ (k >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    k = ((k ^ (k >> 27)) * 0x94D049BB133111EB) & _U64
    return k ^ (k >> 31)


def to_int64(k: int) -> int:
    """The int64 with the bit pattern of ``k`` mod 2**64."""
    k &= _U64
    return k - (1 << 64) if k >> 63 else k


def _mix64_np(k):
    import numpy as np
    with np.errstate(over="ignore"):
        k = k + np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return k ^ (k >> np.uint64(31))


def stochastic_rounding_bits(seed: int, step: int,
                             offsets: torch.Tensor) -> torch.Tensor:
    """The 16 random bits r of each table offset, as int64 in [0, 65536)."""
    import numpy as np
    o = offsets.detach().cpu().to(torch.int64).contiguous().numpy()
    o = o.astype(np.uint64)
    key = np.uint64(mix64_int((int(seed) & _U64) ^ mix64_int(int(step) & _U64)))
    with np.errstate(over="ignore"):
        h = _mix64_np(key + (o >> np.uint64(2)))
    r = (h >> (np.uint64(16) * (o & np.uint64(3)))) & np.uint64(0xFFFF)
    return torch.from_numpy(r.astype(np.int64))


def _stochastic_round_bf16_ref(x: torch.Tensor, seed: int, step: int,
                               offsets: torch.Tensor) -> torch.Tensor:
    """CPU reference: fp32 ``x`` -> bf16, element ``i`` rounded with the bits
    of table offset ``offsets[i]`` (same shape as ``x``)."""
    x = x.detach().to(torch.float32).contiguous()
    r = stochastic_rounding_bits(seed, step, offsets.reshape(-1)).view(x.shape)
    u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    finite = (u & 0x7F800000) != 0x7F800000
    # inf keeps its top half; NaN keeps it too, quieted (0x7fc00000 ->
    # 0x7fc0, what the device conversion stores).  Done on the bits:
    # torch's own CPU cast gives NaN two different encodings, depending on
    # whether the element falls into a vectorized stretch.
    is_nan = ~finite & ((u & 0x007FFFFF) != 0)
    hi = torch.where(finite, (u + r) >> 16,
                     (u >> 16) | torch.where(is_nan, 0x0040, 0))
    hi = torch.where(hi >= 0x8000, hi - 0x10000, hi).to(torch.int16)
    return hi.view(torch.bfloat16)


def stochastic_round_bf16(x: torch.Tensor, seed: int, step: int = 0,
                          base_offset: int = 0) -> torch.Tensor:
    """fp32 ``x`` -> bf16 by the stochastic rounding the fused optimizers
    apply to bf16 tables: element ``i`` of the flattened ``x`` gets the bits
    of table offset ``base_offset + i`` at ``(seed, step)``.

    A finite value goes to one of its two bf16 neighbours, away from zero
    with probability ``low16(bits) / 65536`` (unbiased; a representable value
    stays).  Inf and NaN round to nearest-even; a finite value above the
    largest finite bf16 may become +-inf.  On the GPU this is a HIP kernel,
    on the CPU the numpy reference of the same function.
    """
    if x.dtype != torch.float32:
        raise ValueError("stochastic_round_bf16 takes an fp32 tensor")
    if base_offset < 0:
        raise ValueError("base_offset must not be negative")
    seed, step = to_int64(int(seed)), to_int64(int(step))
    if x.is_cuda:
        return _backend.ops().stochastic_round_bf16(
            x.detach().contiguous(), seed, step, int(base_offset))
    offsets = torch.arange(x.numel(), dtype=torch.int64) + int(base_offset)
    return _stochastic_round_bf16_ref(x, seed, step, offsets.view(x.shape))


# ---------------------------------------------------------------------------
# Multi-hot expansion and group id packing
# ---------------------------------------------------------------------------
#
# A one-hot id x of feature f becomes a bag of `hotness` ids, a pure function
# of (seed, f, x), all arithmetic mod 2**64:
#
#     key_f  = mix64(seed ^ mix64(f))
#     inner  = mix64(key_f + x)
#     bag[0] = x
#     bag[k] = mix64(inner + k) % vocab        k = 1 .. hotness-1, unsigned
#
# An id outside [0, vocab) goes to every slot unhashed.  The numpy code below
# is the definition and the CPU path; csrc/pack_ids.hip is tested against it
# bit for bit.


def multi_hot_key(seed: int, feature: int) -> int:
    """``key_f`` of the expansion, as a Python int in [0, 2**64)."""
    return mix64_int((int(seed) & _U64) ^ mix64_int(int(feature) & _U64))


def _multi_hot_expand_np(ids: torch.Tensor, vocab: int, hotness: int,
                         key_f: int) -> torch.Tensor:
    import numpy as np
    x = ids.detach().cpu().to(torch.int64).contiguous().numpy()
    xu = x.astype(np.uint64)
    out = np.empty(x.shape + (hotness,), dtype=np.int64)
    out[..., :] = x[..., None]
    valid = xu < np.uint64(vocab)
    with np.errstate(over="ignore"):
        inner = _mix64_np(xu + np.uint64(key_f))
        for k in range(1, hotness):
            hashed = _mix64_np(inner + np.uint64(k)) % np.uint64(vocab)
            out[..., k] = np.where(valid, hashed.astype(np.int64), x)
    return torch.from_numpy(out)


def _check_multi_hot(vocab, hotness) -> None:
    if int(vocab) < 1:
        raise ValueError(f"vocab must be >= 1, got {vocab!r}")
    if int(hotness) < 1:
        raise ValueError(f"hotness must be >= 1, got {hotness!r}")


def multi_hot_expand(ids: torch.Tensor, vocab: int, hotness: int, seed: int,
                     feature: int = 0) -> torch.Tensor:
    """Expands one-hot ``ids`` into bags: int64 ``[*ids.shape, hotness]``.

    Slot 0 of a bag is the id itself; slot ``k`` is
    ``mix64(mix64(key_f + id) + k) % vocab`` with
    ``key_f = mix64(seed ^ mix64(feature))`` (unsigned 64-bit arithmetic,
    ``mix64`` the splitmix64 finalizer the project uses elsewhere).  The bag
    is a pure function of ``(seed, feature, id)``, uniform over the
    vocabulary, and may hold duplicates.  An id outside ``[0, vocab)`` fills
    every slot unhashed.  ``hotness == 1`` returns ``ids[..., None]``.

    On the GPU this is the ``pack_ids`` HIP kernel, on the CPU numpy; the two
    agree bit for bit.
    """
    _check_multi_hot(vocab, hotness)
    return multi_hot_expand_keyed(ids, int(vocab), int(hotness),
                                  multi_hot_key(seed, feature))


def multi_hot_expand_keyed(ids: torch.Tensor, vocab: int, hotness: int,
                           key_f: int) -> torch.Tensor:
    """:func:`multi_hot_expand` with ``key_f`` (:func:`multi_hot_key`)
    already formed."""
    if hotness == 1:
        return ids.to(torch.int64)[..., None]
    if ids.is_cuda:
        flat = pack_ids([(ids.detach().to(torch.int64).contiguous(),
                          hotness, (vocab, key_f), 0)])
        return flat.view(*ids.shape, hotness)
    return _multi_hot_expand_np(ids, vocab, hotness, key_f)


def pack_ids_enabled() -> bool:
    """``DE_PACK_IDS`` (default on): build fused-group id vectors with the
    ``pack_ids`` kernel instead of ``torch.cat`` + offset add."""
    return os.environ.get("DE_PACK_IDS", "1") != "0"


def pack_ids(segments) -> torch.Tensor:
    """The flat int64 id vector of ``segments``, one after the other, in one
    pass of the ``pack_ids`` HIP kernel (``csrc/pack_ids.hip``).

    A segment is ``(src, h_out, expand, offset)``.  With ``expand`` None,
    ``src`` holds ``rows * h_out`` ids and the segment is ``src + offset``.
    With ``expand = (vocab, key_f)``, ``src`` holds one id per row and the
    segment is that id's bag of ``h_out`` ids (:func:`multi_hot_expand`,
    ``key_f`` from :func:`multi_hot_key`) ``+ offset``.  Every ``src`` is a
    contiguous int64 tensor on one GPU.  More segments than one launch holds
    (64) take several launches; empty segments are legal.
    """
    srcs, h_out, expand, vocab, key_f, offset = [], [], [], [], [], []
    for src, h, exp, off in segments:
        srcs.append(src)
        h_out.append(int(h))
        expand.append(exp is not None)
        vocab.append(int(exp[0]) if exp is not None else 0)
        key_f.append(to_int64(int(exp[1])) if exp is not None else 0)
        offset.append(int(off))
    return _backend.ops().pack_ids(srcs, h_out, expand, vocab, key_f, offset)


def pack_ids_reference(segments) -> torch.Tensor:
    """:func:`pack_ids` composed from the numpy expansion, ``torch.cat`` and
    an add, on any device and never through the kernel: the definition the
    kernel is tested against."""
    parts = []
    for src, h, exp, off in segments:
        if exp is not None:
            part = _multi_hot_expand_np(
                src.reshape(-1), int(exp[0]), int(h),
                int(exp[1])).to(src.device).reshape(-1)
        else:
            part = src.reshape(-1)
        parts.append(part + int(off) if int(off) else part)
    return torch.cat(parts)


def _check_sr(sr, weight) -> None:
    if sr is None:
        return
    if weight.dtype != torch.bfloat16:
        raise ValueError("stochastic rounding needs a bf16 table: an fp32 "
                         "table has nothing to round")
    if (sr.dtype != torch.int64 or sr.shape != (2,)
            or sr.device != weight.device):
        raise ValueError("sr must be an int64 [2] tensor (seed, step) on the "
                         "weight's device")


def _write_rows_sr(weight, ids, new_rows, sr) -> None:
    """CPU: writes fp32 ``new_rows`` over the bf16 ``weight[ids]`` (unique
    ids), stochastically rounded at the rows' table offsets, and advances the
    step ``sr[1]``."""
    seed, step = (int(v) for v in sr.tolist())
    width = weight.shape[1]
    offsets = ids.unsqueeze(1) * width + torch.arange(width, dtype=torch.int64)
    weight[ids] = _stochastic_round_bf16_ref(new_rows, seed, step, offsets)
    sr[1] += 1


def check_betas(betas) -> None:
    """Raises ValueError unless both Adam betas lie in ``[0, 1)``."""
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"betas must be two values in [0, 1), got {betas!r}")


def _check_adam(adam, adagrad, state, weight) -> None:
    if adam is None:
        return
    step, beta1, beta2 = adam
    if adagrad:
        raise ValueError("adam and adagrad exclude each other")
    check_betas((beta1, beta2))
    if (state.dtype != torch.float32 or state.device != weight.device
            or state.shape != (2,) + tuple(weight.shape)):
        raise ValueError("lazy Adam needs an fp32 state [2, vocab, width] on "
                         f"the weight's device, got {tuple(state.shape)} "
                         f"{state.dtype} for weight {tuple(weight.shape)}")
    if (step.dtype != torch.int64 or step.shape != (1,)
            or step.device != weight.device):
        raise ValueError("the Adam step must be an int64 [1] tensor on the "
                         "weight's device")


def _lazy_adam_rows(state, ids, g, lr, beta1, beta2, eps, t):
    """Lazy Adam at step ``t`` on the rows ``ids`` (unique) of the fp32 state
    ``[2, vocab, ...]`` with their fp32 summed gradients ``g``: updates ``m``
    and ``v`` of those rows in place and returns the rows' weight delta.  The
    fp32 torch-op form of the update the HIP kernels apply."""
    m = state[0].index_select(0, ids).mul_(beta1).add_(g, alpha=1.0 - beta1)
    v = state[1].index_select(0, ids).mul_(beta2).addcmul_(
        g, g, value=1.0 - beta2)
    state[0].index_copy_(0, ids, m)
    state[1].index_copy_(0, ids, v)
    a_t = lr * (1.0 - beta2 ** t) ** 0.5 / (1.0 - beta1 ** t)
    return m.mul_(-a_t).div_(v.sqrt_().add_(eps))


class _CsrLookupFusedOptimizer(torch.autograd.Function):
    """CSR lookup whose backward applies the optimizer update in place.

    SGD is linear in the grad (order-free up to fp rounding); Adagrad uses
    the same all-device sorted-segment pipeline so per-unique-row sums are
    exact.  No gradient tensor is materialized for the table, there is no
    host sync, and the whole training step becomes hipGraph-capturable.
    ``lr`` is a 1-element fp32 device tensor so schedules can update it
    without touching the graph; ``state`` is the Adagrad accumulator (empty
    tensor for SGD).  With ``adagrad`` set, a 1-D fp32 ``[vocab]`` state
    selects row-wise Adagrad: ``state[r] += mean_c(G[r, c]^2)`` on the summed
    row ``G[r]``, then ``w[r] -= lr * G[r] / (sqrt(state[r]) + eps)``.

    With ``per_id_w`` the gradient of the weights is taken from the table as
    the forward read it: it is computed before the update touches the table.

    ``sr`` (optional, bf16 tables only): int64 ``[2]`` tensor ``(seed, step)``
    on the weight's device.  The updated weights are then stored with
    stochastic rounding (``stochastic_round_bf16`` at the elements' table
    offsets) and every backward that applies an update adds 1 to ``sr[1]`` --
    on the device, so a captured step draws fresh bits on every replay.

    ``adam`` (optional): ``(step, beta1, beta2)`` selects lazy Adam
    (``adagrad`` then has to be false).  ``state`` is fp32
    ``[2, vocab, width]``, ``m`` first, and ``step`` an int64 ``[1]`` tensor
    on the weight's device.  A backward that applies an update first adds 1
    to ``step`` -- on the device, so every replay of a captured step takes
    the next ``t`` -- and then, for every unique in-range id ``u`` with
    summed gradient row ``G[u]``::

        m[u] = b1 m[u] + (1 - b1) G[u]
        v[u] = b2 v[u] + (1 - b2) G[u]^2
        w[u] -= lr sqrt(1 - b2^t) / (1 - b1^t) * m[u] / (sqrt(v[u]) + eps)

    in fp32, which is ``torch.optim.SparseAdam``'s update.  Rows whose id
    does not occur keep ``w``, ``m`` and ``v`` bit for bit.
    """

    @staticmethod
    def forward(ctx, weight, values, row_splits, combiner, lr, state, adagrad,
                eps, out_dtype=None, per_id_w=None, sr=None, adam=None):
        _check_sr(sr, weight)
        _check_adam(adam, adagrad, state, weight)
        w32 = _kernel_weights(per_id_w)
        need_dw = per_id_w is not None and ctx.needs_input_grad[9]
        ctx.save_for_backward(weight, values, row_splits, lr, state, w32)
        # int64 counters the backward itself advances: kept off the saved
        # tensors, whose version check would reject that
        ctx.sr = sr
        ctx.adam = adam
        ctx.combiner = combiner
        ctx.adagrad = adagrad
        ctx.eps = eps
        ctx.dw_dtype = per_id_w.dtype if need_dw else None
        # the backward runs in the mode the forward saw
        ctx.deterministic = is_deterministic()
        if weight.is_cuda:
            return _backend.ops().csr_lookup_forward(
                weight, values, row_splits, combiner == "mean",
                out_dtype == torch.bfloat16, w32,
                deterministic=ctx.deterministic)
        out = _csr_lookup_ref(weight, values, row_splits, combiner, w32)
        return out.to(out_dtype) if out_dtype is not None else out

    @staticmethod
    def backward(ctx, grad_out):
        weight, values, row_splits, lr, state, w32 = ctx.saved_tensors
        sr = ctx.sr
        grad_out = grad_out.contiguous()
        dw = None
        with torch.no_grad():
            if ctx.dw_dtype is not None:
                # before the update: the table as the forward read it
                dw = _csr_weight_grad(grad_out, weight, values, row_splits,
                                      ctx.combiner).to(ctx.dw_dtype)
            adam = ctx.adam
            # the kernels' condition for launching (and advancing the steps)
            launches = values.numel() > 0 and row_splits.numel() > 1
            if weight.is_cuda and adam is not None:
                _backend.ops().csr_fused_optimizer_apply(
                    weight, state, values, row_splits, grad_out, lr,
                    ctx.combiner == "mean", False, ctx.eps, w32, sr,
                    adam_step=adam[0], beta1=adam[1], beta2=adam[2],
                    deterministic=ctx.deterministic)
            elif weight.is_cuda:
                _backend.ops().csr_fused_optimizer_apply(
                    weight, state, values, row_splits, grad_out, lr,
                    ctx.combiner == "mean", ctx.adagrad, ctx.eps, w32, sr,
                    deterministic=ctx.deterministic)
            else:
                unique_ids, unique_grad = _csr_lookup_backward_ref(
                    grad_out.float(), values, row_splits, weight.shape[0],
                    ctx.combiner, w32)
                lr_v = lr.item()
                if adam is not None:
                    delta = None
                    if launches:
                        step = adam[0]
                        step += 1
                        delta = _lazy_adam_rows(
                            state, unique_ids, unique_grad, lr_v, adam[1],
                            adam[2], ctx.eps, int(step))
                elif ctx.adagrad:
                    sq = unique_grad * unique_grad
                    rowwise = state.dim() == 1
                    state.index_add_(0, unique_ids,
                                     sq.mean(dim=1) if rowwise else sq)
                    denom = state.index_select(0, unique_ids).sqrt_().add_(ctx.eps)
                    if rowwise:
                        denom = denom.unsqueeze(1)
                    delta = -lr_v * unique_grad / denom
                else:
                    delta = unique_grad * (-lr_v)
                if delta is None:
                    pass
                elif sr is None:
                    weight.index_add_(0, unique_ids, delta.to(weight.dtype))
                elif launches:
                    rows = weight.index_select(0, unique_ids).float() + delta
                    _write_rows_sr(weight, unique_ids, rows, sr)
        return (None,) * 9 + (dw, None, None)


def csr_lookup_fused_sgd(weight, values, row_splits, combiner, lr,
                         out_dtype=None, per_id_w=None):
    empty = torch.empty(0, dtype=torch.float32, device=weight.device)
    return _CsrLookupFusedOptimizer.apply(weight, values, row_splits, combiner,
                                          lr, empty, False, 0.0, out_dtype,
                                          per_id_w)


def csr_lookup_fused_optimizer(weight, values, row_splits, combiner, lr, state,
                               adagrad, eps, out_dtype=None, per_id_w=None,
                               sr=None, adam=None):
    return _CsrLookupFusedOptimizer.apply(weight, values, row_splits, combiner,
                                          lr, state, adagrad, eps, out_dtype,
                                          per_id_w, sr, adam)


def check_per_id_weights(per_id_w, nnz: int) -> None:
    """Raises ValueError unless per_id_w is a floating tensor of nnz weights."""
    if not isinstance(per_id_w, torch.Tensor) or not per_id_w.is_floating_point():
        raise ValueError("per-sample weights must be a floating-point tensor")
    if per_id_w.numel() != nnz:
        raise ValueError(f"got {per_id_w.numel()} per-sample weights for "
                         f"{nnz} ids")


def _dense_fixed_hotness(weight, ids, combiner, per_sample_weights=None):
    """Dense [batch, hotness] ids + combiner -> gather + reduce.

    Parity: reference dispatcher's native path for fixed hotness
    (``embedding_lookup_ops.py:97-102``).
    """
    out = _CsrLookup.apply(
        weight,
        ids.reshape(-1),
        torch.arange(
            0, ids.numel() + 1, ids.shape[1], device=ids.device, dtype=torch.long
        ),
        combiner,
        None,
        None if per_sample_weights is None else per_sample_weights.reshape(-1),
    )
    return out


def embedding_lookup(
    weight: torch.Tensor,
    ids: Union[torch.Tensor, Ragged],
    combiner: Optional[str] = None,
    per_sample_weights: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """Looks up and optionally combines embedding rows.

    Routing parity with the reference dispatcher (``embedding_lookup_ops.py:
    37-102``):

    * ``combiner is None`` -> plain gather (dense int ids of any rank).
    * ``Ragged`` input + combiner -> CSR custom-kernel path; hotness-all-1
      collapses to plain gather.
    * ``torch.sparse_coo`` ids + combiner -> ``row_to_split`` then CSR path.
    * dense ``[batch, hotness]`` + combiner -> gather + reduce.

    Per-sample weights (one floating weight per id; beyond the reference)
    scale each row before the reduce: ``out[r] = c_r * sum_k w_k * T[i_k]``
    with ``c_r = 1`` for ``sum`` and ``1 / len(r)`` for ``mean``.  A
    ``Ragged`` carries them in ``.weights``; dense ``[batch, hotness]`` ids
    take a same-shape ``per_sample_weights``; sparse COO ids take a sparse
    COO tensor of the same shape or a 1-D tensor aligned with the coalesced
    values.  Weights need a combiner, and their gradient flows back in the
    weights' dtype.
    """
    if combiner not in (None, "sum", "mean"):
        raise ValueError(f"combiner must be None, 'sum' or 'mean', got {combiner!r}")

    if isinstance(ids, Ragged):
        if ids.weights is not None and per_sample_weights is not None:
            raise ValueError("give the weights either as Ragged.weights or "
                             "as per_sample_weights, not both")
        w = ids.weights if ids.weights is not None else per_sample_weights
        if combiner is None:
            raise ValueError("Ragged input requires a combiner ('sum' or 'mean')")
        if w is None:
            return _CsrLookup.apply(weight, ids.values, ids.row_splits, combiner)
        check_per_id_weights(w, ids.values.numel())
        return _CsrLookup.apply(weight, ids.values, ids.row_splits, combiner,
                                None, w.reshape(-1))

    if per_sample_weights is not None and combiner is None:
        raise ValueError("per_sample_weights require a combiner "
                         "('sum' or 'mean')")

    if ids.layout == torch.sparse_coo:
        if combiner is None:
            raise ValueError("Sparse input requires a combiner ('sum' or 'mean')")
        ids = ids.coalesce()
        splits = row_to_split(ids.indices().t().contiguous(), ids.shape[0])
        if per_sample_weights is None:
            return _CsrLookup.apply(weight, ids.values(), splits, combiner)
        w = per_sample_weights
        if w.layout == torch.sparse_coo:
            if w.shape != ids.shape:
                raise ValueError(f"sparse weights shape {tuple(w.shape)} does "
                                 f"not match ids shape {tuple(ids.shape)}")
            w = w.coalesce().values()
        elif w.dim() != 1:
            raise ValueError("weights for sparse ids must be sparse COO or "
                             "1-D, aligned with the coalesced values")
        check_per_id_weights(w, ids.values().numel())
        return _CsrLookup.apply(weight, ids.values(), splits, combiner, None, w)

    if combiner is None:
        return weight.index_select(0, ids.reshape(-1)).view(*ids.shape, weight.shape[1])

    if ids.dim() != 2:
        raise ValueError(f"Dense ids with combiner must be 2-D, got {ids.dim()}-D")
    if per_sample_weights is not None:
        if per_sample_weights.shape != ids.shape:
            raise ValueError(
                f"per_sample_weights shape {tuple(per_sample_weights.shape)} "
                f"does not match ids shape {tuple(ids.shape)}")
        check_per_id_weights(per_sample_weights, ids.numel())
    # hotness-1 included: the CSR path keeps the sparse-grad (IndexedSlices)
    # contract and the OOB->zero semantics on every combiner lookup.
    return _dense_fixed_hotness(weight, ids, combiner, per_sample_weights)


# ---------------------------------------------------------------------------
# int8 row-wise quantized tables (inference only)
# ---------------------------------------------------------------------------
#
# Storage: uint8 [vocab, width + 8], contiguous.  Row i holds width bytes
# q[i, c] in 0..255, then fp32 scale[i], then fp32 bias[i] (native byte
# order), and stands for scale[i] * q[i, c] + bias[i] — byte for byte the
# "fused 8-bit rowwise" layout of FBGEMM / torch.ops.quantized.
# embedding_bag_byte_prepack.  width % 4 == 0 keeps every dword, scale and
# bias 4-byte aligned.

#
# int4 row-wise quantized tables
#
# Storage: uint8 [vocab, width / 2 + 4], contiguous.  Row i holds width / 2
# bytes of nibbles q[i, c] in 0..15 (column 2j in the low nibble of byte j,
# column 2j + 1 in the high one), then fp16 scale[i], then fp16 bias[i], and
# stands for scale[i] * q[i, c] + bias[i] — byte for byte the "fused 4-bit
# rowwise" layout of FBGEMM / torch.ops.quantized.embedding_bag_4bit_prepack.
# That layout only needs an even width; this project requires width % 8 == 0,
# which makes a lane's dword eight whole columns and keeps the row stride and
# the scale/bias dword 4-byte aligned.
#
# A packed shape alone does not say which of the two formats it holds, so
# every consumer takes ``bits`` (8 or 4) explicitly.

_Q8_TAIL = 8
_Q4_TAIL = 4


def _check_bits(bits) -> int:
    if bits not in (4, 8):
        raise ValueError(f"bits must be 4 or 8, got {bits!r}")
    return int(bits)


def _check_packed(packed: torch.Tensor, bits: int = 8) -> int:
    """Validates an int8 (``bits=8``) or int4 (``bits=4``) row-wise packed
    table and returns its width."""
    _check_bits(bits)
    if not isinstance(packed, torch.Tensor) or packed.dtype != torch.uint8:
        raise ValueError("a quantized table must be a uint8 tensor")
    if bits == 4:
        if (packed.dim() != 2 or packed.shape[1] < _Q4_TAIL + 4
                or (packed.shape[1] - _Q4_TAIL) % 4 != 0):
            raise ValueError(
                f"an int4 quantized table must be [vocab, width / 2 + 4] "
                f"with width a positive multiple of 8, got "
                f"{tuple(packed.shape)}")
        return 2 * (packed.shape[1] - _Q4_TAIL)
    if (packed.dim() != 2 or packed.shape[1] < _Q8_TAIL + 4
            or (packed.shape[1] - _Q8_TAIL) % 4 != 0):
        raise ValueError(
            f"a quantized table must be [vocab, width + 8] with width a "
            f"positive multiple of 4, got {tuple(packed.shape)}")
    return packed.shape[1] - _Q8_TAIL


def _quantize_rows_ref(x: torch.Tensor) -> torch.Tensor:
    """Pure-torch quantizer of fp32 [n, width] rows (CPU path)."""
    n, width = x.shape
    out = torch.empty(n, width + _Q8_TAIL, dtype=torch.uint8, device=x.device)
    if n == 0:
        return out
    lo = x.min(dim=1, keepdim=True).values
    hi = x.max(dim=1, keepdim=True).values
    rng = hi - lo
    scale = rng / 255
    inv = torch.where(rng > 0, 255 / rng, torch.zeros_like(rng))
    q = torch.round((x - lo) * inv).clamp_(0, 255)
    out[:, :width] = q.to(torch.uint8)
    tail = torch.cat([scale, lo], dim=1).contiguous()
    out[:, width:] = tail.view(torch.uint8)
    return out


def quantize_rowwise_int8(weight: torch.Tensor,
                          chunk_rows: Optional[int] = None) -> torch.Tensor:
    """fp32 or bf16 ``[vocab, width]`` -> int8 row-wise packed
    ``[vocab, width + 8]`` uint8 on the same device.

    Per row: ``bias = min``, ``scale = (max - min) / 255`` and
    ``q = clamp(rint((x - bias) * (255 / (max - min))), 0, 255)``; a
    constant row stores ``q = 0`` and dequantizes exactly.  ``width`` must be
    a multiple of 4.  On the device the HIP kernel converts ``chunk_rows``
    rows per launch (all of them by default); the temporaries are bounded by
    the chunk.
    """
    if weight.dim() != 2:
        raise ValueError(f"weight must be 2-D, got {weight.dim()}-D")
    if weight.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("weight must be fp32 or bf16")
    width = weight.shape[1]
    if width < 4 or width % 4 != 0:
        raise ValueError(f"int8 row-wise quantization needs a width that is "
                         f"a multiple of 4, got width {width}")

    def convert(rows):
        rows = rows.contiguous()
        if rows.is_cuda:
            return _backend.ops().quantize_rows_q8(rows)
        return _quantize_rows_ref(rows.float())

    return _quantize_chunked(weight, chunk_rows, width + _Q8_TAIL, convert)


def _quantize_chunked(weight, chunk_rows, row_bytes, convert):
    """``convert`` over ``chunk_rows`` rows at a time (all by default) into
    one ``[vocab, row_bytes]`` uint8 table on ``weight``'s device."""
    if chunk_rows is not None and chunk_rows <= 0:
        raise ValueError("chunk_rows must be positive")
    weight = weight.detach()
    n = weight.shape[0]
    step = n if chunk_rows is None else int(chunk_rows)
    if step >= n:
        return convert(weight)
    out = torch.empty(n, row_bytes, dtype=torch.uint8, device=weight.device)
    for s in range(0, n, step):
        out[s:s + step].copy_(convert(weight[s:s + step]))
    return out


def _quantize_rows_q4_ref(x: torch.Tensor) -> torch.Tensor:
    """Pure-torch int4 quantizer of fp32 [n, width] rows (CPU path): the
    contract of :func:`quantize_rowwise_int4`, step by step."""
    n, width = x.shape
    out = torch.empty(n, width // 2 + _Q4_TAIL, dtype=torch.uint8,
                      device=x.device)
    if n == 0:
        return out
    bias_h = x.min(dim=1, keepdim=True).values.to(torch.float16)
    bias = bias_h.float()
    rng = x.max(dim=1, keepdim=True).values - bias
    one = torch.ones_like(rng)
    scale_h = torch.where(rng == 0, one, rng / 15).to(torch.float16)
    scale = scale_h.float()
    unusable = (scale == 0) | torch.isinf(1 / scale)
    scale_h = torch.where(unusable, one.to(torch.float16), scale_h)
    inv = 1 / scale_h.float()
    q = torch.round((x - bias) * inv).clamp_(0, 15).to(torch.uint8)
    out[:, :width // 2] = q[:, 0::2] | (q[:, 1::2] << 4)
    tail = torch.cat([scale_h, bias_h], dim=1).contiguous()
    out[:, width // 2:] = tail.view(torch.uint8)
    return out


def quantize_rowwise_int4(weight: torch.Tensor,
                          chunk_rows: Optional[int] = None) -> torch.Tensor:
    """fp32 or bf16 ``[vocab, width]`` -> int4 row-wise packed
    ``[vocab, width / 2 + 4]`` uint8 on the same device: the bytes of
    ``torch.ops.quantized.embedding_bag_4bit_prepack`` (of ``weight.float()``
    for a bf16 table).

    Per row, in fp32: ``b = fp16(min)`` (nearest-even, widened again),
    ``range = max - b``, ``s = fp16(1 if range == 0 else range / 15)``
    widened again, ``s = 1`` if ``s == 0`` or ``1 / s`` is infinite, and
    ``q = clamp(rint((x - b) * (1 / s)), 0, 15)``.  A constant row whose
    value is fp16-representable stores all-zero nibbles, scale 1 and that
    value.  Any other constant ``x`` leaves ``range = x - fp16(x) != 0`` and
    takes the general path, as in torch: nibbles of 15 and a tiny scale,
    which is negative when ``fp16(x) > x``.  Rows holding ``|x| > 65504`` or NaN are
    outside the contract, as they are in torch (fp16 overflows); they are
    not checked for, which would cost a host sync.

    ``width`` must be a multiple of 8 (torch's layout itself only needs an
    even width).  ``chunk_rows`` as in :func:`quantize_rowwise_int8`.
    """
    if weight.dim() != 2:
        raise ValueError(f"weight must be 2-D, got {weight.dim()}-D")
    if weight.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("weight must be fp32 or bf16")
    width = weight.shape[1]
    if width < 8 or width % 8 != 0:
        raise ValueError(
            f"int4 row-wise quantization needs a width that is a multiple "
            f"of 8 (the 4-bit layout itself only needs an even width), got "
            f"width {width}")

    def convert(rows):
        rows = rows.contiguous()
        if rows.is_cuda:
            return _backend.ops().quantize_rows_q4(rows)
        return _quantize_rows_q4_ref(rows.float())

    return _quantize_chunked(weight, chunk_rows, width // 2 + _Q4_TAIL,
                             convert)


def dequantize_rowwise_int4(packed: torch.Tensor) -> torch.Tensor:
    """int4 row-wise packed ``[vocab, width / 2 + 4]`` -> fp32
    ``[vocab, width]``: ``fma(scale, q, bias)`` with scale and bias widened
    from fp16, one fp32 rounding per element (the CPU path evaluates in fp64,
    where product and sum are exact, and rounds once)."""
    width = _check_packed(packed, 4)
    packed = packed.contiguous()
    if packed.is_cuda:
        return _backend.ops().dequantize_rows_q4(packed)
    nib = packed[:, :width // 2]
    q = torch.stack([nib & 0xF, nib >> 4], dim=2).reshape(-1, width).double()
    tail = packed[:, width // 2:].contiguous().view(torch.float16).double()
    return (q * tail[:, 0:1] + tail[:, 1:2]).float()


def dequantize_rowwise_int8(packed: torch.Tensor) -> torch.Tensor:
    """int8 row-wise packed ``[vocab, width + 8]`` -> fp32 ``[vocab, width]``:
    ``fma(scale, q, bias)``, one fp32 rounding per element.

    The CPU path evaluates in fp64 and rounds once: ``scale * q`` is exact
    there (24 x 8 bits), and so is the sum unless the two terms are more than
    2**21 apart in magnitude, so the result is the fused multiply-add's."""
    width = _check_packed(packed)
    packed = packed.contiguous()
    if packed.is_cuda:
        return _backend.ops().dequantize_rows_q8(packed)
    tail = packed[:, width:].contiguous().view(torch.float32).double()
    return (packed[:, :width].double() * tail[:, 0:1] + tail[:, 1:2]).float()


def _csr_lookup_q8(packed, values, row_splits, combiner, out_dtype=None,
                   per_id_w=None, bits=8):
    """CSR lookup from a packed table (int8, or int4 with ``bits=4``): HIP
    kernel, or on the CPU ``_csr_lookup_ref`` over the gathered, dequantized
    rows."""
    w32 = _kernel_weights(per_id_w)
    if packed.is_cuda:
        ext = _backend.ops()
        forward = (ext.csr_lookup_forward_q4 if bits == 4
                   else ext.csr_lookup_forward_q8)
        return forward(packed, values, row_splits, combiner == "mean",
                       out_dtype == torch.bfloat16, w32,
                       deterministic=is_deterministic())
    vocab = packed.shape[0]
    valid = (values >= 0) & (values < vocab)
    # dequantize only the rows the batch touches, and append one zero row:
    # an out-of-range id becomes that row's id, so the gathered table is
    # never empty, even when no id of the call is valid
    pos = torch.cumsum(valid.to(torch.long), 0) - 1
    dequantize = (dequantize_rowwise_int4 if bits == 4
                  else dequantize_rowwise_int8)
    rows = dequantize(packed.index_select(0, values[valid]))
    n_valid = rows.shape[0]
    rows = torch.cat([rows, rows.new_zeros(1, rows.shape[1])])
    local = torch.where(valid, pos, torch.full_like(pos, n_valid))
    out = _csr_lookup_ref(rows, local, row_splits, combiner, w32)
    return out.to(out_dtype) if out_dtype is not None else out


def quantized_embedding_lookup(
    packed: torch.Tensor,
    ids: Union[torch.Tensor, Ragged],
    combiner: Optional[str] = None,
    per_sample_weights: Optional[torch.Tensor] = None,
    out_dtype: Optional[torch.dtype] = None,
    bits: int = 8,
) -> torch.Tensor:
    """:func:`embedding_lookup` from an int8 row-wise quantized table
    (:func:`quantize_rowwise_int8`) or, with ``bits=4``, an int4 one
    (:func:`quantize_rowwise_int4`), forward only.  ``bits`` is explicit
    because a packed shape alone does not say which format it holds; anything
    but 4 or 8 raises ``ValueError``.

    Same routing: dense ids of any rank without a combiner (a hotness-1
    ``sum``), dense ``[batch, hotness]``, ``Ragged`` (with or without
    ``.weights``) and sparse COO ids with one.  Rows are dequantized on the
    fly and accumulated in fp32; an id outside ``[0, vocab)`` contributes a
    zero row.  The result is fp32, or ``out_dtype=torch.bfloat16``, and never
    requires grad.
    """
    if combiner not in (None, "sum", "mean"):
        raise ValueError(f"combiner must be None, 'sum' or 'mean', got {combiner!r}")
    if out_dtype not in (None, torch.float32, torch.bfloat16):
        raise ValueError("out_dtype must be None, float32 or bfloat16")
    width = _check_packed(packed, bits)

    def run(values, splits, comb, w=None):
        if w is not None:
            check_per_id_weights(w, values.numel())
            w = w.reshape(-1)
        with torch.no_grad():
            return _csr_lookup_q8(packed, values.long().contiguous(),
                                  splits.long().contiguous(), comb, out_dtype,
                                  w, bits)

    if isinstance(ids, Ragged):
        if ids.weights is not None and per_sample_weights is not None:
            raise ValueError("give the weights either as Ragged.weights or "
                             "as per_sample_weights, not both")
        if combiner is None:
            raise ValueError("Ragged input requires a combiner ('sum' or 'mean')")
        w = ids.weights if ids.weights is not None else per_sample_weights
        return run(ids.values, ids.row_splits, combiner, w)

    if per_sample_weights is not None and combiner is None:
        raise ValueError("per_sample_weights require a combiner "
                         "('sum' or 'mean')")

    if ids.layout == torch.sparse_coo:
        if combiner is None:
            raise ValueError("Sparse input requires a combiner ('sum' or 'mean')")
        ids = ids.coalesce()
        splits = row_to_split(ids.indices().t().contiguous(), ids.shape[0])
        w = per_sample_weights
        if w is not None:
            if w.layout == torch.sparse_coo:
                if w.shape != ids.shape:
                    raise ValueError(f"sparse weights shape {tuple(w.shape)} does "
                                     f"not match ids shape {tuple(ids.shape)}")
                w = w.coalesce().values()
            elif w.dim() != 1:
                raise ValueError("weights for sparse ids must be sparse COO or "
                                 "1-D, aligned with the coalesced values")
        return run(ids.values(), splits, combiner, w)

    if combiner is None:
        flat = ids.reshape(-1)
        splits = torch.arange(flat.numel() + 1, device=flat.device,
                              dtype=torch.long)
        return run(flat, splits, "sum").view(*ids.shape, width)

    if ids.dim() != 2:
        raise ValueError(f"Dense ids with combiner must be 2-D, got {ids.dim()}-D")
    if per_sample_weights is not None and per_sample_weights.shape != ids.shape:
        raise ValueError(
            f"per_sample_weights shape {tuple(per_sample_weights.shape)} "
            f"does not match ids shape {tuple(ids.shape)}")
    b, h = ids.shape
    splits = torch.arange(b + 1, device=ids.device, dtype=torch.long) * h
    return run(ids.reshape(-1), splits, combiner, per_sample_weights)
