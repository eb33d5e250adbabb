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

from typing import NamedTuple, Optional, Sequence, Tuple, Union

import torch

from . import _backend


class Ragged(NamedTuple):
    """A batch of variable-hotness (ragged) id lists in CSR form.

    ``values``: 1-D int tensor of ids, ``row_splits``: int tensor of shape
    ``[num_rows + 1]``; row ``i`` owns ``values[row_splits[i]:row_splits[i+1]]``.

    Equivalent of ``tf.RaggedTensor`` in the reference API (rank-2 only, which
    is all the reference supports — ``embedding.py:129-131``).
    """

    values: torch.Tensor
    row_splits: torch.Tensor

    @property
    def nrows(self) -> int:
        return self.row_splits.numel() - 1

    @staticmethod
    def from_row_lengths(values: torch.Tensor, row_lengths: torch.Tensor) -> "Ragged":
        zero = torch.zeros(1, dtype=torch.long, device=row_lengths.device)
        splits = torch.cat([zero, row_lengths.cumsum(0)])
        return Ragged(values, splits)

    def row_lengths(self) -> torch.Tensor:
        return self.row_splits[1:] - self.row_splits[:-1]

    @staticmethod
    def from_lists(lists: Sequence[Sequence[int]], device=None) -> "Ragged":
        flat = [i for row in lists for i in row]
        lengths = torch.tensor([len(row) for row in lists], dtype=torch.long, device=device)
        values = torch.tensor(flat, dtype=torch.long, device=device)
        return Ragged.from_row_lengths(values, lengths)

    def to(self, *args, **kwargs) -> "Ragged":
        return Ragged(self.values.to(*args, **kwargs), self.row_splits.to(*args, **kwargs))


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
) -> torch.Tensor:
    """Pure-PyTorch CSR segmented gather-reduce (fp32 oracle + CPU path).

    Accumulates in fp32 and returns fp32 regardless of the table storage
    dtype (fp32 or bf16) — matching the HIP kernels.
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
    """

    @staticmethod
    def forward(ctx, weight, values, row_splits, combiner, out_dtype=None):
        ctx.save_for_backward(values, row_splits)
        ctx.combiner = combiner
        ctx.vocab = weight.shape[0]
        ctx.width = weight.shape[1]
        ctx.wdtype = weight.dtype
        if weight.is_cuda:
            # bf16 out is stored directly by the kernel (no cast kernel);
            # the backward consumes bf16 grads natively too
            return _backend.ops().csr_lookup_forward(
                weight, values, row_splits, combiner == "mean",
                out_dtype == torch.bfloat16)
        out = _csr_lookup_ref(weight, values, row_splits, combiner)
        return out.to(out_dtype) if out_dtype is not None else out

    @staticmethod
    def backward(ctx, grad_out):
        values, row_splits = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        if grad_out.is_cuda:
            unique_ids, unique_grad = _backend.ops().csr_lookup_backward(
                grad_out, values, row_splits, ctx.vocab, ctx.combiner == "mean"
            )
        else:
            unique_ids, unique_grad = _csr_lookup_backward_ref(
                grad_out, values, row_splits, ctx.vocab, ctx.combiner
            )
        grad_weight = torch.sparse_coo_tensor(
            unique_ids.unsqueeze(0),
            unique_grad.to(ctx.wdtype),  # autograd: grad dtype == param dtype
            size=(ctx.vocab, ctx.width),
            is_coalesced=True,
        )
        return grad_weight, None, None, None, None


def _csr_lookup_backward_ref(grad_out, values, row_splits, vocab, combiner):
    """CPU reference backward: unique ids + per-unique summed grad rows."""
    num_rows = row_splits.numel() - 1
    lengths = (row_splits[1:] - row_splits[:-1]).to(torch.long)
    seg_ids = torch.repeat_interleave(torch.arange(num_rows, device=values.device), lengths)
    g = grad_out.index_select(0, seg_ids)  # [nnz, width]
    if combiner == "mean":
        w = 1.0 / lengths.clamp(min=1).to(grad_out.dtype)
        g = g * w.index_select(0, seg_ids).unsqueeze(1)
    valid = (values >= 0) & (values < vocab)
    vals = values[valid]
    g = g[valid]
    unique_ids, inverse = torch.unique(vals, sorted=True, return_inverse=True)
    unique_grad = torch.zeros(unique_ids.numel(), grad_out.shape[1],
                              dtype=torch.float32, device=grad_out.device)
    unique_grad.index_add_(0, inverse, g.float())
    return unique_ids, unique_grad


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
    """

    @staticmethod
    def forward(ctx, weight, values, row_splits, combiner, lr, state, adagrad,
                eps, out_dtype=None):
        ctx.save_for_backward(weight, values, row_splits, lr, state)
        ctx.combiner = combiner
        ctx.adagrad = adagrad
        ctx.eps = eps
        if weight.is_cuda:
            return _backend.ops().csr_lookup_forward(
                weight, values, row_splits, combiner == "mean",
                out_dtype == torch.bfloat16)
        out = _csr_lookup_ref(weight, values, row_splits, combiner)
        return out.to(out_dtype) if out_dtype is not None else out

    @staticmethod
    def backward(ctx, grad_out):
        weight, values, row_splits, lr, state = ctx.saved_tensors
        grad_out = grad_out.contiguous()
        with torch.no_grad():
            if weight.is_cuda:
                _backend.ops().csr_fused_optimizer_apply(
                    weight, state, values, row_splits, grad_out, lr,
                    ctx.combiner == "mean", ctx.adagrad, ctx.eps)
            else:
                unique_ids, unique_grad = _csr_lookup_backward_ref(
                    grad_out.float(), values, row_splits, weight.shape[0],
                    ctx.combiner)
                lr_v = lr.item()
                if ctx.adagrad:
                    sq = unique_grad * unique_grad
                    rowwise = state.dim() == 1
                    state.index_add_(0, unique_ids,
                                     sq.mean(dim=1) if rowwise else sq)
                    denom = state.index_select(0, unique_ids).sqrt_().add_(ctx.eps)
                    if rowwise:
                        denom = denom.unsqueeze(1)
                    weight.index_add_(
                        0, unique_ids,
                        (-lr_v * unique_grad / denom).to(weight.dtype))
                else:
                    weight.index_add_(0, unique_ids,
                                      (unique_grad * (-lr_v)).to(weight.dtype))
        return (None,) * 9


def csr_lookup_fused_sgd(weight, values, row_splits, combiner, lr,
                         out_dtype=None):
    empty = torch.empty(0, dtype=torch.float32, device=weight.device)
    return _CsrLookupFusedOptimizer.apply(weight, values, row_splits, combiner,
                                          lr, empty, False, 0.0, out_dtype)


def csr_lookup_fused_optimizer(weight, values, row_splits, combiner, lr, state,
                               adagrad, eps, out_dtype=None):
    return _CsrLookupFusedOptimizer.apply(weight, values, row_splits, combiner,
                                          lr, state, adagrad, eps, out_dtype)


def _dense_fixed_hotness(weight, ids, combiner):
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
    )
    return out


def embedding_lookup(
    weight: torch.Tensor,
    ids: Union[torch.Tensor, Ragged],
    combiner: Optional[str] = None,
) -> torch.Tensor:
    """Looks up and optionally combines embedding rows.

    Routing parity with the reference dispatcher (``embedding_lookup_ops.py:
    37-102``):

    * ``combiner is None`` -> plain gather (dense int ids of any rank).
    * ``Ragged`` input + combiner -> CSR custom-kernel path; hotness-all-1
      collapses to plain gather.
    * ``torch.sparse_coo`` ids + combiner -> ``row_to_split`` then CSR path.
    * dense ``[batch, hotness]`` + combiner -> gather + reduce.
    """
    if combiner not in (None, "sum", "mean"):
        raise ValueError(f"combiner must be None, 'sum' or 'mean', got {combiner!r}")

    if isinstance(ids, Ragged):
        if combiner is None:
            raise ValueError("Ragged input requires a combiner ('sum' or 'mean')")
        return _CsrLookup.apply(weight, ids.values, ids.row_splits, combiner)

    if ids.layout == torch.sparse_coo:
        if combiner is None:
            raise ValueError("Sparse input requires a combiner ('sum' or 'mean')")
        ids = ids.coalesce()
        splits = row_to_split(ids.indices().t().contiguous(), ids.shape[0])
        return _CsrLookup.apply(weight, ids.values(), splits, combiner)

    if combiner is None:
        return weight.index_select(0, ids.reshape(-1)).view(*ids.shape, weight.shape[1])

    if ids.dim() != 2:
        raise ValueError(f"Dense ids with combiner must be 2-D, got {ids.dim()}-D")
    # hotness-1 included: the CSR path keeps the sparse-grad (IndexedSlices)
    # contract and the OOB->zero semantics on every combiner lookup.
    return _dense_fixed_hotness(weight, ids, combiner)
