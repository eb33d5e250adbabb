"""Fused concat + average pool: the synthetic models' interaction (gfx950).

``concat_avg_pool(inputs, numerical, stride)`` is::

    x = torch.cat(inputs, dim=1)
    x = avg_pool1d(x, stride, stride, ceil_mode=True)     # per row
    out = torch.cat([x, numerical], dim=1)

in one pass over the inputs (``csrc/concat_pool.hip``): the concatenated row
and the pooled row's fp32 promotion are never written.  The backward is one
hand-written pass too, and the inputs' gradients are views of one allocation.

``DE_FUSED_POOL=0`` switches the kernels off: the composition above under
autograd.
"""

import os
from typing import Optional, Sequence

import torch
from torch.nn import functional as F

from . import _backend

_DTYPES = (torch.bfloat16, torch.float32)
# the kernels keep stride * (output columns of a block) in one LDS row
MAX_STRIDE = 256


def _enabled() -> bool:
    return os.environ.get("DE_FUSED_POOL", "1") != "0" and _backend.available()


def fused_ok(inputs: Sequence[torch.Tensor], numerical: Optional[torch.Tensor],
             stride: int, out_dtype: Optional[torch.dtype] = None) -> bool:
    """Whether :func:`concat_avg_pool` takes the HIP kernels for these
    arguments (see there)."""
    if len(inputs) == 0 or not 1 <= stride <= MAX_STRIDE:
        return False
    first = inputs[0]
    if not first.is_cuda or first.dim() != 2 or first.dtype not in _DTYPES:
        return False
    if out_dtype is not None and out_dtype not in _DTYPES:
        return False
    chunk = 8 if first.dtype == torch.bfloat16 else 4
    b, dtype, device = first.shape[0], first.dtype, first.device
    for t in inputs:
        if not (t.dim() == 2 and t.shape[0] == b and t.dtype == dtype
                and t.device == device and t.shape[1] >= chunk
                and t.shape[1] % chunk == 0 and t.is_contiguous()
                and t.data_ptr() % 16 == 0):
            return False
    if numerical is not None and not (
            numerical.dim() == 2 and numerical.shape[0] == b
            and numerical.device == device and numerical.dtype in _DTYPES
            and numerical.is_contiguous()):
        return False
    return _enabled()


class _ConcatAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, numerical, stride, out_dtype, *inputs):
        ctx.stride = stride
        ctx.widths = [t.shape[1] for t in inputs]
        ctx.in_bf16 = inputs[0].dtype == torch.bfloat16
        ctx.num = None if numerical is None else \
            (numerical.shape[1], numerical.dtype)
        return _backend.ops().concat_pool_fwd(
            [t.detach() for t in inputs],
            None if numerical is None else numerical.detach(), stride,
            out_dtype == torch.bfloat16)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        nn_cols = 0 if ctx.num is None else ctx.num[0]
        if gout.dtype not in _DTYPES:
            gout = gout.float()
        gout = gout.contiguous()
        gins = [None] * len(ctx.widths)
        if any(ctx.needs_input_grad[3:]):
            gins = _backend.ops().concat_pool_bwd(
                gout, ctx.widths, ctx.stride, nn_cols, ctx.in_bf16)
        gnum = None
        if ctx.num is not None and ctx.needs_input_grad[0]:
            gnum = gout[:, gout.shape[1] - nn_cols:].to(ctx.num[1])
        return (gnum, None, None, *gins)


def concat_avg_pool(inputs: Sequence[torch.Tensor],
                    numerical: Optional[torch.Tensor], stride: int,
                    out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """``[avg_pool(cat(inputs)) | numerical]`` as ``[B, ceil(W / stride) + Nn]``.

    ``inputs[t]`` is ``[B, w_t]`` and ``W`` their total width.  Output column
    ``o < ceil(W / stride)`` is the mean of concatenated columns
    ``[o * stride, min((o + 1) * stride, W))``: the last, partial window is
    divided by its real length, as ``AvgPool1d(stride, stride,
    ceil_mode=True)`` does.  ``numerical`` ``[B, Nn]`` (or ``None``) follows,
    converted to ``out_dtype``, which defaults to the inputs' dtype.

    One HIP pass forward and one backward when all inputs are contiguous,
    16-byte aligned 2-D bf16 or fp32 tensors of one dtype and batch on one
    GPU with ``w_t % 8 == 0`` (bf16) or ``w_t % 4 == 0`` (fp32), ``numerical``
    is a contiguous bf16 or fp32 ``[B, Nn]`` tensor there, ``out_dtype`` is
    bf16 or fp32 and ``1 <= stride <= 256``.  A window is summed in fp32 in
    ascending column order, divided once and rounded once, with no atomics:
    two calls agree bit for bit, and ``stride == 1`` equals ``torch.cat``.
    The inputs' gradients are contiguous views of one flat allocation.
    Everything else, CPU tensors included, is the torch composition, with the
    pooled columns and ``numerical`` converted to the same ``out_dtype``.
    """
    inputs = list(inputs)
    if fused_ok(inputs, numerical, stride, out_dtype):
        return _ConcatAvgPool.apply(numerical, int(stride),
                                    out_dtype or inputs[0].dtype, *inputs)
    x = torch.cat(inputs, dim=1)
    x = F.avg_pool1d(x.unsqueeze(1), stride, stride=stride,
                     ceil_mode=True).squeeze(1)
    # the kernels' result dtype, not what cat would promote to
    out_dtype = out_dtype or inputs[0].dtype
    x = x.to(out_dtype)
    if numerical is None:
        return x
    return torch.cat([x, numerical.to(out_dtype)], dim=1)
