"""DCN-v2 low-rank cross interaction with a fused backward (gfx950).

The cross network of DLRM-DCNv2 runs over the concatenated features
``x0 [B, N]``::

    x_{l+1} = x0 * (W_l (V_l x_l) + b_l) + x_l        l = 0 .. L-1

with ``V_l [r, N]`` and ``W_l [N, r]``; the top MLP reads ``x_L``.

Next to its GEMMs the backward of a layer needs, for the gradient ``G`` of
``x_{l+1}``: ``gu = G * x0``, the bias gradient ``colsum(gu)``, and
``G * u_l`` summed over the layers into ``x0``'s gradient.  ``cross_bwd``
does the three in one pass (``csrc/mlp_ops.hip``); ``LowRankCrossNet`` wraps
the whole stack in one autograd function, so the sum over the layers is the
kernel's accumulator and not ``L - 1`` extra adds by the autograd engine.

``concat_packed`` builds ``x0`` from the bottom MLP's output and the packed
embeddings (``csrc/cross_ops.hip``).

``DE_FUSED_CROSS=0`` switches the kernels off: the plain composition under
autograd, and ``index_select`` + ``cat``.
"""

import os
from typing import Tuple

import torch
from torch import nn
from torch.nn import functional as F

from . import _backend
from .mlp import weight_grad


def _enabled() -> bool:
    return os.environ.get("DE_FUSED_CROSS", "1") != "0" and _backend.available()


def _bf16_2d_ok(*ts: torch.Tensor) -> bool:
    first = ts[0]
    return all(t.is_cuda and t.dim() == 2 and t.dtype == torch.bfloat16
               and t.shape == first.shape and t.is_contiguous()
               and t.data_ptr() % 16 == 0 for t in ts)


def cross_bwd(G: torch.Tensor, x0: torch.Tensor, u: torch.Tensor,
              acc: torch.Tensor, init: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(gu, gb)`` with ``gu = G * x0``, ``gb = gu.sum(0)``; in place,
    ``acc = G * u`` when ``init`` and ``acc += G * u`` otherwise.

    One HIP pass for contiguous, 16-byte aligned bf16 ``[B, N]`` GPU tensors
    with ``N % 8 == 0``: ``gu`` equals torch's product bit for bit, ``acc`` is
    formed in fp32 and rounded once, and with ``init`` the old ``acc`` is not
    read.  The plain torch ops, at any dtype, for anything else.
    """
    if (_bf16_2d_ok(G, x0, u, acc) and G.shape[1] % 8 == 0 and _enabled()):
        gu, gb = _backend.ops().cross_bwd(G, x0, u, acc, bool(init))
        return gu, gb
    gu = G * x0
    if init:
        acc.copy_(G * u)
    else:
        acc.add_(G * u)
    return gu, gu.sum(0)


class _ConcatPacked(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bottom, packed, perm, sample_major):
        ctx.save_for_backward(perm)
        ctx.sample_major = sample_major
        return _backend.ops().cross_concat_fwd(bottom, packed, perm,
                                               sample_major)

    @staticmethod
    def backward(ctx, gx0):
        (perm,) = ctx.saved_tensors
        gbottom, gpacked = _backend.ops().cross_concat_bwd(
            gx0.contiguous(), perm, ctx.sample_major)
        return gbottom, gpacked, None, None


def concat_packed(packed: torch.Tensor, bottom: torch.Tensor,
                  perm: torch.Tensor, sample_major: bool = False) -> torch.Tensor:
    """``x0 [B, (P+1)*D] = [bottom | embeddings in model order]``.

    ``packed`` and ``perm`` are those of
    ``ops.dot_interact.dot_interact_packed``: ``[P, B, D]`` feature-major or
    ``[B, P, D]`` sample-major, and ``x0[b, f*D:(f+1)*D]`` is packed row
    ``perm[f-1]`` of sample ``b``.  ``perm`` has to be a permutation.
    """
    d = packed.shape[2]
    if (packed.is_cuda and packed.dtype == torch.bfloat16
            and bottom.dtype == torch.bfloat16 and d % 8 == 0 and _enabled()):
        bottom, packed = bottom.contiguous(), packed.contiguous()
        if bottom.data_ptr() % 16 == 0 and packed.data_ptr() % 16 == 0:
            return _ConcatPacked.apply(bottom, packed, perm, sample_major)
    sel = packed.index_select(1, perm.long()) if sample_major else \
        packed.index_select(0, perm.long()).transpose(0, 1)
    return torch.cat([bottom, sel.reshape(bottom.shape[0], -1)], dim=1)


class _CrossStack(torch.autograd.Function):
    """The whole cross stack, forward and hand-derived backward.

    ``apply(x0, dtype, V_0, W_0, b_0, ..., V_{L-1}, W_{L-1}, b_{L-1})`` with
    ``dtype`` the compute dtype: bf16 under autocast, and float64 on the CPU
    in the tests, where every step is a torch op.
    """

    @staticmethod
    def forward(ctx, x0, dtype, *params):
        num_layers = len(params) // 3
        xc = x0.to(dtype).contiguous()
        saved = [xc]
        x = xc
        for l in range(num_layers):
            vb = params[3 * l].to(dtype)
            wb = params[3 * l + 1].to(dtype)
            v = x.mm(vb.t())
            u = torch.addmm(params[3 * l + 2].to(dtype), v, wb.t())
            saved += [x, v, u, vb, wb]
            x = torch.addcmul(x, xc, u)
        ctx.save_for_backward(*saved)
        ctx.num_layers = num_layers
        ctx.x_dtype = x0.dtype
        return x

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        saved = ctx.saved_tensors
        xc = saved[0]
        num_layers = ctx.num_layers
        G = grad_out.to(xc.dtype).contiguous()
        acc = torch.empty_like(xc)
        grads = [None] * (3 * num_layers)
        for l in range(num_layers - 1, -1, -1):
            x, v, u, vb, wb = saved[1 + 5 * l:6 + 5 * l]
            gu, gb = cross_bwd(G, xc, u, acc, l == num_layers - 1)
            grads[3 * l + 2] = gb
            grads[3 * l + 1] = weight_grad(gu, v)
            gv = gu.mm(wb)
            grads[3 * l] = weight_grad(gv, x)
            # residual + low-rank path in one GEMM epilogue
            G = torch.addmm(G, gv, vb)
        gx0 = None
        if ctx.needs_input_grad[0]:
            gx0 = (acc + G).to(ctx.x_dtype)
        # compute-dtype gradients of the parameters: the engine converts them
        return (gx0, None, *grads)


class LowRankCrossNet(nn.Module):
    """DCN-v2 low-rank cross network over ``x0 [B, in_features]``.

    Layer ``l`` holds ``v[l] = nn.Linear(N, r, bias=False)`` and
    ``w[l] = nn.Linear(r, N)`` (Xavier-normal weights, zero biases);
    ``forward(x0)`` returns ``x_L``.  For a 2-D bf16 GPU input under bf16
    autocast, with fp32 parameters, ``N % 8 == 0`` and the HIP extension
    built, the stack runs as one autograd function whose backward uses
    ``cross_bwd``; everything else is the plain composition under autograd.
    """

    def __init__(self, in_features: int, num_layers: int = 3,
                 low_rank: int = 512):
        super().__init__()
        if in_features < 1 or num_layers < 1 or low_rank < 1:
            raise ValueError("in_features, num_layers and low_rank must be "
                             "positive")
        self.in_features = in_features
        self.num_layers = num_layers
        self.low_rank = low_rank
        self.v = nn.ModuleList(nn.Linear(in_features, low_rank, bias=False)
                               for _ in range(num_layers))
        self.w = nn.ModuleList(nn.Linear(low_rank, in_features)
                               for _ in range(num_layers))
        for lin in list(self.v) + list(self.w):
            nn.init.xavier_normal_(lin.weight)
        for lin in self.w:
            nn.init.zeros_(lin.bias)

    def _params(self):
        out = []
        for v, w in zip(self.v, self.w):
            out += [v.weight, w.weight, w.bias]
        return out

    def _fused(self, x0: torch.Tensor) -> bool:
        return (x0.is_cuda and x0.dim() == 2
                and x0.dtype == torch.bfloat16
                and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16
                and self.in_features % 8 == 0
                and all(p.dtype == torch.float32 for p in self._params())
                and _enabled())

    def forward(self, x0: torch.Tensor) -> torch.Tensor:
        if self._fused(x0):
            return _CrossStack.apply(x0, torch.bfloat16, *self._params())
        x = x0
        for v, w in zip(self.v, self.w):
            u = F.linear(F.linear(x, v.weight), w.weight, w.bias)
            x = torch.addcmul(x, x0, u)
        return x
