"""Linear/ReLU stacks with the ReLU backward and the bias gradient fused.

Under bf16 autocast a plain ``nn.Sequential`` of ``Linear``/``ReLU`` makes,
next to its GEMMs, two full passes over every ``[B, N]`` gradient in
backward: ``threshold_backward``, then the bias-gradient column sum that
re-reads what the first wrote.  ``MLP`` keeps the module tree, the parameter
names and every GEMM call of that path and replaces the two passes by one
(``relu_bwd_bias_grad``, ``csrc/mlp_ops.hip``).

The weight gradient ``g.t().mm(x)``, summed over the batch, goes to the
split-K kernels of ``csrc/wgrad_splitk.hip`` at the shapes their plan routes
(``weight_grad``).

``DE_FUSED_MLP=0`` switches the fast path off (plain ``nn.Sequential``);
``DE_WGRAD_SPLITK=0`` keeps the weight gradients on the GEMM library.
"""

import os
from typing import Tuple

import torch
from torch import nn

from . import _backend


def relu_bwd_bias_grad(grad_out: torch.Tensor,
                       y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(threshold_backward(grad_out, y, 0), its column sum)``.

    One HIP pass for contiguous bf16 ``[B, N]`` GPU tensors with
    ``N % 8 == 0``; the plain torch ops for anything else.
    """
    if (grad_out.is_cuda and grad_out.dim() == 2
            and grad_out.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
            and grad_out.shape == y.shape and grad_out.shape[1] % 8 == 0
            and grad_out.is_contiguous() and y.is_contiguous()):
        g, gb = _backend.ops().relu_bwd_bias_grad(grad_out, y)
        return g, gb
    g = torch.ops.aten.threshold_backward(grad_out, y, 0)
    return g, g.sum(0)


def _wgrad_routed(k: int, m: int, n: int) -> bool:
    """Whether the plan (``wgrad_splitk_plan``) sends this shape to the kernel."""
    return bool(_backend.ops().wgrad_splitk_plan(k, m, n)[0])


def weight_grad(g: torch.Tensor, xb: torch.Tensor) -> torch.Tensor:
    """``g.t().mm(xb)``: the split-K HIP kernels (``csrc/wgrad_splitk.hip``)
    for the shapes their plan routes (contiguous, 16-byte aligned bf16 GPU
    operands, a large batch), the GEMM library for everything else.
    ``DE_WGRAD_SPLITK=0`` keeps every shape on the library.
    """
    if (g.is_cuda and g.dim() == 2 and xb.dim() == 2
            and g.dtype == torch.bfloat16 and xb.dtype == torch.bfloat16
            and g.is_contiguous() and xb.is_contiguous()
            and g.data_ptr() % 16 == 0 and xb.data_ptr() % 16 == 0
            and os.environ.get("DE_WGRAD_SPLITK", "1") != "0"
            and _wgrad_routed(g.shape[0], g.shape[1], xb.shape[1])):
        return _backend.ops().wgrad_splitk(g, xb)
    return g.t().mm(xb)


class _LinearReLU(torch.autograd.Function):
    """``relu(addmm(b, x, W^T))`` in bf16 for fp32 parameters.

    Issues exactly the casts and GEMM calls of autocast ``F.linear`` + ReLU
    and of their autograd backward (``addmm``; ``g.mm(W)``; ``g.t().mm(x)``),
    so the TunableOp selections in ``profiles/`` keep applying; only the
    masking and the bias gradient differ (one kernel instead of two) and, at
    the shapes ``weight_grad`` routes, the weight gradient.
    """

    @staticmethod
    def forward(ctx, x, w, b):
        xb = x.to(torch.bfloat16)
        wb = w.to(torch.bfloat16)
        y = torch.addmm(b.to(torch.bfloat16), xb, wb.t())
        torch.relu_(y)
        ctx.save_for_backward(xb, wb, y)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xb, wb, y = ctx.saved_tensors
        g, gb = relu_bwd_bias_grad(grad_out, y)
        gx = None
        if ctx.needs_input_grad[0]:
            gx = g.mm(wb).to(ctx.x_dtype)
        gw = weight_grad(g, xb)
        # bf16 gradients of the fp32 parameters: the engine converts them
        return gx, gw, gb


class MLP(nn.Sequential):
    """``nn.Sequential`` of ``Linear`` and ``ReLU`` with a fused GPU path.

    Same children, parameter names and ``state_dict`` as the plain
    ``nn.Sequential``.  For a 2-D GPU input under bf16 autocast, with the HIP
    extension built, every ``Linear`` (fp32, with bias) followed by a
    ``ReLU`` runs as one ``_LinearReLU``; every other module runs as it is.
    Everything else takes the unchanged ``nn.Sequential`` forward.
    """

    def _fused(self, x: torch.Tensor) -> bool:
        return (x.is_cuda and x.dim() == 2 and torch.is_autocast_enabled()
                and torch.get_autocast_dtype("cuda") == torch.bfloat16
                and os.environ.get("DE_FUSED_MLP", "1") != "0"
                and _backend.available())

    def forward(self, input):  # noqa: A002 (nn.Sequential's signature)
        if not self._fused(input):
            return super().forward(input)
        mods = list(self)
        h = input
        i = 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.Linear) and m.bias is not None
                    and m.weight.dtype == torch.float32
                    and m.bias.dtype == torch.float32
                    and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
                    and h.dim() == 2):
                h = _LinearReLU.apply(h, m.weight, m.bias)
                i += 2
            else:
                h = m(h)
                i += 1
        return h
