"""Linear/ReLU stacks with the ReLU backward and the bias gradient fused.

Under bf16 autocast a plain ``nn.Sequential`` of ``Linear``/``ReLU`` makes,
next to its GEMMs, two full passes over every ``[B, N]`` gradient in
backward: ``threshold_backward``, then the bias-gradient column sum that
re-reads what the first wrote.  ``MLP`` keeps the module tree, the parameter
names and every GEMM call of that path and replaces the two passes by one
(``relu_bwd_bias_grad``, ``csrc/mlp_ops.hip``).

The weight gradient ``g.t().mm(x)``, summed over the batch, goes to the
split-K kernels of ``csrc/wgrad_splitk.hip`` at the shapes their plan routes
(``weight_grad``).  A closing ``Linear`` with one output feature (the logit
layer) gets its weight and bias gradient from one streaming pass
(``final_layer_grads``).

An fp32 input without autocast takes the same three routes on fp32 kernels
(``relu_bwd_bias_grad_f32``, ``wgrad_splitk_f32``, ``wgrad_gemv_f32``); its
GEMM calls are those of the plain path, so the forward output and the input
gradient do not change by a bit.

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
    ``N % 8 == 0``, and for contiguous, 16-byte aligned fp32 ones with
    ``N % 4 == 0``; the plain torch ops for anything else.
    """
    if (grad_out.is_cuda and grad_out.dim() == 2
            and grad_out.dtype == torch.bfloat16 and y.dtype == torch.bfloat16
            and grad_out.shape == y.shape and grad_out.shape[1] % 8 == 0
            and grad_out.is_contiguous() and y.is_contiguous()):
        g, gb = _backend.ops().relu_bwd_bias_grad(grad_out, y)
        return g, gb
    if (grad_out.is_cuda and grad_out.dim() == 2
            and grad_out.dtype == torch.float32 and y.dtype == torch.float32
            and grad_out.shape == y.shape and grad_out.shape[1] % 4 == 0
            and grad_out.is_contiguous() and y.is_contiguous()
            and grad_out.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0):
        g, gb = _backend.ops().relu_bwd_bias_grad_f32(grad_out, y)
        return g, gb
    g = torch.ops.aten.threshold_backward(grad_out, y, 0)
    return g, g.sum(0)


def _wgrad_routed(k: int, m: int, n: int) -> bool:
    """Whether the plan (``wgrad_splitk_plan``) sends this shape to the kernel."""
    return bool(_backend.ops().wgrad_splitk_plan(k, m, n)[0])


def _wgrad_f32_routed(k: int, m: int, n: int) -> bool:
    """The same for fp32 operands (``wgrad_splitk_f32_plan``)."""
    return bool(_backend.ops().wgrad_splitk_f32_plan(k, m, n)[0])


def weight_grad(g: torch.Tensor, xb: torch.Tensor) -> torch.Tensor:
    """``g.t().mm(xb)``: the split-K HIP kernels (``csrc/wgrad_splitk.hip``,
    ``csrc/wgrad_splitk_f32.hip``) for the shapes their plan routes
    (contiguous, 16-byte aligned GPU operands, both bf16 or both fp32, a large
    batch), the GEMM library for everything else.
    ``DE_WGRAD_SPLITK=0`` keeps every shape on the library.
    """
    if (g.is_cuda and g.dim() == 2 and xb.dim() == 2
            and g.dtype == torch.bfloat16 and xb.dtype == torch.bfloat16
            and g.is_contiguous() and xb.is_contiguous()
            and g.data_ptr() % 16 == 0 and xb.data_ptr() % 16 == 0
            and os.environ.get("DE_WGRAD_SPLITK", "1") != "0"
            and _wgrad_routed(g.shape[0], g.shape[1], xb.shape[1])):
        return _backend.ops().wgrad_splitk(g, xb)
    if (g.is_cuda and g.dim() == 2 and xb.dim() == 2
            and g.dtype == torch.float32 and xb.dtype == torch.float32
            and g.is_contiguous() and xb.is_contiguous()
            and g.data_ptr() % 16 == 0 and xb.data_ptr() % 16 == 0
            and os.environ.get("DE_WGRAD_SPLITK", "1") != "0"
            and _wgrad_f32_routed(g.shape[0], g.shape[1], xb.shape[1])):
        return _backend.ops().wgrad_splitk_f32(g, xb)
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


def _wgrad_gemv_routed(k: int, n: int) -> bool:
    """Whether the plan (``wgrad_gemv_plan``) sends this shape to the kernel."""
    return bool(_backend.ops().wgrad_gemv_plan(k, n)[0])


def _wgrad_gemv_f32_routed(k: int, n: int) -> bool:
    """The same for fp32 operands (``wgrad_gemv_f32_plan``)."""
    return bool(_backend.ops().wgrad_gemv_f32_plan(k, n)[0])


def final_layer_grads(g: torch.Tensor,
                      xb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(g.t().mm(xb), g.sum(0))`` for ``g [K, 1]``: one streaming pass
    (``wgrad_gemv``, ``csrc/wgrad_splitk.hip``) under the guards of
    ``weight_grad``, the library for everything else.
    """
    if (g.is_cuda and g.dim() == 2 and xb.dim() == 2 and g.shape[1] == 1
            and g.dtype == torch.bfloat16 and xb.dtype == torch.bfloat16
            and g.is_contiguous() and xb.is_contiguous()
            and xb.data_ptr() % 16 == 0
            and os.environ.get("DE_WGRAD_SPLITK", "1") != "0"
            and _wgrad_gemv_routed(g.shape[0], xb.shape[1])):
        gw, gb = _backend.ops().wgrad_gemv(g, xb)
        return gw, gb
    if (g.is_cuda and g.dim() == 2 and xb.dim() == 2 and g.shape[1] == 1
            and g.dtype == torch.float32 and xb.dtype == torch.float32
            and g.is_contiguous() and xb.is_contiguous()
            and xb.data_ptr() % 16 == 0
            and os.environ.get("DE_WGRAD_SPLITK", "1") != "0"
            and _wgrad_gemv_f32_routed(g.shape[0], xb.shape[1])):
        gw, gb = _backend.ops().wgrad_gemv_f32(g, xb)
        return gw, gb
    return g.t().mm(xb), g.sum(0)


class _LinearReLUF32(torch.autograd.Function):
    """``relu(addmm(b, x, W^T))`` on fp32 tensors, autocast off.

    Issues exactly the calls of ``F.linear`` + ReLU and of their autograd
    backward (``addmm``, ``relu_``; ``g.mm(W)``), no casts and no copies, so
    the output and the input gradient are those of the plain path bit for
    bit; the masking and the bias gradient come from one kernel and the
    weight gradient from ``weight_grad``.
    """

    @staticmethod
    def forward(ctx, x, w, b):
        y = torch.addmm(b, x, w.t())
        torch.relu_(y)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, w, y = ctx.saved_tensors
        g, gb = relu_bwd_bias_grad(grad_out, y)
        gx = g.mm(w) if ctx.needs_input_grad[0] else None
        return gx, weight_grad(g, x), gb


class _LinearOut1F32(torch.autograd.Function):
    """``addmm(b, x, W^T)`` on fp32 tensors for a ``Linear`` with one output
    feature and no ReLU behind it; ``final_layer_grads`` in backward."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return torch.addmm(b, x, w.t())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        x, w = ctx.saved_tensors
        gx = grad_out.mm(w) if ctx.needs_input_grad[0] else None
        gw, gb = final_layer_grads(grad_out, x)
        return gx, gw, gb


class _LinearOut1(torch.autograd.Function):
    """``addmm(b, x, W^T)`` in bf16 for an fp32 ``Linear`` with one output
    feature and no ReLU behind it (the logit layer).

    Issues exactly the casts and GEMM calls of autocast ``F.linear`` and of
    its autograd backward, except that the weight gradient ``g.t().mm(x)``
    and the bias gradient ``g.sum(0)``, two passes with ``M = 1`` that the
    library runs on a handful of workgroups, come from ``final_layer_grads``.
    """

    @staticmethod
    def forward(ctx, x, w, b):
        xb = x.to(torch.bfloat16)
        wb = w.to(torch.bfloat16)
        y = torch.addmm(b.to(torch.bfloat16), xb, wb.t())
        ctx.save_for_backward(xb, wb)
        ctx.x_dtype = x.dtype
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        xb, wb = ctx.saved_tensors
        gx = None
        if ctx.needs_input_grad[0]:
            gx = grad_out.mm(wb).to(ctx.x_dtype)
        gw, gb = final_layer_grads(grad_out, xb)
        return gx, gw, gb


class MLP(nn.Sequential):
    """``nn.Sequential`` of ``Linear`` and ``ReLU`` with a fused GPU path.

    Same children, parameter names and ``state_dict`` as the plain
    ``nn.Sequential``.  For a 2-D GPU input under bf16 autocast, with the HIP
    extension built, every ``Linear`` (fp32, with bias) followed by a
    ``ReLU`` runs as one ``_LinearReLU``, such a ``Linear`` with one output
    feature and no ``ReLU`` as ``_LinearOut1``; every other module runs as it is.
    A 2-D fp32 GPU input with autocast off takes the same route through
    ``_LinearReLUF32`` / ``_LinearOut1F32``, whose GEMM calls are those of the
    plain path on the same fp32 tensors.
    Everything else takes the unchanged ``nn.Sequential`` forward.
    """

    def _fused(self, x: torch.Tensor):
        """The (``Linear`` + ``ReLU``, closing ``Linear``) functions of the
        lane ``x`` takes, or ``None`` for the plain path."""
        if not (x.is_cuda and x.dim() == 2
                and os.environ.get("DE_FUSED_MLP", "1") != "0"
                and _backend.available()):
            return None
        if torch.is_autocast_enabled():
            if torch.get_autocast_dtype("cuda") == torch.bfloat16:
                return _LinearReLU, _LinearOut1
            return None
        if x.dtype == torch.float32:
            return _LinearReLUF32, _LinearOut1F32
        return None

    def forward(self, input):  # noqa: A002 (nn.Sequential's signature)
        lane = self._fused(input)
        if lane is None:
            return super().forward(input)
        linear_relu, linear_out1 = lane
        mods = list(self)
        h = input
        i = 0
        while i < len(mods):
            m = mods[i]
            ours = (isinstance(m, nn.Linear) and m.bias is not None
                    and m.weight.dtype == torch.float32
                    and m.bias.dtype == torch.float32 and h.dim() == 2)
            if ours and i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU):
                h = linear_relu.apply(h, m.weight, m.bias)
                i += 2
            elif ours and m.out_features == 1:
                h = linear_out1.apply(h, m.weight, m.bias)
                i += 1
            else:
                h = m(h)
                i += 1
        return h
