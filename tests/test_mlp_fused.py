"""Fused MLP elementwise ops (csrc/mlp_ops.hip, ops/mlp.py).

GPU tests compare the HIP kernels with the torch ops they replace:
``threshold_backward`` bit for bit, the bias gradient against the fp64 column
sum S of the masked gradient within

    |bias_grad - S| <= 2^-8 |S| + B 2^-24 sum_b |grad_in[b, n]|

(one bf16 rounding, half-ulp 2^-9, with a factor 2 margin, plus the worst case
of an fp32 accumulation of B terms in any order).  CPU tests cover the
unchanged ``nn.Sequential`` path and the ``state_dict`` layout.
"""

import math

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.ops import mlp as mlp_ops
from distributed_embeddings_amd.ops.mlp import MLP, relu_bwd_bias_grad

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")


def _assert_bias_grad_within_bound(bias_grad, grad_in):
    """bias_grad [N] against the fp64 column sum of the masked grad_in [B, N]."""
    gi = grad_in.double()
    s = gi.sum(0)
    a = gi.abs().sum(0)
    bound = 2.0 ** -8 * s.abs() + grad_in.shape[0] * 2.0 ** -24 * a
    got = bias_grad.double()
    nan_cols = s.isnan()
    assert torch.equal(got.isnan(), nan_cols)
    err = (got - s).abs()[~nan_cols]
    ok = err <= bound[~nan_cols]
    worst = (err / bound[~nan_cols].clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print(f"bias_grad: worst error / bound = {worst:.3f} over {err.numel()} columns")
    assert bool(ok.all()), f"worst error / bound = {worst}"


def _relu_inputs(b, n, device):
    g = torch.Generator().manual_seed(1000 * b + n)
    grad_out = torch.randn(b, n, generator=g).bfloat16()
    y = torch.randn(b, n, generator=g).bfloat16()
    flat = y.view(-1)
    special = [0.0, -0.0, float("nan")]
    for i, v in enumerate(special):          # first entries
        flat[i] = v
    for i, v in enumerate(special):          # and the last ones
        flat[flat.numel() - 1 - i] = v
    return grad_out.to(device), y.to(device)


RELU_SHAPES = [(1, 8), (3, 8), (257, 136), (4099, 128), (5000, 1024)]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("b,n", RELU_SHAPES)
def test_relu_bwd_bias_grad_vs_torch(b, n):
    grad_out, y = _relu_inputs(b, n, "cuda")
    g_before, y_before = grad_out.clone(), y.clone()
    grad_in, bias_grad = relu_bwd_bias_grad(grad_out, y)
    ref = torch.ops.aten.threshold_backward(grad_out, y, 0)
    assert grad_in.dtype == torch.bfloat16 and grad_in.shape == (b, n)
    assert bias_grad.dtype == torch.bfloat16 and bias_grad.shape == (n,)
    assert torch.equal(grad_in, ref)
    # sign of zero included
    assert torch.equal(grad_in.view(torch.int16), ref.view(torch.int16))
    # inputs untouched (not in place over grad_out)
    assert torch.equal(grad_out, g_before)
    assert torch.equal(y.view(torch.int16), y_before.view(torch.int16))
    _assert_bias_grad_within_bound(bias_grad.cpu(), grad_in.cpu())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("b,n", RELU_SHAPES)
def test_relu_bwd_bias_grad_deterministic(b, n):
    grad_out, y = _relu_inputs(b, n, "cuda")
    g1, b1 = relu_bwd_bias_grad(grad_out, y)
    g2, b2 = relu_bwd_bias_grad(grad_out, y)
    assert torch.equal(g1, g2)
    assert torch.equal(b1, b2)


@pytest.mark.gpu
@requires_gpu
def test_relu_bwd_bias_grad_nan_gradient_column():
    grad_out, y = _relu_inputs(40, 16, "cuda")
    y[5, 3] = 1.0
    grad_out[5, 3] = float("nan")
    grad_in, bias_grad = relu_bwd_bias_grad(grad_out, y)
    assert bool(bias_grad[3].isnan())
    _assert_bias_grad_within_bound(bias_grad.cpu(), grad_in.cpu())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", ["noncontiguous", "n13"])
def test_relu_bwd_bias_grad_fallback(case):
    if case == "noncontiguous":
        go, yy = _relu_inputs(64, 32, "cuda")
        grad_out, y = go[:, ::2], yy[:, ::2]
        assert not grad_out.is_contiguous()
    else:
        grad_out, y = _relu_inputs(50, 13, "cuda")
    grad_in, bias_grad = relu_bwd_bias_grad(grad_out, y)
    ref = torch.ops.aten.threshold_backward(grad_out, y, 0)
    assert torch.equal(grad_in, ref)
    assert torch.equal(bias_grad, ref.sum(0))


def _layers(dims, seed):
    torch.manual_seed(seed)
    mods = []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(nn.ReLU(inplace=True))
    return mods


def _run_mlp(mlp, x, gout):
    for p in mlp.parameters():
        p.grad = None
    xin = x.detach().clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = mlp(xin)
    out.backward(gout)
    grads = {n: p.grad.clone() for n, p in mlp.named_parameters()}
    return out.detach(), xin.grad.clone(), grads


@pytest.mark.gpu
@requires_gpu
def test_mlp_fused_matches_sequential_path(monkeypatch):
    b = 300
    mlp = MLP(*_layers([13, 64, 32, 1], seed=3)).cuda()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(b, 13, generator=g).cuda()
    gout = torch.randn(b, 1, generator=g).bfloat16().cuda()

    monkeypatch.setenv("DE_FUSED_MLP", "1")
    calls = []
    real = mlp_ops.relu_bwd_bias_grad
    monkeypatch.setattr(mlp_ops, "relu_bwd_bias_grad",
                        lambda g, y: calls.append(tuple(g.shape)) or real(g, y))
    out_f, gx_f, grads_f = _run_mlp(mlp, x, gout)
    assert calls == [(b, 32), (b, 64)], "fast path did not run"
    monkeypatch.setenv("DE_FUSED_MLP", "0")
    out_p, gx_p, grads_p = _run_mlp(mlp, x, gout)

    assert out_f.dtype == out_p.dtype == torch.bfloat16
    assert torch.equal(out_f, out_p)
    assert torch.equal(gx_f, gx_p)
    for name in grads_p:
        assert grads_f[name].dtype == torch.float32
        if name.endswith("weight"):
            assert torch.equal(grads_f[name], grads_p[name]), name

    # masked gradient of every layer, by hand on the bf16 operands
    w = [mlp[i].weight.detach().bfloat16() for i in (0, 2, 4)]
    bias = [mlp[i].bias.detach().bfloat16() for i in (0, 2, 4)]
    h1 = torch.relu(torch.addmm(bias[0], x.bfloat16(), w[0].t()))
    h2 = torch.relu(torch.addmm(bias[1], h1, w[1].t()))
    g3 = gout
    g2 = torch.ops.aten.threshold_backward(g3.mm(w[2]), h2, 0)
    g1 = torch.ops.aten.threshold_backward(g2.mm(w[1]), h1, 0)
    for idx, masked in ((0, g1), (2, g2), (4, g3)):
        _assert_bias_grad_within_bound(grads_f[f"{idx}.bias"].cpu(), masked.cpu())


@pytest.mark.gpu
@requires_gpu
def test_mlp_weights_refreshed_inside_graph(monkeypatch):
    monkeypatch.setenv("DE_FUSED_MLP", "1")
    b = 512
    mlp = MLP(*_layers([13, 64, 32, 1], seed=5)).cuda()
    g = torch.Generator().manual_seed(13)
    x = torch.randn(b, 13, generator=g).cuda()
    gout = torch.randn(b, 1, generator=g).bfloat16().cuda()

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = mlp(x)
        out.backward(gout)
        return out

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_out = step()
    graph.replay()
    torch.cuda.synchronize()
    first = static_out.detach().clone()

    with torch.no_grad():
        for p in mlp.parameters():
            p.add_(0.05)
    graph.replay()
    torch.cuda.synchronize()
    second = static_out.detach().clone()

    monkeypatch.setenv("DE_FUSED_MLP", "0")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        expect = mlp(x)
    assert torch.equal(second, expect)
    assert not torch.equal(first, second)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def test_mlp_cpu_path_is_plain_sequential():
    mods = _layers([13, 64, 32, 1], seed=9)
    mlp, seq = MLP(*mods), nn.Sequential(*mods)
    x = torch.randn(20, 13)
    xa = x.clone().requires_grad_(True)
    xb = x.clone().requires_grad_(True)
    out_a = mlp(xa)
    out_a.sum().backward()
    ga = [p.grad.clone() for p in mlp.parameters()]
    for p in mlp.parameters():
        p.grad = None
    out_b = seq(xb)
    out_b.sum().backward()
    gb = [p.grad.clone() for p in seq.parameters()]
    assert torch.equal(out_a, out_b)
    assert torch.equal(xa.grad, xb.grad)
    assert all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_relu_bwd_bias_grad_cpu_fallback():
    g = torch.Generator().manual_seed(2)
    grad_out = torch.randn(9, 16, generator=g)
    y = torch.randn(9, 16, generator=g)
    y[0, 0], y[0, 1], y[0, 2] = 0.0, -0.0, math.nan
    grad_in, bias_grad = relu_bwd_bias_grad(grad_out, y)
    ref = torch.ops.aten.threshold_backward(grad_out, y, 0)
    assert torch.equal(grad_in, ref)
    assert torch.equal(bias_grad, ref.sum(0))
    assert grad_in[0, 0] == 0 and grad_in[0, 1] == 0 and grad_in[0, 2] == grad_out[0, 2]


def test_state_dict_keys_unchanged():
    from distributed_embeddings_amd.models.config import EmbeddingConfig, ModelConfig
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.models.synthetic import SyntheticModel
    dlrm = DLRM([10, 20, 30], embedding_dim=8, bottom_mlp_dims=(16, 8),
                top_mlp_dims=(16, 1), num_numerical=4)
    assert list(dlrm.state_dict().keys()) == [
        "bottom_mlp.0.weight", "bottom_mlp.0.bias",
        "bottom_mlp.2.weight", "bottom_mlp.2.bias",
        "top_mlp.0.weight", "top_mlp.0.bias",
        "top_mlp.2.weight", "top_mlp.2.bias",
        "embeddings.col_layers.0.weight",
    ]
    assert isinstance(dlrm.bottom_mlp, MLP) and isinstance(dlrm.top_mlp, MLP)
    cfg = ModelConfig("t", [EmbeddingConfig(2, [1], 50, 8, False)], [16, 8], 3, None)
    syn = SyntheticModel(cfg)
    assert list(syn.state_dict().keys()) == [
        "embeddings.col_layers.0.weight",
        "mlp.0.weight", "mlp.0.bias", "mlp.2.weight", "mlp.2.bias",
        "mlp.4.weight", "mlp.4.bias",
    ]
    assert isinstance(syn.mlp, MLP)


def test_plain_sequential_state_dict_loads():
    seq = nn.Sequential(*_layers([13, 64, 32, 1], seed=1))
    mlp = MLP(*_layers([13, 64, 32, 1], seed=2))
    result = mlp.load_state_dict(seq.state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    for (na, a), (nb, b) in zip(mlp.state_dict().items(), seq.state_dict().items()):
        assert na == nb and torch.equal(a, b)
    seq.load_state_dict(mlp.state_dict(), strict=True)
