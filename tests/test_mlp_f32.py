"""fp32 MLP backward kernels (csrc/wgrad_splitk_f32.hip, csrc/mlp_ops.hip).

``wgrad_splitk_f32(g [K, M], x [K, N])`` is compared with the fp64 product
``S = g^T x`` within

    |gw - S| <= (K + splitk) 2^-24 (|g|^T |x|)

the worst case of an fp32 sum of that many terms in any order (the output is
fp32, so there is no rounding term), and exactly where the sum is exact.  The
bindings are called directly, so the routing does not hide small shapes.
"""

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.ops import _backend
from distributed_embeddings_amd.ops import mlp as mlp_ops
from distributed_embeddings_amd.ops.mlp import MLP

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

BK = 32
KS = [1, BK - 1, BK, BK + 1, 300, 4099]
# smallest legal output; ragged edges both ways; one full tile; more than one
# tile each way; the 13-column (narrow-load) path
MNS = [(4, 4), (16, 132), (132, 16), (128, 128), (260, 516), (64, 13), (512, 13)]


def _operands(k, m, n, seed=0):
    gen = torch.Generator().manual_seed(seed + 100003 * k + 1009 * m + n)
    return (torch.randn(k, m, generator=gen).cuda(),
            torch.randn(k, n, generator=gen).cuda())


def _small_integers(k, m, n, seed):
    """every product and every partial sum is an integer below 2^24"""
    gen = torch.Generator().manual_seed(seed + k + m + n)
    return (torch.randint(-4, 5, (k, m), generator=gen).float().cuda(),
            torch.randint(-4, 5, (k, n), generator=gen).float().cuda())


def _assert_within_bound(got, g, x, terms, what):
    s = g.double().t() @ x.double()
    bound = terms * 2.0 ** -24 * (g.double().abs().t() @ x.double().abs())
    assert got.dtype == torch.float32 and got.shape == s.shape
    assert not bool(got.isnan().any())
    err = (got.double() - s).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error / bound = {worst:.3f} over {err.numel()} entries")
    assert bool((err <= bound).all()), f"{what}: worst error / bound = {worst}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", MNS)
@pytest.mark.parametrize("k", KS)
def test_wgrad_splitk_f32_vs_fp64(k, m, n):
    ext = _backend.ops()
    g, x = _operands(k, m, n)
    g0, x0 = g.clone(), x.clone()
    gw = ext.wgrad_splitk_f32(g, x)
    splitk = ext.wgrad_splitk_f32_plan(k, m, n)[1]
    _assert_within_bound(gw, g, x, k + splitk, f"K={k} M={m} N={n}")
    assert torch.equal(g, g0) and torch.equal(x, x0), "inputs changed"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n,tiles", [(16, 132, (0, 1)), (260, 516, (0, 1)),
                                       (512, 13, (2,))])
@pytest.mark.parametrize("splitk", [2, 5, 65])
def test_wgrad_splitk_f32_forced_slices_and_tiles(splitk, m, n, tiles):
    # 4099 = 2 x 2080 - 61 = 4 x 832 + 771 = 64 x 64 + 3: ragged last slice
    g, x = _operands(4099, m, n, seed=1)
    gi, xi = _small_integers(4099, m, n, seed=9)
    expect = (gi.double().t() @ xi.double()).float()
    ext = _backend.ops()
    for tile in tiles:
        gw = ext.wgrad_splitk_f32(g, x, splitk, tile)
        _assert_within_bound(gw, g, x, 4099 + splitk,
                             f"splitk={splitk} tile={tile} M={m} N={n}")
        assert torch.equal(gw, ext.wgrad_splitk_f32(g, x, splitk, tile))
        assert torch.equal(ext.wgrad_splitk_f32(gi, xi, splitk, tile), expect)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", [(260, 516), (512, 13)])
@pytest.mark.parametrize("row", [0, 2047, 4098])
def test_wgrad_splitk_f32_single_row_is_exact(row, m, n):
    """g and x nonzero in one row k: gw = fp32(g[k, m] x[k, n]), nothing
    dropped, nothing doubled, nothing transposed."""
    g, x = _operands(4099, m, n, seed=2)
    keep_g, keep_x = g[row].clone(), x[row].clone()
    g.zero_()
    x.zero_()
    g[row], x[row] = keep_g, keep_x
    expect = (keep_g.double()[:, None] * keep_x.double()[None, :]).float()
    for splitk in (0, 5):
        gw = _backend.ops().wgrad_splitk_f32(g, x, splitk)
        assert torch.equal(gw, expect), f"splitk={splitk}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("k,m,n", [(33, 16, 132), (300, 132, 16),
                                   (4099, 260, 516), (4099, 64, 13)])
def test_wgrad_splitk_f32_small_integers_exact(k, m, n):
    g, x = _small_integers(k, m, n, seed=7)
    expect = (g.double().t() @ x.double()).float()
    for splitk in (0, 3):
        assert torch.equal(_backend.ops().wgrad_splitk_f32(g, x, splitk), expect)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("b,n", [(1, 4), (17, 4), (300, 132), (1030, 516)])
def test_relu_bwd_bias_grad_f32(b, n):
    gen = torch.Generator().manual_seed(31 * b + n)
    grad_out = torch.randn(b, n, generator=gen).cuda()
    y = torch.randn(b, n, generator=gen).cuda()
    y[0, 0], y[0, 1], y[0, 2] = 0.0, -0.0, float("nan")
    ext = _backend.ops()
    grad_in, bias_grad = ext.relu_bwd_bias_grad_f32(grad_out, y)
    ref = torch.ops.aten.threshold_backward(grad_out, y, 0)
    assert torch.equal(grad_in, ref)
    assert bias_grad.dtype == torch.float32 and bias_grad.shape == (n,)
    err = (bias_grad.double() - ref.double().sum(0)).abs()
    assert bool((err <= b * 2.0 ** -24 * ref.double().abs().sum(0)).all())
    again = ext.relu_bwd_bias_grad_f32(grad_out, y)
    assert torch.equal(again[0], grad_in) and torch.equal(again[1], bias_grad)

    # a NaN gradient: through where y > 0, stopped where y <= 0, in its column
    y[:, 3] = 1.0
    grad_out[b // 2, 3] = float("nan")
    grad_out[0, 1] = float("nan")
    grad_in, bias_grad = ext.relu_bwd_bias_grad_f32(grad_out, y)
    ref = torch.ops.aten.threshold_backward(grad_out, y, 0)
    assert torch.equal(grad_in.view(torch.int32), ref.view(torch.int32))
    assert bias_grad.isnan().nonzero().flatten().tolist() == [3]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n", [4, 132, 256])
@pytest.mark.parametrize("k", [1, 33, 4099])
def test_wgrad_gemv_f32_vs_fp64(k, n):
    g, x = _operands(k, 1, n, seed=3)
    gw, gb = _backend.ops().wgrad_gemv_f32(g, x)
    _assert_within_bound(gw, g, x, k, f"gemv K={k} N={n}")
    assert gb.dtype == torch.float32 and gb.shape == (1,)
    err = (gb.double() - g.double().sum(0)).abs()
    assert bool((err <= k * 2.0 ** -24 * g.double().abs().sum(0)).all())
    again = _backend.ops().wgrad_gemv_f32(g, x)
    assert torch.equal(again[0], gw) and torch.equal(again[1], gb)


@pytest.mark.gpu
@requires_gpu
def test_f32_ops_reject_what_they_cannot_take():
    ext = _backend.ops()
    g, x = _operands(64, 16, 16)
    y = torch.randn(64, 16).cuda()
    for bad_g, bad_x in [(g.bfloat16(), x.bfloat16()),         # bf16
                         (g[:, :6].contiguous(), x),           # M % 4 != 0
                         (g, torch.cat([x, x[:, :2]], 1)),     # N = 18
                         (g.t(), x.t())]:                      # not contiguous
        with pytest.raises(RuntimeError):
            ext.wgrad_splitk_f32(bad_g, bad_x)
    for bad_g, bad_y in [(g.bfloat16(), y.bfloat16()),
                         (g[:, :6].contiguous(), y[:, :6].contiguous()),
                         (g.t(), y.t())]:
        with pytest.raises(RuntimeError):
            ext.relu_bwd_bias_grad_f32(bad_g, bad_y)
    g1 = g[:, :1].contiguous()
    for bad_g, bad_x in [(g1.bfloat16(), x.bfloat16()),
                         (g1, torch.cat([x, x[:, :2]], 1)),
                         (g1, x.t()[:, :16])]:
        with pytest.raises(RuntimeError):
            ext.wgrad_gemv_f32(bad_g, bad_x)


def test_f32_plans_route_what_was_measured_ahead():
    if not _backend.available():
        pytest.skip("HIP extension not built")
    ext = _backend.ops()
    for m, n in [(512, 13), (256, 512), (128, 256)]:
        assert ext.wgrad_splitk_f32_plan(65536, m, n)[0] == 1
        assert ext.wgrad_splitk_f32_plan(4096, m, n)[0] == 0
    for m, n in [(1024, 512), (512, 1024), (1024, 1024)]:
        assert ext.wgrad_splitk_f32_plan(65536, m, n)[0] == 0
    assert ext.wgrad_splitk_f32_plan(65536, 6, 64)[2] == -1   # M % 4 != 0
    assert ext.wgrad_splitk_f32_plan(65536, 64, 18)[2] == -1  # N % 4 != 0, N > 16
    assert ext.wgrad_gemv_f32_plan(65536, 256)[0] == 1
    assert ext.wgrad_gemv_f32_plan(4096, 256)[0] == 0
    assert ext.wgrad_gemv_f32_plan(65536, 18) == [0, 0]


def _mlp(seed):
    torch.manual_seed(seed)
    dims, mods = [13, 64, 32, 16, 1], []
    for i in range(len(dims) - 1):
        mods.append(nn.Linear(dims[i], dims[i + 1]))
        if i < len(dims) - 2:
            mods.append(nn.ReLU(inplace=True))
    return MLP(*mods).cuda()


def _step(mlp, x, gout):
    for p in mlp.parameters():
        p.grad = None
    x.grad = None
    out = mlp(x)
    out.backward(gout)
    return [out.detach(), x.grad] + [p.grad for p in mlp.parameters()]


def _force_f32_plans(monkeypatch):
    monkeypatch.setenv("DE_FUSED_MLP", "1")
    monkeypatch.setenv("DE_WGRAD_SPLITK", "1")
    monkeypatch.setattr(mlp_ops, "_wgrad_f32_routed", lambda k, m, n: True)
    monkeypatch.setattr(mlp_ops, "_wgrad_gemv_f32_routed", lambda k, n: True)


@pytest.mark.gpu
@requires_gpu
def test_fp32_mlp_runs_on_the_f32_kernels(monkeypatch):
    b = 4099
    mlp = _mlp(seed=21)
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(b, 13, generator=gen).cuda().requires_grad_(True)
    gout = torch.randn(b, 1, generator=gen).cuda()
    _force_f32_plans(monkeypatch)
    ext = _backend.ops()
    calls = {"wgrad_splitk_f32": [], "wgrad_gemv_f32": []}
    for name, seen in calls.items():
        monkeypatch.setattr(
            ext, name, lambda g, xb, real=getattr(ext, name), seen=seen:
            seen.append((g.clone(), xb.clone())) or real(g, xb))
    new = [t.clone() for t in _step(mlp, x, gout)]
    shapes = {k: [(g.shape[1], xb.shape[1]) for g, xb in v] for k, v in calls.items()}
    assert shapes == {"wgrad_splitk_f32": [(16, 32), (32, 64), (64, 13)],
                      "wgrad_gemv_f32": [(1, 16)]}
    operands = calls["wgrad_gemv_f32"] + calls["wgrad_splitk_f32"]

    monkeypatch.setenv("DE_FUSED_MLP", "0")
    plain = _step(mlp, x, gout)
    assert sum(len(v) for v in calls.values()) == 4, "DE_FUSED_MLP=0 ran a kernel"
    assert torch.equal(new[0], plain[0]) and torch.equal(new[1], plain[1])
    # parameters: (weight, bias) of layers 0, 2, 4, 6; operands: last layer first
    for layer, (g, xb) in zip((3, 2, 1, 0), operands):
        gw, gb = new[2 + 2 * layer], new[3 + 2 * layer]
        splitk = ext.wgrad_splitk_f32_plan(b, g.shape[1], xb.shape[1])[1]
        _assert_within_bound(gw, g, xb, b + splitk, f"layer {layer} weight")
        err = (gb.double() - g.double().sum(0)).abs()
        assert bool((err <= b * 2.0 ** -24 * g.double().abs().sum(0)).all())


@pytest.mark.gpu
@requires_gpu
def test_fp32_mlp_step_inside_graph(monkeypatch):
    b = 4099
    mlp = _mlp(seed=23)
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(b, 13, generator=gen).cuda().requires_grad_(True)
    gout = torch.randn(b, 1, generator=gen).cuda()
    _force_f32_plans(monkeypatch)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(mlp, x, gout)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(mlp, x, gout)
    for _ in range(2):
        with torch.no_grad():
            x.copy_(torch.randn(b, 13, generator=gen))
            gout.copy_(torch.randn(b, 1, generator=gen))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [t.clone() for t in static]
        eager = _step(mlp, x, gout)
        assert all(torch.equal(r, e) for r, e in zip(replayed, eager))
