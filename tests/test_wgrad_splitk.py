"""Split-K weight-gradient kernels (csrc/wgrad_splitk.hip, ops/mlp.py).

``wgrad_splitk(g [K, M], x [K, N])`` is compared with the fp64 product
``S = g^T x`` within

    |gw - S| <= 2^-8 |S| + K 2^-24 (|g|^T |x|)

(one bf16 rounding, half-ulp 2^-9, with a factor 2 margin, plus the worst case
of an fp32 sum of K terms in any order), and exactly where the sum is exact.
The binding is called directly, so the routing does not hide small shapes.
"""

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.ops import _backend
from distributed_embeddings_amd.ops import mlp as mlp_ops
from distributed_embeddings_amd.ops.mlp import MLP

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

KS = [1, 63, 64, 65, 300, 4099]
# smallest legal output; ragged edges both ways; one full tile; more than one
# tile each way; the 13-column (narrow-load) path
MNS = [(8, 8), (16, 136), (136, 16), (128, 128), (264, 520), (64, 13), (512, 13)]


def _operands(k, m, n, seed=0):
    gen = torch.Generator().manual_seed(seed + 100003 * k + 1009 * m + n)
    g = torch.randn(k, m, generator=gen).bfloat16().cuda()
    x = torch.randn(k, n, generator=gen).bfloat16().cuda()
    return g, x


def _assert_within_bound(gw, g, x, what):
    s = g.double().t() @ x.double()
    a = g.double().abs().t() @ x.double().abs()
    bound = 2.0 ** -8 * s.abs() + g.shape[0] * 2.0 ** -24 * a
    assert gw.dtype == torch.bfloat16 and gw.shape == s.shape
    got = gw.double()
    assert not bool(got.isnan().any())
    err = (got - s).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error / bound = {worst:.3f} over {err.numel()} entries")
    assert bool((err <= bound).all()), f"{what}: worst error / bound = {worst}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", MNS)
@pytest.mark.parametrize("k", KS)
def test_wgrad_splitk_vs_fp64(k, m, n):
    g, x = _operands(k, m, n)
    g0, x0 = g.clone(), x.clone()
    gw = _backend.ops().wgrad_splitk(g, x)
    _assert_within_bound(gw, g, x, f"K={k} M={m} N={n}")
    assert torch.equal(g, g0) and torch.equal(x, x0), "inputs changed"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", MNS)
@pytest.mark.parametrize("splitk", [2, 5, 65])
def test_wgrad_splitk_forced_slices_vs_fp64(splitk, m, n):
    # 4099 = 2 x 2112 - 125 = 4 x 832 + 771 = 64 x 64 + 3: ragged last slice
    g, x = _operands(4099, m, n, seed=1)
    gw = _backend.ops().wgrad_splitk(g, x, splitk)
    _assert_within_bound(gw, g, x, f"splitk={splitk} M={m} N={n}")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", [(16, 136), (128, 128), (264, 520)])
@pytest.mark.parametrize("tile", [0, 1])
def test_wgrad_splitk_either_tile_vs_fp64(tile, m, n):
    """the 128 x 128 and the 64 x 64 tile where the plan picks the other"""
    g, x = _operands(4099, m, n, seed=8)
    gw = _backend.ops().wgrad_splitk(g, x, 5, tile)
    _assert_within_bound(gw, g, x, f"tile={tile} M={m} N={n}")
    gen = torch.Generator().manual_seed(9)
    g = torch.randint(-4, 5, (4099, m), generator=gen).bfloat16().cuda()
    x = torch.randint(-4, 5, (4099, n), generator=gen).bfloat16().cuda()
    expect = (g.double().t() @ x.double()).float().bfloat16()
    assert torch.equal(_backend.ops().wgrad_splitk(g, x, 5, tile), expect)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("m,n", [(264, 520), (512, 13)])
@pytest.mark.parametrize("row", [0, 2047, 4098])
def test_wgrad_splitk_single_row_is_exact(row, m, n):
    """g nonzero in one row k: gw = bf16(g[k, m] x[k, n]), nothing dropped,
    nothing doubled, nothing transposed."""
    g, x = _operands(4099, m, n, seed=2)
    keep = g[row].clone()
    g.zero_()
    g[row] = keep
    expect = (g[row].double()[:, None] * x[row].double()[None, :]).float().bfloat16()
    for splitk in (0, 5):
        gw = _backend.ops().wgrad_splitk(g, x, splitk)
        assert torch.equal(gw, expect), f"splitk={splitk}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("k,m,n", [(65, 16, 136), (4099, 264, 520), (4099, 64, 13)])
def test_wgrad_splitk_small_integers_exact(k, m, n):
    """every product and every partial sum is an integer below 2^24"""
    gen = torch.Generator().manual_seed(7 + k + m + n)
    g = torch.randint(-4, 5, (k, m), generator=gen).bfloat16().cuda()
    x = torch.randint(-4, 5, (k, n), generator=gen).bfloat16().cuda()
    expect = (g.double().t() @ x.double()).float().bfloat16()
    for splitk in (0, 3):
        assert torch.equal(_backend.ops().wgrad_splitk(g, x, splitk), expect)


@pytest.mark.gpu
@requires_gpu
def test_wgrad_splitk_deterministic():
    g, x = _operands(4099, 264, 520, seed=3)
    a = _backend.ops().wgrad_splitk(g, x, 5)
    b = _backend.ops().wgrad_splitk(g, x, 5)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n", [136, 13])
def test_wgrad_splitk_nan_stays_in_its_row(n):
    g, x = _operands(4099, 136, n, seed=4)
    g[3000, 77] = float("nan")
    gw = _backend.ops().wgrad_splitk(g, x, 5)
    nan_rows = gw.isnan().any(1)
    assert bool(gw[77].isnan().all())
    assert int(nan_rows.sum()) == 1


@pytest.mark.gpu
@requires_gpu
def test_wgrad_splitk_rejects_what_it_cannot_take():
    ext = _backend.ops()
    g, x = _operands(64, 16, 16)
    with pytest.raises(RuntimeError):
        ext.wgrad_splitk(g[:, :12].contiguous(), x)       # M % 8 != 0
    with pytest.raises(RuntimeError):
        ext.wgrad_splitk(g, torch.cat([x, x[:, :4]], 1))  # N = 20
    with pytest.raises(RuntimeError):
        ext.wgrad_splitk(g.t(), x)                         # not contiguous
    with pytest.raises(RuntimeError):
        ext.wgrad_splitk(g.float(), x.float())


@pytest.mark.gpu
@requires_gpu
def test_wgrad_splitk_inside_graph():
    k, m, n = 4099, 136, 264
    g, x = _operands(k, m, n, seed=5)
    ext = _backend.ops()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.wgrad_splitk(g, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.wgrad_splitk(g, x)
    for seed in (6, 7):
        g2, x2 = _operands(k, m, n, seed=seed)
        g.copy_(g2)
        x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        eager = ext.wgrad_splitk(g2, x2)
        assert torch.equal(out.view(torch.int16), eager.view(torch.int16))


def test_plan_leaves_small_batches_to_the_gemm_library():
    if not _backend.available():
        pytest.skip("HIP extension not built")
    ext = _backend.ops()
    for m, n in [(64, 13), (512, 13), (256, 512), (1024, 1024)]:
        assert ext.wgrad_splitk_plan(300, m, n)[0] == 0
        assert ext.wgrad_splitk_plan(2048, m, n)[0] == 0
    assert ext.wgrad_splitk_plan(65536, 12, 64)[2] == -1   # M % 8 != 0
    assert ext.wgrad_splitk_plan(65536, 64, 20)[2] == -1   # N % 8 != 0, N > 16


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
    return out.detach(), xin.grad.clone(), \
        {n: p.grad.clone() for n, p in mlp.named_parameters()}


def _count_op_calls(monkeypatch):
    ext = _backend.ops()
    real = ext.wgrad_splitk
    calls = []

    def counted(g, x, *a):
        calls.append((g.detach().clone(), x.detach().clone()))
        return real(g, x, *a)

    monkeypatch.setattr(ext, "wgrad_splitk", counted)
    return calls


@pytest.mark.gpu
@requires_gpu
def test_mlp_routes_weight_gradients_to_the_kernel(monkeypatch):
    """bottom-MLP-like stack at a small batch, the plan forced on"""
    b = 4099
    mlp = MLP(*_layers([13, 64, 32, 16, 1], seed=21)).cuda()
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(b, 13, generator=gen).cuda()
    gout = torch.randn(b, 1, generator=gen).bfloat16().cuda()

    monkeypatch.setenv("DE_FUSED_MLP", "1")
    monkeypatch.setenv("DE_WGRAD_SPLITK", "1")
    monkeypatch.setattr(mlp_ops, "_wgrad_routed", lambda k, m, n: True)
    calls = _count_op_calls(monkeypatch)
    out_n, gx_n, grads_n = _run_mlp(mlp, x, gout)
    assert [(tuple(g.shape), tuple(xb.shape)) for g, xb in calls] == [
        ((b, 16), (b, 32)), ((b, 32), (b, 64)), ((b, 64), (b, 13))]

    monkeypatch.setenv("DE_WGRAD_SPLITK", "0")
    operands = list(calls)
    del calls[:]
    out_p, gx_p, grads_p = _run_mlp(mlp, x, gout)
    assert calls == [], "DE_WGRAD_SPLITK=0 still ran the kernel"

    assert torch.equal(out_n, out_p)
    assert torch.equal(gx_n, gx_p)
    for idx, (g, xb) in zip((4, 2, 0), operands):
        name = f"{idx}.weight"
        assert grads_n[name].dtype == torch.float32
        assert torch.equal(grads_n[f"{idx}.bias"], grads_p[f"{idx}.bias"])
        # the kernel's gradient against fp64, and against the plain run
        _assert_within_bound(grads_n[name].bfloat16(), g, xb, name)
        a = g.double().abs().t() @ xb.double().abs()
        ref = grads_p[name].double()
        bound = 2.0 ** -8 * ref.abs() + b * 2.0 ** -24 * a
        err = (grads_n[name].double() - ref).abs()
        worst = (err / bound.clamp_min(1e-300)).max().item()
        print(f"{name}: worst |new - plain| / bound = {worst:.3f}")
        assert bool((err <= bound).all()), name
    assert torch.equal(grads_n["6.weight"], grads_p["6.weight"])


@pytest.mark.gpu
@requires_gpu
def test_mlp_keeps_small_batches_on_the_gemm_library(monkeypatch):
    b = 300
    mlp = MLP(*_layers([13, 64, 32, 1], seed=23)).cuda()
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(b, 13, generator=gen).cuda()
    gout = torch.randn(b, 1, generator=gen).bfloat16().cuda()
    monkeypatch.setenv("DE_FUSED_MLP", "1")
    monkeypatch.setenv("DE_WGRAD_SPLITK", "1")
    calls = _count_op_calls(monkeypatch)
    _run_mlp(mlp, x, gout)
    assert calls == []
