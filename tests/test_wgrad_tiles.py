"""The logit layer's gradient kernels (``wgrad_gemv``, csrc/wgrad_splitk.hip,
ops/mlp.py) and the documented split-K plan.

``wgrad_gemv(g [K, 1], x [K, N])`` gives ``gw = bf16(g^T x)`` and
``gb = bf16(sum g)``.  Both are compared with their fp64 values ``S`` within
the bound of ``tests/test_wgrad_splitk.py``,

    |gw - S| <= 2^-8 |S| + K 2^-24 (|g|^T |x|)      (|x| = 1 for gb)

and exactly where the sums are exact.  The binding is called directly, so the
routing does not hide small shapes.  K = 63 makes 2 row chunks, 4099 makes
129; N = 520 needs three column tiles of 256.

This change adds no tile geometry to ``wgrad_splitk``: indices 0, 1 and 2 are
covered by ``tests/test_wgrad_splitk.py``.
"""

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.ops import _backend
from distributed_embeddings_amd.ops import mlp as mlp_ops
from distributed_embeddings_amd.ops.mlp import MLP

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

KS = [1, 63, 4099]
NS = [8, 136, 256, 520]


def _operands(k, n, seed=0):
    gen = torch.Generator().manual_seed(seed + 100003 * k + n)
    g = torch.randn(k, 1, generator=gen).bfloat16().cuda()
    x = torch.randn(k, n, generator=gen).bfloat16().cuda()
    return g, x


def _assert_within_bound(got, s, a, k, what):
    """got against the fp64 value s; a = the same sum over absolute values"""
    bound = 2.0 ** -8 * s.abs() + k * 2.0 ** -24 * a
    assert got.dtype == torch.bfloat16 and got.shape == s.shape, what
    got = got.double()
    assert not bool(got.isnan().any())
    err = (got - s).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{what}: worst error / bound = {worst:.3f} over {err.numel()} entries")
    assert bool((err <= bound).all()), f"{what}: worst error / bound = {worst}"


def _assert_grads_within_bound(gw, gb, g, x, what):
    k = g.shape[0]
    gd, xd = g.double(), x.double()
    _assert_within_bound(gw, gd.t() @ xd, gd.abs().t() @ xd.abs(), k,
                         f"{what} weight")
    _assert_within_bound(gb, gd.sum(0), gd.abs().sum(0), k, f"{what} bias")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", KS)
def test_wgrad_gemv_vs_fp64(k, n):
    g, x = _operands(k, n)
    g0, x0 = g.clone(), x.clone()
    gw, gb = _backend.ops().wgrad_gemv(g, x)
    assert gw.shape == (1, n) and gb.shape == (1,)
    _assert_grads_within_bound(gw, gb, g, x, f"K={k} N={n}")
    assert torch.equal(g, g0) and torch.equal(x, x0), "inputs changed"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("k,n", [(63, 8), (4099, 136), (4099, 520)])
def test_wgrad_gemv_small_integers_exact(k, n):
    """every product and every partial sum is an integer below 2^24"""
    gen = torch.Generator().manual_seed(7 + k + n)
    g = torch.randint(-4, 5, (k, 1), generator=gen).bfloat16().cuda()
    x = torch.randint(-4, 5, (k, n), generator=gen).bfloat16().cuda()
    gw, gb = _backend.ops().wgrad_gemv(g, x)
    assert torch.equal(gw, (g.double().t() @ x.double()).float().bfloat16())
    assert torch.equal(gb, g.double().sum(0).float().bfloat16())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("row", [0, 2047, 4098])
def test_wgrad_gemv_single_row_is_exact(row):
    """g nonzero in one row k: gw = bf16(g[k] x[k, :]), gb = g[k]"""
    g, x = _operands(4099, 264, seed=2)
    keep = g[row].clone()
    g.zero_()
    g[row] = keep
    gw, gb = _backend.ops().wgrad_gemv(g, x)
    expect = (g[row].double()[:, None] * x[row].double()[None, :]).float().bfloat16()
    assert torch.equal(gw, expect)
    assert torch.equal(gb, keep)


@pytest.mark.gpu
@requires_gpu
def test_wgrad_gemv_deterministic():
    g, x = _operands(4099, 520, seed=3)
    a = _backend.ops().wgrad_gemv(g, x)
    b = _backend.ops().wgrad_gemv(g, x)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int16), v.view(torch.int16))


@pytest.mark.gpu
@requires_gpu
def test_wgrad_gemv_rejects_what_it_cannot_take():
    ext = _backend.ops()
    g, x = _operands(64, 16)
    with pytest.raises(RuntimeError):
        ext.wgrad_gemv(g, x[:, :12].contiguous())         # N % 8 != 0
    with pytest.raises(RuntimeError):
        ext.wgrad_gemv(g, x.t().contiguous().t())         # not contiguous
    with pytest.raises(RuntimeError):
        ext.wgrad_gemv(g.float(), x.float())
    with pytest.raises(RuntimeError):
        ext.wgrad_gemv(torch.cat([g, g], 1), x)           # two output features
    with pytest.raises(RuntimeError):
        ext.wgrad_gemv(g[:32], x)                         # K mismatch


@pytest.mark.gpu
@requires_gpu
def test_wgrad_gemv_inside_graph():
    k, n = 4099, 264
    g, x = _operands(k, n, seed=5)
    ext = _backend.ops()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ext.wgrad_gemv(g, x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ext.wgrad_gemv(g, x)
    for seed in (6, 7, 8):
        g2, x2 = _operands(k, n, seed=seed)
        g.copy_(g2)
        x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        eager = ext.wgrad_gemv(g2, x2)
        for u, v in zip(out, eager):
            assert torch.equal(u.view(torch.int16), v.view(torch.int16))


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


def _count_op_calls(monkeypatch, name):
    ext = _backend.ops()
    real = getattr(ext, name)
    calls = []

    def counted(g, x, *a):
        calls.append((g.detach().clone(), x.detach().clone()))
        return real(g, x, *a)

    monkeypatch.setattr(ext, name, counted)
    return calls


@pytest.mark.gpu
@requires_gpu
def test_mlp_routes_the_logit_layer_to_the_kernel(monkeypatch):
    """bottom-MLP-like stack closing with Linear(16, 1), both plans forced on"""
    b = 4099
    mlp = MLP(*_layers([13, 64, 32, 16, 1], seed=31)).cuda()
    gen = torch.Generator().manual_seed(32)
    x = torch.randn(b, 13, generator=gen).cuda()
    gout = torch.randn(b, 1, generator=gen).bfloat16().cuda()

    monkeypatch.setenv("DE_FUSED_MLP", "1")
    monkeypatch.setenv("DE_WGRAD_SPLITK", "1")
    monkeypatch.setattr(mlp_ops, "_wgrad_routed", lambda k, m, n: True)
    monkeypatch.setattr(mlp_ops, "_wgrad_gemv_routed", lambda k, n: True)
    splitk_calls = _count_op_calls(monkeypatch, "wgrad_splitk")
    gemv_calls = _count_op_calls(monkeypatch, "wgrad_gemv")
    out_n, gx_n, grads_n = _run_mlp(mlp, x, gout)
    assert [(tuple(g.shape), tuple(xb.shape)) for g, xb in gemv_calls] == [
        ((b, 1), (b, 16))]
    assert len(splitk_calls) == 3

    monkeypatch.setenv("DE_WGRAD_SPLITK", "0")
    (g, xb), = gemv_calls
    del gemv_calls[:], splitk_calls[:]
    out_p, gx_p, grads_p = _run_mlp(mlp, x, gout)
    assert gemv_calls == [] and splitk_calls == [], \
        "DE_WGRAD_SPLITK=0 still ran a kernel"

    assert torch.equal(out_n, out_p)
    assert torch.equal(gx_n, gx_p)
    assert torch.equal(g, gout)
    gw_n, gb_n = grads_n["6.weight"], grads_n["6.bias"]
    assert gw_n.dtype == torch.float32 and gb_n.dtype == torch.float32
    # the kernels' gradients against fp64, and against the plain run
    _assert_grads_within_bound(gw_n.bfloat16(), gb_n.bfloat16(), g, xb, "6")
    gd, xd = g.double(), xb.double()
    _assert_within_bound(gw_n.bfloat16(), grads_p["6.weight"].double(),
                         gd.abs().t() @ xd.abs(), b, "6.weight new - plain")
    _assert_within_bound(gb_n.bfloat16(), grads_p["6.bias"].double(),
                         gd.abs().sum(0), b, "6.bias new - plain")


@pytest.mark.gpu
@requires_gpu
def test_mlp_keeps_a_small_batch_logit_layer_on_the_library(monkeypatch):
    b = 4099
    mlp = MLP(*_layers([13, 32, 16, 1], seed=33)).cuda()
    gen = torch.Generator().manual_seed(34)
    x = torch.randn(b, 13, generator=gen).cuda()
    gout = torch.randn(b, 1, generator=gen).bfloat16().cuda()
    monkeypatch.setenv("DE_FUSED_MLP", "1")
    monkeypatch.setenv("DE_WGRAD_SPLITK", "1")
    calls = _count_op_calls(monkeypatch, "wgrad_gemv")
    _run_mlp(mlp, x, gout)
    assert calls == []


# (M, N) -> (tile geometry, SPLITK) at K = 65536: the decomposition table of
# docs/KERNELS.md ("wgrad_splitk.hip")
DOCUMENTED_PLAN = {
    (512, 13): (2, 128),
    (256, 512): (0, 64),
    (128, 256): (0, 128),
    (1024, 512): (0, 16),
    (1024, 1024): (0, 8),
    (512, 1024): (0, 16),
}


def test_plan_at_the_flagship_shapes_is_the_documented_one():
    if not _backend.available():
        pytest.skip("HIP extension not built")
    ext = _backend.ops()
    k = 65536
    # the seven _LinearReLU layers (256 x 512 twice) ...
    for m, n in [(512, 13), (256, 512), (128, 256),
                 (1024, 512), (1024, 1024), (512, 1024), (256, 512)]:
        use, splitk, cfg = ext.wgrad_splitk_plan(k, m, n)
        assert use == 1
        assert (cfg, splitk) == DOCUMENTED_PLAN[(m, n)], (m, n)
        np_ = (n + 3) // 4 * 4
        assert splitk * m * np_ * 4 <= k * (m + n) * 2, (m, n)
    # ... and the logit layer: 1024 row chunks, slab [1024, 257] fp32
    use, chunks = ext.wgrad_gemv_plan(k, 256)
    assert (use, chunks) == (1, 1024)
    assert chunks * 257 * 4 <= k * 257 * 2
    assert ext.wgrad_gemv_plan(4099, 16)[0] == 0     # small K: the library
    assert ext.wgrad_gemv_plan(k, 12) == [0, 0]      # N % 8 != 0
