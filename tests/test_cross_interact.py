"""DCN-v2 low-rank cross interaction (ops/cross.py, csrc/mlp_ops.hip,
csrc/cross_ops.hip, DLRM(interaction="cross")).

CPU tests check the module against the formula written out, the hand-derived
backward of the whole-stack function with ``gradcheck`` in float64, the
fallbacks and the model wiring.  GPU tests check the kernels:

* ``gu = G * x0`` bit for bit (the fp32 product of two bf16 values is exact);
* ``acc`` against ``s = acc_old + G * u`` in float64,
  ``|acc - s| <= 2^-8 |s| + 2^-23 (|acc_old| + |G * u|)``: bf16's unit
  roundoff, plus the rounding of the fp32 sum with a factor 2 margin;
* the bias gradient within the bound of ``tests/test_mlp_fused.py``,
  ``|gb - S| <= 2^-8 |S| + B 2^-24 sum_b |gu[b, n]|``.
"""

import copy
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.models.dlrm import DLRM
from distributed_embeddings_amd.ops import _backend
from distributed_embeddings_amd.ops import cross as cross_ops
from distributed_embeddings_amd.ops.cross import (LowRankCrossNet, _CrossStack,
                                                   concat_packed, cross_bwd)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------

def _net64(n, r, layers, seed):
    torch.manual_seed(seed)
    net = LowRankCrossNet(n, num_layers=layers, low_rank=r).double()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for w in net.w:                   # zero by default: make them count
            w.bias.copy_(torch.randn(n, generator=g, dtype=torch.float64))
    return net


def test_cross_net_matches_formula():
    b, n, r, layers = 5, 16, 4, 3
    net = _net64(n, r, layers, seed=1)
    x0 = torch.randn(b, n, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(2))
    x = x0
    for l in range(layers):
        vw, ww, wb = net.v[l].weight, net.w[l].weight, net.w[l].bias
        assert vw.shape == (r, n) and ww.shape == (n, r) and wb.shape == (n,)
        u = (x @ vw.t()) @ ww.t() + wb
        x = x0 * u + x
    torch.testing.assert_close(net(x0), x)


def test_cross_net_init():
    torch.manual_seed(0)
    net = LowRankCrossNet(64, num_layers=2, low_rank=8)
    assert list(net.state_dict().keys()) == [
        "v.0.weight", "v.1.weight",
        "w.0.weight", "w.0.bias", "w.1.weight", "w.1.bias"]
    for w in net.w:
        assert torch.count_nonzero(w.bias) == 0
    assert all(v.bias is None for v in net.v)
    assert all(float(lin.weight.detach().std()) > 0
               for lin in list(net.v) + list(net.w))


@pytest.mark.parametrize("layers", [1, 2, 3])
def test_cross_stack_gradcheck(layers):
    b, n, r = 3, 8, 2
    net = _net64(n, r, layers, seed=10 + layers)
    x0 = torch.randn(b, n, dtype=torch.float64,
                     generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    params = net._params()
    assert len(params) == 3 * layers and all(p.requires_grad for p in params)

    def fn(x, *ps):
        return _CrossStack.apply(x, torch.float64, *ps)

    assert torch.autograd.gradcheck(fn, (x0, *params))


@pytest.mark.parametrize("layers", [1, 3])
def test_cross_stack_matches_unfused_composition(layers):
    b, n, r = 7, 16, 4
    net = _net64(n, r, layers, seed=20)
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(b, n, dtype=torch.float64, generator=g)
    gout = torch.randn(b, n, dtype=torch.float64, generator=g)
    params = net._params()

    xa = x0.clone().requires_grad_(True)
    out_a = _CrossStack.apply(xa, torch.float64, *params)
    grads_a = torch.autograd.grad(out_a, [xa] + params, gout)
    xb = x0.clone().requires_grad_(True)
    out_b = net(xb)                       # CPU: the plain composition
    grads_b = torch.autograd.grad(out_b, [xb] + params, gout)

    torch.testing.assert_close(out_a, out_b)
    for ga, gb in zip(grads_a, grads_b):
        torch.testing.assert_close(ga, gb)


def test_cross_bwd_cpu_fallback_any_dtype():
    g = torch.Generator().manual_seed(5)
    G, x0, u, acc0 = (torch.randn(9, 12, generator=g) for _ in range(4))
    acc = acc0.clone()
    gu, gb = cross_bwd(G, x0, u, acc, init=False)
    assert torch.equal(gu, G * x0) and torch.equal(gb, (G * x0).sum(0))
    assert torch.equal(acc, acc0 + G * u)
    acc = torch.full_like(acc0, float("nan"))
    cross_bwd(G, x0, u, acc, init=True)
    assert torch.equal(acc, G * u)


SIZES4 = [11, 20, 7, 30]


def _small_dlrm(**kw):
    torch.manual_seed(0)
    return DLRM(SIZES4, embedding_dim=8, bottom_mlp_dims=(16, 8),
                top_mlp_dims=(16, 1), num_numerical=4, **kw)


def test_dlrm_cross_cpu_forward_backward(monkeypatch):
    model = _small_dlrm(interaction="cross", cross_layers=2, cross_rank=4)
    assert isinstance(model.cross, LowRankCrossNet)
    assert model.cross.in_features == 5 * 8
    assert model.top_mlp[0].in_features == 64      # 40 padded to 64
    keys = list(model.state_dict().keys())
    for l in range(2):
        assert f"cross.v.{l}.weight" in keys
        assert f"cross.w.{l}.weight" in keys and f"cross.w.{l}.bias" in keys
    g = torch.Generator().manual_seed(6)
    num = torch.rand(6, 4, generator=g)
    cats = [torch.randint(0, s, (6,), generator=g) for s in SIZES4]
    out = model(num, cats)
    assert out.shape == (6, 1)
    out.square().sum().backward()
    for name, p in model.named_parameters():
        assert p.grad is not None, name
    # the list branch (no packed view) computes the same thing
    assert model._dot_perm is not None
    monkeypatch.setenv("DE_PACKED", "0")
    legacy = _small_dlrm(interaction="cross", cross_layers=2, cross_rank=4)
    assert legacy._dot_perm is None
    legacy.load_state_dict(model.state_dict())
    legacy.embeddings.set_weights(model.embeddings.get_weights(all_ranks=True))
    torch.testing.assert_close(legacy(num, cats), out)


def test_dlrm_cross_no_padding_at_multiple_of_64():
    torch.manual_seed(0)
    model = DLRM([9, 9, 9], embedding_dim=16, bottom_mlp_dims=(16,),
                 top_mlp_dims=(8, 1), num_numerical=4, interaction="cross",
                 cross_layers=1, cross_rank=2)
    assert model.interact_pad == 64 == model.cross.in_features


def test_dlrm_default_keys_unchanged():
    model = _small_dlrm()
    assert model.cross is None
    assert list(model.state_dict().keys()) == [
        "bottom_mlp.0.weight", "bottom_mlp.0.bias",
        "bottom_mlp.2.weight", "bottom_mlp.2.bias",
        "top_mlp.0.weight", "top_mlp.0.bias",
        "top_mlp.2.weight", "top_mlp.2.bias",
        "embeddings.col_layers.0.weight",
    ]
    assert [n for n, _ in model.named_children()] == [
        "bottom_mlp", "top_mlp", "embeddings"]
    # the dot interaction's width: 5 * 4 / 2 + 8 = 18, padded to 64
    assert model.top_mlp[0].in_features == 64
    # the constructor's own defaults
    torch.manual_seed(0)
    full = DLRM([10, 20, 30])
    assert list(full.state_dict().keys()) == [
        "bottom_mlp.0.weight", "bottom_mlp.0.bias",
        "bottom_mlp.2.weight", "bottom_mlp.2.bias",
        "bottom_mlp.4.weight", "bottom_mlp.4.bias",
        "top_mlp.0.weight", "top_mlp.0.bias",
        "top_mlp.2.weight", "top_mlp.2.bias",
        "top_mlp.4.weight", "top_mlp.4.bias",
        "top_mlp.6.weight", "top_mlp.6.bias",
        "top_mlp.8.weight", "top_mlp.8.bias",
        "embeddings.col_layers.0.weight",
    ]
    assert full.top_mlp[0].in_features == 192      # 4 * 3 / 2 + 128 = 134


def test_dlrm_bad_interaction_raises():
    with pytest.raises(ValueError):
        _small_dlrm(interaction="dcn")


@pytest.mark.parametrize("sample_major", [False, True])
def test_concat_packed_fallback(sample_major):
    b, p, d = 5, 3, 4
    g = torch.Generator().manual_seed(7)
    feats = [torch.randn(b, d, generator=g) for _ in range(p)]  # packed rows
    bottom = torch.randn(b, d, generator=g).requires_grad_(True)
    packed = torch.stack(feats, dim=1 if sample_major else 0).requires_grad_(True)
    perm = torch.tensor([2, 0, 1], dtype=torch.int32)
    x0 = concat_packed(packed, bottom, perm, sample_major=sample_major)
    expect = torch.cat([bottom.detach(), feats[2], feats[0], feats[1]], dim=1)
    assert torch.equal(x0, expect)
    gout = torch.randn(b, (p + 1) * d, generator=g)
    gbottom, gpacked = torch.autograd.grad(x0, [bottom, packed], gout)
    assert torch.equal(gbottom, gout[:, :d])
    for f, row in enumerate(perm.tolist()):
        piece = gout[:, (f + 1) * d:(f + 2) * d]
        got = gpacked[:, row] if sample_major else gpacked[row]
        assert torch.equal(got, piece)


def test_dlrm_example_cross_smoke():
    proc = subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "dlrm_main.py"),
         "--batch-size", "128", "--num-batches", "3", "--embedding-dim", "16",
         "--table-size-cap", "1000", "--interaction", "cross",
         "--cross-layers", "2", "--cross-rank", "8"],
        capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert proc.returncode == 0, (
        f"dlrm_main.py failed:\n{proc.stdout[-2000:]}\n{proc.stderr[-2000:]}")
    assert "loss" in proc.stdout


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------

def _assert_bias_grad_within_bound(bias_grad, grad_in):
    """bias_grad [N] against the fp64 column sum of grad_in [B, N]."""
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


def _cross_inputs(b, n):
    g = torch.Generator().manual_seed(1000 * b + n)
    return tuple(torch.randn(b, n, generator=g).bfloat16().cuda() for _ in range(4))


CROSS_SHAPES = [(1, 8), (3, 8), (257, 136), (4099, 128), (300, 3456)]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("b,n", CROSS_SHAPES)
def test_cross_bwd_kernel(b, n, init):
    G, x0, u, acc_old = _cross_inputs(b, n)
    before = [t.clone() for t in (G, x0, u)]

    def run(fn):
        acc = torch.full_like(acc_old, float("nan")) if init else acc_old.clone()
        gu, gb = fn(G, x0, u, acc, init)
        return gu, gb, acc

    gu, gb, acc = run(_backend.ops().cross_bwd)      # the kernel itself
    assert gu.dtype == torch.bfloat16 and gu.shape == (b, n)
    assert gb.dtype == torch.bfloat16 and gb.shape == (n,)

    ref_gu = G * x0
    assert torch.equal(gu.view(torch.int16), ref_gu.view(torch.int16))

    gw = G.double() * u.double()
    old = torch.zeros_like(gw) if init else acc_old.double()
    s = old + gw
    assert bool(torch.isfinite(acc).all())
    err = (acc.double() - s).abs()
    bound = 2.0 ** -8 * s.abs() + 2.0 ** -23 * (old.abs() + gw.abs())
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"acc: worst error / bound = {worst:.3f} over {err.numel()} elements")
    assert bool((err <= bound).all()), f"worst error / bound = {worst}"

    _assert_bias_grad_within_bound(gb.cpu(), gu.cpu())

    for t, t0 in zip((G, x0, u), before):
        assert torch.equal(t.view(torch.int16), t0.view(torch.int16))
    # a second call, through the op (whose gate these inputs pass), agrees
    assert cross_ops._bf16_2d_ok(G, x0, u, acc_old) and cross_ops._enabled()
    gu2, gb2, acc2 = run(cross_bwd)
    assert torch.equal(gu, gu2) and torch.equal(gb, gb2)
    assert torch.equal(acc.view(torch.int16), acc2.view(torch.int16))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", ["n12", "noncontiguous"])
@pytest.mark.parametrize("init", [True, False])
def test_cross_bwd_fallback_gate(case, init):
    if case == "n12":
        G, x0, u, acc_old = _cross_inputs(50, 12)
    else:
        full = _cross_inputs(64, 32)
        G = full[0][:, ::2]
        assert not G.is_contiguous()
        x0, u, acc_old = (t[:, :16].contiguous() for t in full[1:])
    acc = acc_old.clone()
    gu, gb = cross_bwd(G, x0, u, acc, init)
    ref_gu = G * x0
    assert torch.equal(gu, ref_gu)
    assert torch.equal(gb, ref_gu.sum(0))
    expect = (G * u) if init else acc_old.clone().add_(G * u)
    assert torch.equal(acc, expect)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("sample_major", [False, True])
@pytest.mark.parametrize("b", [1, 257])
@pytest.mark.parametrize("d", [8, 128])
@pytest.mark.parametrize("p", [1, 26, 33])
def test_cross_concat_kernels(p, d, b, sample_major, monkeypatch):
    g = torch.Generator().manual_seed(100 * p + d + b)
    shape = (b, p, d) if sample_major else (p, b, d)
    packed = torch.randn(shape, generator=g).bfloat16().cuda()
    bottom = torch.randn(b, d, generator=g).bfloat16().cuda()
    perm = torch.randperm(p, generator=g).to(torch.int32).cuda()
    gx0 = torch.randn(b, (p + 1) * d, generator=g).bfloat16().cuda()
    ext = _backend.ops()

    sel = packed.index_select(1, perm.long()) if sample_major else \
        packed.index_select(0, perm.long()).transpose(0, 1)
    expect = torch.cat([bottom, sel.reshape(b, -1)], dim=1)
    x0 = ext.cross_concat_fwd(bottom, packed, perm, sample_major)
    assert x0.shape == (b, (p + 1) * d) and x0.dtype == torch.bfloat16
    assert torch.equal(x0.view(torch.int16), expect.view(torch.int16))

    gbottom, gpacked = ext.cross_concat_bwd(gx0, perm, sample_major)
    assert gbottom.shape == bottom.shape and gpacked.shape == packed.shape
    assert torch.equal(gbottom, gx0[:, :d])
    pieces = gx0[:, d:].reshape(b, p, d)          # piece f-1 -> packed row perm[f-1]
    inv = torch.empty_like(perm, dtype=torch.long)
    inv[perm.long()] = torch.arange(p, device="cuda")
    want = pieces.index_select(1, inv)
    if not sample_major:
        want = want.transpose(0, 1)
    assert torch.equal(gpacked, want)

    # the op: kernels under autograd == the index_select + cat fallback
    def run():
        pk = packed.clone().requires_grad_(True)
        bt = bottom.clone().requires_grad_(True)
        out = concat_packed(pk, bt, perm, sample_major=sample_major)
        return (out.detach(),) + torch.autograd.grad(out, [bt, pk], gx0)

    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    seen = []
    real_apply = cross_ops._ConcatPacked.apply
    monkeypatch.setattr(cross_ops._ConcatPacked, "apply",
                        lambda *a: seen.append(1) or real_apply(*a))
    fused = run()
    assert seen == [1], "kernel path did not run"
    monkeypatch.setenv("DE_FUSED_CROSS", "0")
    plain = run()
    assert seen == [1]
    for a, c in zip(fused, plain):
        assert torch.equal(a, c)


def _run_net(net, x0, gout):
    xin = x0.detach().clone().requires_grad_(True)
    params = net._params()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = net(xin)
    grads = torch.autograd.grad(out, [xin] + params, gout)
    return [out.detach()] + [t.detach() for t in grads]


def _rel_err(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.gpu
@requires_gpu
def test_cross_net_autocast_error_vs_unfused(monkeypatch):
    b, n, r, layers = 512, 256, 32, 3
    torch.manual_seed(31)
    net = LowRankCrossNet(n, num_layers=layers, low_rank=r)
    g = torch.Generator().manual_seed(32)
    with torch.no_grad():
        for w in net.w:
            w.bias.copy_(0.1 * torch.randn(n, generator=g))
    x0 = torch.randn(b, n, generator=g).bfloat16()
    gout = torch.randn(b, n, generator=g).bfloat16()

    net64 = copy.deepcopy(net).double()
    x64 = x0.double().requires_grad_(True)
    out64 = net64(x64)
    ref = [out64.detach()] + list(torch.autograd.grad(
        out64, [x64] + net64._params(), gout.double()))

    net = net.cuda()
    calls = []
    real = cross_ops.cross_bwd
    monkeypatch.setattr(cross_ops, "cross_bwd",
                        lambda *a: calls.append(a[4]) or real(*a))
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    fused = _run_net(net, x0.cuda(), gout.cuda())
    assert calls == [True, False, False], "fused path did not run"
    monkeypatch.setenv("DE_FUSED_CROSS", "0")
    plain = _run_net(net, x0.cuda(), gout.cuda())
    assert len(calls) == 3

    names = ["out", "x0.grad"]
    for l in range(layers):
        names += [f"v.{l}.weight.grad", f"w.{l}.weight.grad", f"w.{l}.bias.grad"]
    bad = []
    for name, f, p, want in zip(names, fused, plain, ref):
        assert f.shape == want.shape and f.dtype == p.dtype, name
        ef, ep = _rel_err(f, want), _rel_err(p, want)
        print(f"{name}: fused {ef:.3e}  unfused {ep:.3e}  ratio {ef / ep:.2f}")
        if not ef <= 2 * ep:
            bad.append((name, ef, ep))
    assert not bad, bad


@pytest.mark.gpu
@requires_gpu
def test_cross_net_graph_capture(monkeypatch):
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    b, n, r, layers = 256, 128, 16, 3
    torch.manual_seed(41)
    net = LowRankCrossNet(n, num_layers=layers, low_rank=r).cuda()
    g = torch.Generator().manual_seed(42)
    x = torch.randn(b, n, generator=g).bfloat16().cuda().requires_grad_(True)
    gout = torch.randn(b, n, generator=g).bfloat16().cuda()
    params = net._params()

    def step():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = net(x)
        return (out,) + torch.autograd.grad(out, [x] + params, gout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    graph.replay()
    torch.cuda.synchronize()
    first = [t.detach().clone() for t in static]

    with torch.no_grad():
        x.copy_(torch.randn(b, n, generator=g).bfloat16())
        gout.copy_(torch.randn(b, n, generator=g).bfloat16())
    graph.replay()
    torch.cuda.synchronize()
    second = [t.detach().clone() for t in static]
    eager = step()
    torch.cuda.synchronize()
    assert not torch.equal(first[0], second[0])
    for got, want in zip(second, eager):
        assert torch.equal(got, want.detach())


@pytest.mark.gpu
@requires_gpu
def test_dlrm_cross_gpu_train_step(monkeypatch):
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    sizes = [100, 37, 500, 64]
    torch.manual_seed(0)
    model = DLRM(sizes, embedding_dim=32, bottom_mlp_dims=(64, 32),
                 top_mlp_dims=(64, 1), num_numerical=13, interaction="cross",
                 cross_layers=3, cross_rank=16).cuda()
    b = 64
    g = torch.Generator().manual_seed(51)
    num = torch.rand(b, 13, generator=g).cuda()
    cats = [torch.randint(0, s, (b,), generator=g).cuda() for s in sizes]
    labels = torch.randint(0, 2, (b, 1), generator=g).float().cuda()
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}

    calls = []
    real = cross_ops.cross_bwd
    monkeypatch.setattr(cross_ops, "cross_bwd",
                        lambda *a: calls.append(tuple(a[0].shape)) or real(*a))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(num, cats)
        loss = nn.functional.binary_cross_entropy_with_logits(
            logits.float(), labels)
    loss.backward()
    assert calls == [(b, 5 * 32)] * 3, "fused cross path did not run"
    assert torch.isfinite(loss).item()
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        grad = p.grad.to_dense() if p.grad.is_sparse else p.grad
        assert bool(torch.isfinite(grad).all()), name
        assert float(grad.abs().max()) > 0, name
    opt.step()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[name]), name
