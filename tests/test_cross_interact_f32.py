"""The fp32 lane of the DCN-v2 cross interaction (ops/cross.py,
``cross_bwd_partial_f32`` in csrc/mlp_ops.hip, csrc/cross_ops.hip) on the GPU,
against the rounding contract of docs/KERNELS.md, "fp32 inputs"."""

import copy

import pytest
import torch
from torch import nn

from distributed_embeddings_amd.models.dlrm import DLRM
from distributed_embeddings_amd.ops import _backend
from distributed_embeddings_amd.ops import cross as cross_ops
from distributed_embeddings_amd.ops.cross import (LowRankCrossNet,
                                                   concat_packed, cross_bwd)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")]
F32 = torch.float32


def _inputs(b, n, dtypes=(F32,) * 4):
    g = torch.Generator().manual_seed(1000 * b + n)
    return [torch.randn(b, n, generator=g).to(dt).cuda() for dt in dtypes]


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("b,n", [(1, 4), (3, 4), (257, 68), (4099, 128),
                                 (300, 3456)])
def test_cross_bwd_f32_kernel(b, n, init):
    G, x0, u, acc_old = _inputs(b, n)
    before = [t.clone() for t in (G, x0, u)]

    def run(fn):
        acc = torch.full_like(acc_old, float("nan")) if init else acc_old.clone()
        return (*fn(G, x0, u, acc, init), acc)

    gu, gb, acc = run(_backend.ops().cross_bwd_f32)   # the kernel itself
    assert torch.equal(_bits(gu), _bits(G * x0))
    assert bool(torch.isfinite(acc).all())
    if init:
        assert torch.equal(_bits(acc), _bits(G * u))
    else:
        gw, old = G.double() * u.double(), acc_old.double()
        err = (acc.double() - (old + gw)).abs()
        bound = 2.0 ** -23 * (old.abs() + gw.abs())
        print("acc: worst error / bound", (err / bound.clamp_min(1e-300)).max().item())
        assert bool((err <= bound).all())
    gud = gu.double()
    err = (gb.double() - gud.sum(0)).abs()
    bound = b * 2.0 ** -24 * gud.abs().sum(0)
    print("gb: worst error / bound", (err / bound.clamp_min(1e-300)).max().item())
    assert gb.dtype == F32 and bool((err <= bound).all())
    for t, t0 in zip((G, x0, u), before):
        assert torch.equal(_bits(t), _bits(t0))
    # a second call, through the op (whose fp32 gate these inputs pass), agrees
    assert cross_ops._f32_2d_ok(G, x0, u, acc_old) and cross_ops._enabled()
    for first, second in zip((gu, gb, acc), run(cross_bwd)):
        assert torch.equal(_bits(first), _bits(second))


@pytest.mark.parametrize("case", ["n6", "noncontiguous", "mixed"])
@pytest.mark.parametrize("init", [True, False])
def test_cross_bwd_f32_fallback_gate(case, init, monkeypatch):
    monkeypatch.setattr(_backend.ops(), "cross_bwd_f32",
                        lambda *a: pytest.fail("the kernel ran"))
    if case == "n6":
        G, x0, u, acc_old = _inputs(50, 6)
    elif case == "noncontiguous":
        full = _inputs(64, 32)
        G = full[0][:, ::2]
        x0, u, acc_old = (t[:, :16].contiguous() for t in full[1:])
    else:
        G, x0, u, acc_old = _inputs(64, 16, (F32, F32, torch.bfloat16, F32))
    acc = acc_old.clone()
    gu, gb = cross_bwd(G, x0, u, acc, init)
    assert torch.equal(gu, G * x0) and torch.equal(gb, (G * x0).sum(0))
    assert torch.equal(acc, G * u if init else acc_old.clone().add_(G * u))


@pytest.mark.parametrize("sample_major", [False, True])
@pytest.mark.parametrize("b", [1, 257])
@pytest.mark.parametrize("d", [4, 128])
@pytest.mark.parametrize("p", [1, 26, 33])
def test_cross_concat_f32_kernels(p, d, b, sample_major, monkeypatch):
    g = torch.Generator().manual_seed(100 * p + d + b)
    packed = torch.randn((b, p, d) if sample_major else (p, b, d), generator=g).cuda()
    bottom = torch.randn(b, d, generator=g).cuda()
    perm = torch.randperm(p, generator=g).to(torch.int32).cuda()
    gx0 = torch.randn(b, (p + 1) * d, generator=g).cuda()
    ext = _backend.ops()

    sel = packed.index_select(1, perm.long()) if sample_major else \
        packed.index_select(0, perm.long()).transpose(0, 1)
    x0 = ext.cross_concat_f32_fwd(bottom, packed, perm, sample_major)
    assert torch.equal(_bits(x0), _bits(torch.cat([bottom, sel.reshape(b, -1)], 1)))

    gbottom, gpacked = ext.cross_concat_f32_bwd(gx0, perm, sample_major)
    inv = torch.empty_like(perm, dtype=torch.long)
    inv[perm.long()] = torch.arange(p, device="cuda")
    want = gx0[:, d:].reshape(b, p, d).index_select(1, inv)  # piece f-1 -> row perm[f-1]
    assert torch.equal(gbottom, gx0[:, :d])
    assert torch.equal(gpacked, want if sample_major else want.transpose(0, 1))

    def run():          # the op: kernels under autograd == index_select + cat
        pk = packed.clone().requires_grad_(True)
        bt = bottom.clone().requires_grad_(True)
        out = concat_packed(pk, bt, perm, sample_major=sample_major)
        return (out.detach(),) + torch.autograd.grad(out, [bt, pk], gx0)

    seen = []
    real_apply = cross_ops._ConcatPackedF32.apply
    monkeypatch.setattr(cross_ops._ConcatPackedF32, "apply",
                        lambda *a: seen.append(1) or real_apply(*a))
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    fused = run()
    monkeypatch.setenv("DE_FUSED_CROSS", "0")
    plain = run()
    assert seen == [1], "the kernel path has to run exactly once"
    assert all(torch.equal(a, c) for a, c in zip(fused, plain))


def _net_io(b, n, seed):
    torch.manual_seed(seed)
    net = LowRankCrossNet(n, num_layers=3, low_rank=16)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for w in net.w:                   # zero by default: make them count
            w.bias.copy_(0.1 * torch.randn(n, generator=g))
    return net, torch.randn(b, n, generator=g), torch.randn(b, n, generator=g)


def _step(net, x, gout):
    out = net(x)
    grads = torch.autograd.grad(out, [x] + net._params(), gout)
    return [t.detach() for t in (out, *grads)]    # out, x0.grad, (V, W, b) per layer


def test_cross_net_f32_error_vs_unfused(monkeypatch):
    net, x0, gout = _net_io(261, 72, 31)
    ref = _step(copy.deepcopy(net).double(), x0.double().requires_grad_(True),
                gout.double())
    net, x0, gout = net.cuda(), x0.cuda().requires_grad_(True), gout.cuda()
    calls = []
    real, kernel = cross_ops.cross_bwd, _backend.ops().cross_bwd_f32
    monkeypatch.setattr(cross_ops, "cross_bwd",
                        lambda *a: calls.append(a[4]) or real(*a))
    monkeypatch.setattr(_backend.ops(), "cross_bwd_f32",
                        lambda *a: calls.append("f32") or kernel(*a))
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    fused = _step(net, x0, gout)
    assert calls == [True, "f32", False, "f32", False, "f32"], "fused lane did not run"
    monkeypatch.setenv("DE_FUSED_CROSS", "0")
    plain = _step(net, x0, gout)
    assert len(calls) == 6
    bad = []
    for i, (f, p, want) in enumerate(zip(fused, plain, ref)):
        ef, ep = (((t.double().cpu() - want).abs().max() / want.abs().max()).item()
                  for t in (f, p))
        print(f"tensor {i}: fused {ef:.3e}  unfused {ep:.3e}  ratio {ef / ep:.2f}")
        if f.dtype != F32 or not ef <= 2 * ep:
            bad.append((i, ef, ep))
    assert not bad, bad


def test_cross_net_f32_graph_capture(monkeypatch):
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    net, x, gout = _net_io(256, 128, 41)
    net, x, gout = net.cuda(), x.cuda().requires_grad_(True), gout.cuda()
    assert net._fused(x) == F32
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _step(net, x, gout)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = _step(net, x, gout)
    replays = []
    for _ in range(2):                    # the second replay on new inputs
        graph.replay()
        torch.cuda.synchronize()
        replays.append([t.clone() for t in static])
        with torch.no_grad():
            x.copy_(torch.randn_like(x))
            gout.copy_(torch.randn_like(gout))
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(replays[0][0], static[0])
    assert all(torch.equal(got, want) for got, want in zip(static, _step(net, x, gout)))


def test_dlrm_cross_f32_reaches_f32_kernels(monkeypatch):
    """The logits against the DE_FUSED_CROSS=0 run, within 1e-4 max|logit| (the
    criterion of test_dlrm_fp32_reaches_f32_kernels; no float64 model copy)."""
    monkeypatch.setenv("DE_FUSED_CROSS", "1")
    sizes, b = [100, 37, 500, 64], 64
    torch.manual_seed(0)
    model = DLRM(sizes, embedding_dim=32, bottom_mlp_dims=(64, 32),
                 top_mlp_dims=(64, 1), num_numerical=13, interaction="cross",
                 cross_layers=3, cross_rank=16).cuda()
    g = torch.Generator().manual_seed(51)
    num = torch.rand(b, 13, generator=g).cuda()
    cats = [torch.randint(0, s, (b,), generator=g).cuda() for s in sizes]
    labels = torch.randint(0, 2, (b, 1), generator=g).float().cuda()
    ext = _backend.ops()
    calls, concats = [], []
    kernel, concat = ext.cross_bwd_f32, ext.cross_concat_f32_fwd
    monkeypatch.setattr(ext, "cross_bwd_f32",
                        lambda *a: calls.append(tuple(a[0].shape)) or kernel(*a))
    monkeypatch.setattr(ext, "cross_concat_f32_fwd",
                        lambda *a: concats.append(1) or concat(*a))
    logits = model(num, cats)
    nn.functional.binary_cross_entropy_with_logits(logits, labels).backward()
    assert logits.dtype == F32 and calls == [(b, 5 * 32)] * 3
    assert concats == [1] * (model._dot_perm is not None)
    for name, p in model.named_parameters():
        grad = p.grad.to_dense() if p.grad.is_sparse else p.grad
        assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0, name
    monkeypatch.setenv("DE_FUSED_CROSS", "0")
    with torch.no_grad():
        ref = model(num, cats)
    assert len(calls) == 3
    err = float((logits.detach() - ref).abs().max())
    print("logit err", err, "max", float(ref.abs().max()))
    assert err <= 1e-4 * float(ref.abs().max())
