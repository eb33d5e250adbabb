"""fp32 interaction kernels (F <= 32, D % 8 == 0, 8 <= D <= 256) against float64.

An fp32 sum of n terms is off by at most n * 2**-24 * sum|terms|; with a
factor 2 for the roundings of the products, against a float64 reference of the
same fp32 inputs

    forward:   |out - ref| <= D  * 2**-23 * sum_d |x_id * x_jd|
    backward:  |g - ref|   <= 33 * 2**-23 * sum_k |terms|

(32 features plus the bottom-concat gradient; F + 1 terms where the torch
fallback sums more than 32 features).  The bottom block is a bit copy, the
pad exact zeros, and a repeated call gives the same bits.
"""

import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")


def _reference(feats, gout, out_w):
    """float64 forward / backward of ``feats [B, F, D]``, ``gout [B, out_w]``,
    each with the sum of absolute terms per element."""
    b, f, d = feats.shape
    tri_n = f * (f - 1) // 2
    x, gd = feats.double(), gout.double()
    ii, jj = torch.tril_indices(f, f, offset=-1)
    ref = torch.zeros(b, out_w, dtype=torch.float64)
    mag = torch.zeros(b, out_w, dtype=torch.float64)
    ref[:, :tri_n] = (x @ x.transpose(1, 2))[:, ii, jj]
    mag[:, :tri_n] = (x.abs() @ x.abs().transpose(1, 2))[:, ii, jj]
    ref[:, tri_n:tri_n + d] = x[:, 0]
    gs = torch.zeros(b, f, f, dtype=torch.float64)
    gs[:, ii, jj] = gd[:, :tri_n]
    gs = gs + gs.transpose(1, 2)
    ref_g, mag_g = gs @ x, gs.abs() @ x.abs()
    ref_g[:, 0] += gd[:, tri_n:tri_n + d]
    mag_g[:, 0] += gd[:, tri_n:tri_n + d].abs()
    return ref, mag, ref_g, mag_g


def _inputs(b, f, d, padded, seed=0, dtype=torch.float32):
    """feats [B, F, D] in model order, gout, a non-identity perm, out_w."""
    width = f * (f - 1) // 2 + d
    out_w = (width + 63) // 64 * 64 if padded else width
    g = torch.Generator().manual_seed(seed + 1000 * b + 40 * f + d + int(padded))
    feats = torch.randn(b, f, d, generator=g).to(dtype)
    gout = torch.randn(b, out_w, generator=g).to(dtype)
    perm = torch.arange(f - 1, dtype=torch.int32).roll(3 % max(f - 1, 1)).flip(0)
    return feats, gout, perm, out_w


def _pack(feats, perm, sm):
    """(bottom, packed) on the GPU: packed row perm[i] holds model feature i + 1."""
    b, f, d = feats.shape
    rows = torch.empty(b, f - 1, d, dtype=feats.dtype)
    rows[:, perm.long()] = feats[:, 1:]
    packed = (rows if sm else rows.transpose(0, 1)).contiguous().cuda()
    return feats[:, 0].contiguous().cuda(), packed


def _unpack(gbottom, gpacked, perm, sm):
    grows = gpacked.cpu() if sm else gpacked.cpu().transpose(0, 1)
    return torch.cat([gbottom.cpu().unsqueeze(1), grows[:, perm.long()]], 1)


def _run(ext, layout, feats, gout, perm, out_w):
    """(out, gfeats [B, F, D]) of the f32 bindings for one layout, on CPU."""
    if layout == "stacked":
        fc = feats.cuda()
        out = ext.dot_interact_f32_fwd(fc, out_w)
        return out.cpu(), ext.dot_interact_f32_bwd(gout.cuda(), fc).cpu()
    sm = layout == "sm"
    bottom, packed = _pack(feats, perm, sm)
    out = ext.dot_interact_f32_fwd_packed(bottom, packed, perm.cuda(), out_w, sm)
    gbottom, gpacked = ext.dot_interact_f32_bwd_packed(
        gout.cuda(), bottom, packed, perm.cuda(), sm)
    return out.cpu(), _unpack(gbottom, gpacked, perm, sm)


def _check(out, gfeats, feats, gout, out_w):
    b, f, d = feats.shape
    tri_n = f * (f - 1) // 2
    ref, mag, ref_g, mag_g = _reference(feats, gout, out_w)
    err = (out.double() - ref).abs()[:, :tri_n]
    print("fwd max err / bound:",
          float((err / (d * 2.0 ** -23 * mag[:, :tri_n]).clamp_min(1e-300)).max())
          if tri_n else 0.0)
    assert (err <= d * 2.0 ** -23 * mag[:, :tri_n]).all()
    if gfeats is not None:
        err_g = (gfeats.double() - ref_g).abs()
        bound_g = max(33, f + 1) * 2.0 ** -23 * mag_g
        print("bwd max err / bound:", float((err_g / bound_g.clamp_min(1e-300)).max()))
        assert (err_g <= bound_g).all()


@gpu
@requires_gpu
@pytest.mark.parametrize("padded", (False, True), ids=("exact", "pad64"))
@pytest.mark.parametrize("b", (5, 261))
@pytest.mark.parametrize("layout", ("stacked", "fm", "sm"))
@pytest.mark.parametrize("f", (2, 17, 27, 32))
@pytest.mark.parametrize("d", (8, 40, 128, 256))
def test_f32_against_float64(d, f, layout, b, padded):
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    feats, gout, perm, out_w = _inputs(b, f, d, padded)
    tri_n = f * (f - 1) // 2
    out, gfeats = _run(ext, layout, feats, gout, perm, out_w)
    _check(out, gfeats, feats, gout, out_w)
    assert torch.equal(out[:, tri_n:tri_n + d].view(torch.int32),
                       feats[:, 0].view(torch.int32))
    assert (out[:, tri_n + d:].view(torch.int32) == 0).all()
    out2, gfeats2 = _run(ext, layout, feats, gout, perm, out_w)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(gfeats.view(torch.int32), gfeats2.view(torch.int32))


@gpu
@requires_gpu
@pytest.mark.parametrize("sm", (False, True), ids=("fm", "sm"))
def test_public_op_routes_to_f32(sm, monkeypatch):
    """dot_interact_packed on fp32 at F = 27, D = 128: the f32 bindings' bits
    under autograd; with DE_DI_F32=0 the torch composition, within the same
    bounds."""
    from distributed_embeddings_amd.ops import _backend
    from distributed_embeddings_amd.ops import dot_interact as mod
    ext = _backend.ops()
    b, f, d = 37, 27, 128
    feats, gout, perm, out_w = _inputs(b, f, d, True, seed=7)
    bottom, packed = _pack(feats, perm, sm)
    permc, goutc = perm.cuda(), gout.cuda()

    def run():
        pk, bt = packed.clone().requires_grad_(True), bottom.clone().requires_grad_(True)
        out = mod.dot_interact_packed(pk, bt, permc, pad_to=out_w, sample_major=sm)
        out.backward(goutc)
        return out.detach(), bt.grad, pk.grad

    want = ext.dot_interact_f32_fwd_packed(bottom, packed, permc, out_w, sm)
    wgb, wgp = ext.dot_interact_f32_bwd_packed(goutc, bottom, packed, permc, sm)
    for got, exp in zip(run(), (want, wgb, wgp)):
        assert torch.equal(got.view(torch.int32), exp.view(torch.int32))

    def boom(*a, **k):
        raise AssertionError("f32 kernels called under DE_DI_F32=0")

    monkeypatch.setenv("DE_DI_F32", "0")
    monkeypatch.setattr(mod._DotInteractF32Packed, "apply", boom)
    out, gb, gp = run()
    _check(out.cpu(), _unpack(gb, gp, perm, sm), feats, gout, out_w)


@gpu
@requires_gpu
@pytest.mark.parametrize("f,d", [(40, 128), (27, 20)])
def test_fp32_fallback_shapes_stay_on_torch(f, d, monkeypatch):
    from distributed_embeddings_amd.ops import dot_interact as mod

    def boom(*a, **k):
        raise AssertionError("f32 kernels called outside their shape range")

    monkeypatch.setattr(mod._DotInteractF32, "apply", boom)
    feats, gout, _, out_w = _inputs(9, f, d, False, seed=3)
    fc = feats.cuda().requires_grad_(True)
    out = mod.dot_interact(list(fc.unbind(1)[1:]), fc[:, 0], pad_to=out_w)
    out.backward(gout.cuda())
    _check(out.detach().cpu(), fc.grad.cpu(), feats, gout, out_w)


@gpu
@requires_gpu
def test_bf16_route_unchanged():
    from distributed_embeddings_amd.ops import _backend
    from distributed_embeddings_amd.ops.dot_interact import dot_interact
    feats, _, _, out_w = _inputs(9, 27, 128, True, seed=5, dtype=torch.bfloat16)
    fc = feats.cuda()
    got = dot_interact(list(fc.unbind(1)[1:]), fc[:, 0], pad_to=out_w)
    want = _backend.ops().dot_interact_fwd(fc, out_w)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@gpu
@requires_gpu
def test_dlrm_fp32_reaches_f32_kernels(monkeypatch):
    """fp32 DLRM without autocast, forward + backward: the logits with the f32
    kernels and with DE_DI_F32=0 agree to 1e-4 * max|logit|."""
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    calls = []
    fwd = ext.dot_interact_f32_fwd_packed
    monkeypatch.setattr(ext, "dot_interact_f32_fwd_packed",
                        lambda *a: calls.append(a[1].shape) or fwd(*a))
    torch.manual_seed(0)
    sizes = [500, 600, 700, 400]
    with torch.device("cuda"):
        m = DLRM(sizes, embedding_dim=128, bottom_mlp_dims=(64, 128),
                 top_mlp_dims=(64, 1), num_numerical=4, strategy="basic")
    num = torch.rand(64, 4, device="cuda")
    cats = [torch.randint(0, s, (64,), device="cuda") for s in sizes]
    logits = m(num, cats)
    logits.float().square().sum().backward()
    assert len(calls) == 1 and calls[0][-1] == 128
    assert all(torch.isfinite(p.grad).all() for p in m.top_mlp.parameters())
    monkeypatch.setenv("DE_DI_F32", "0")
    ref = m(num, cats)
    assert len(calls) == 1
    err = float((logits - ref).abs().max())
    print("logit err", err, "max", float(ref.abs().max()))
    assert err <= 1e-4 * float(ref.abs().max())
