"""Narrow interaction kernels (D = 8, 16, 24; F <= 32) against float64.

Every output element is one fp32 accumulation of exact bf16 x bf16 products,
rounded once to bf16 (half an ulp: 2**-8 relative).  An fp32 sum of n terms
is off by at most n * 2**-24 * sum|terms|, so against a float64 reference of
the same bf16 inputs

    forward:   |out - ref| <= 2**-8 * |ref| + D  * 2**-24 * sum_d |x_id * x_jd|
    backward:  |g - ref|   <= 2**-8 * |ref| + 33 * 2**-24 * sum_k |terms|

(32 features plus the bottom-concat gradient).  The bottom block is a bit
copy, the pad exact zeros, and a repeated call gives the same bits.
"""

import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")


def _reference(feats, gout, out_w):
    """float64 forward / backward of bf16 ``feats [B, F, D]``, ``gout [B, out_w]``,
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


def _inputs(b, f, d, padded, seed=0):
    """bf16 feats [B, F, D] in model order, gout, a non-identity perm, out_w."""
    width = f * (f - 1) // 2 + d
    out_w = (width + 63) // 64 * 64 if padded else width
    g = torch.Generator().manual_seed(seed + 1000 * b + 40 * f + d + int(padded))
    feats = torch.randn(b, f, d, generator=g).bfloat16()
    gout = torch.randn(b, out_w, generator=g).bfloat16()
    perm = torch.arange(f - 1, dtype=torch.int32).roll(3 % max(f - 1, 1)).flip(0)
    return feats, gout, perm, out_w


def _run(ext, layout, feats, gout, perm, out_w):
    """(out, gfeats [B, F, D]) of the narrow bindings for one layout, on CPU."""
    if layout == "stacked":
        fc = feats.cuda()
        out = ext.dot_interact_narrow_fwd(fc, out_w)
        return out.cpu(), ext.dot_interact_narrow_bwd(gout.cuda(), fc).cpu()
    sm = layout == "sm"
    b, f, d = feats.shape
    # packed row perm[i] holds model feature i + 1
    rows = torch.empty(b, f - 1, d, dtype=feats.dtype)
    rows[:, perm.long()] = feats[:, 1:]
    packed = (rows if sm else rows.transpose(0, 1)).contiguous().cuda()
    bottom = feats[:, 0].contiguous().cuda()
    out = ext.dot_interact_narrow_fwd_packed(bottom, packed, perm.cuda(), out_w, sm)
    gbottom, gpacked = ext.dot_interact_narrow_bwd_packed(
        gout.cuda(), bottom, packed, perm.cuda(), sm)
    grows = gpacked.cpu() if sm else gpacked.cpu().transpose(0, 1)
    gfeats = torch.cat([gbottom.cpu().unsqueeze(1), grows[:, perm.long()]], 1)
    return out.cpu(), gfeats


@gpu
@requires_gpu
@pytest.mark.parametrize("padded", (False, True), ids=("exact", "pad64"))
@pytest.mark.parametrize("b", (5, 261))
@pytest.mark.parametrize("layout", ("stacked", "fm", "sm"))
@pytest.mark.parametrize("f", (2, 17, 27, 32))
@pytest.mark.parametrize("d", (8, 16, 24))
def test_narrow_against_float64(d, f, layout, b, padded):
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    feats, gout, perm, out_w = _inputs(b, f, d, padded)
    tri_n = f * (f - 1) // 2
    ref, mag, ref_g, mag_g = _reference(feats, gout, out_w)
    out, gfeats = _run(ext, layout, feats, gout, perm, out_w)
    err = (out.double() - ref).abs()[:, :tri_n]
    bound = (2.0 ** -8 * ref.abs() + d * 2.0 ** -24 * mag)[:, :tri_n]
    assert (err <= bound).all()
    assert torch.equal(out[:, tri_n:tri_n + d].view(torch.int16),
                       feats[:, 0].view(torch.int16))
    assert (out[:, tri_n + d:].view(torch.int16) == 0).all()
    err_g = (gfeats.double() - ref_g).abs()
    bound_g = 2.0 ** -8 * ref_g.abs() + 33 * 2.0 ** -24 * mag_g
    assert (err_g <= bound_g).all()
    out2, gfeats2 = _run(ext, layout, feats, gout, perm, out_w)
    assert torch.equal(out.view(torch.int16), out2.view(torch.int16))
    assert torch.equal(gfeats.view(torch.int16), gfeats2.view(torch.int16))


@gpu
@requires_gpu
@pytest.mark.parametrize("sm", (False, True), ids=("fm", "sm"))
def test_public_op_routes_to_narrow(sm, monkeypatch):
    """dot_interact_packed at D = 16, F = 27: the narrow bindings' bits under
    autograd; with DE_DI_NARROW=0 the torch composition, whose forward (one
    fp32-accumulated bmm, rounded once) meets the forward bound too."""
    from distributed_embeddings_amd.ops import _backend
    from distributed_embeddings_amd.ops import dot_interact as mod
    ext = _backend.ops()
    b, f, d = 37, 27, 16
    feats, gout, perm, out_w = _inputs(b, f, d, True, seed=7)
    rows = torch.empty(b, f - 1, d, dtype=feats.dtype)
    rows[:, perm.long()] = feats[:, 1:]
    packed = (rows if sm else rows.transpose(0, 1)).contiguous().cuda()
    bottom, permc, goutc = feats[:, 0].contiguous().cuda(), perm.cuda(), gout.cuda()
    pk, bt = packed.clone().requires_grad_(True), bottom.clone().requires_grad_(True)
    out = mod.dot_interact_packed(pk, bt, permc, pad_to=out_w, sample_major=sm)
    out.backward(goutc)
    want = ext.dot_interact_narrow_fwd_packed(bottom, packed, permc, out_w, sm)
    wgb, wgp = ext.dot_interact_narrow_bwd_packed(goutc, bottom, packed, permc, sm)
    for got, exp in ((out, want), (bt.grad, wgb), (pk.grad, wgp)):
        assert torch.equal(got.view(torch.int16), exp.view(torch.int16))

    def boom(*a, **k):
        raise AssertionError("narrow kernels called under DE_DI_NARROW=0")

    monkeypatch.setenv("DE_DI_NARROW", "0")
    monkeypatch.setattr(mod._DotInteractNarrowPacked, "apply", boom)
    off = mod.dot_interact_packed(packed, bottom, permc, pad_to=out_w,
                                  sample_major=sm).cpu()
    ref, mag, _, _ = _reference(feats, gout, out_w)
    err = (off.double() - ref).abs()
    assert (err <= 2.0 ** -8 * ref.abs() + d * 2.0 ** -24 * mag).all()


@gpu
@requires_gpu
def test_public_op_copies_unaligned_view():
    """A contiguous packed view 2 bytes off a 16-byte boundary gives the bits
    of the aligned tensor instead of failing the bindings' alignment check."""
    from distributed_embeddings_amd.ops.dot_interact import dot_interact_packed
    feats, _, _, out_w = _inputs(5, 4, 16, False)
    bottom, packed = feats[:, 0].contiguous().cuda(), feats[:, 1:].contiguous().cuda()
    perm = torch.arange(3, dtype=torch.int32, device="cuda")
    flat = torch.zeros(packed.numel() + 1, dtype=torch.bfloat16, device="cuda")
    flat[1:] = packed.flatten()
    view = flat[1:].view(5, 3, 16)
    assert view.is_contiguous() and view.data_ptr() % 16 == 2
    got = dot_interact_packed(view, bottom, perm, sample_major=True)
    want = dot_interact_packed(packed, bottom, perm, sample_major=True)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@gpu
@requires_gpu
def test_dlrm_dim16_reaches_packed_narrow(monkeypatch):
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    calls = []
    fwd = ext.dot_interact_narrow_fwd_packed
    monkeypatch.setattr(ext, "dot_interact_narrow_fwd_packed",
                        lambda *a: calls.append(a[1].shape) or fwd(*a))
    torch.manual_seed(0)
    sizes = [50, 20, 70, 33, 40]
    model = DLRM(sizes, embedding_dim=16, bottom_mlp_dims=(32, 16),
                 top_mlp_dims=(32, 1), num_numerical=13).cuda()
    num = torch.rand(24, 13, device="cuda")
    cats = [torch.randint(0, s, (24,), device="cuda") for s in sizes]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = model(num, cats).float().sum()
    loss.backward()
    assert len(calls) == 1 and calls[0][-1] == 16
    assert torch.isfinite(loss).item()
    assert all(torch.isfinite(p.grad).all() for p in model.top_mlp.parameters())


@gpu
@requires_gpu
@pytest.mark.parametrize("f,d,dw,gb,ok", [
    (27, 16, 0, 3, True),     # the exact width passes
    (27, 32, 0, 3, False), (27, 12, 0, 3, False), (33, 16, 0, 3, False),
    (27, 16, -1, 3, False),   # short out_w / gout
    (27, 16, 0, 4, False),    # gout of another batch size (backward only)
])
@pytest.mark.parametrize("packed", (False, True), ids=("stacked", "packed"))
def test_narrow_binding_checks(f, d, dw, gb, ok, packed):
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    z = dict(dtype=torch.bfloat16, device="cuda")
    out_w = f * (f - 1) // 2 + d + dw
    gout = torch.zeros(gb, out_w, **z)
    if packed:
        args = (torch.zeros(3, d, **z), torch.zeros(f - 1, 3, d, **z),
                torch.arange(f - 1, dtype=torch.int32, device="cuda"))
        fwd = lambda: ext.dot_interact_narrow_fwd_packed(*args, out_w, False)
        bwd = lambda: ext.dot_interact_narrow_bwd_packed(gout, *args, False)
    else:
        feats = torch.zeros(3, f, d, **z)
        fwd = lambda: ext.dot_interact_narrow_fwd(feats, out_w)
        bwd = lambda: ext.dot_interact_narrow_bwd(gout, feats)
    if ok:
        assert fwd().shape == (3, out_w)
        bwd()
        return
    if gb == 3:
        with pytest.raises(RuntimeError):
            fwd()
    with pytest.raises(RuntimeError):
        bwd()


def test_narrow_shape_ok_truth_table():
    from distributed_embeddings_amd.ops.dot_interact import (
        kernel_shape_ok, narrow_shape_ok)
    for d in range(0, 70):
        for f in range(0, 40):
            assert narrow_shape_ok(f, d) == (d in (8, 16, 24) and 1 <= f <= 32)
    assert not kernel_shape_ok(27, 16)
