"""Packed interaction kernels against a float64 reference, element by element.

Every output element of ``dot_interact_fwd_packed`` / ``dot_interact_bwd_packed``
is one fp32 accumulation of exact bf16 x bf16 products rounded once to bf16,
so against a float64 reference computed from the same bf16 inputs

    |got - ref| <= 2**-8 * |ref| + 2**-20 * sum|terms|

must hold for every element: half a bf16 ulp for the rounding, plus generous
room for an fp32 sum of at most 128 terms.  ``sum|terms|`` is the sum of the
absolute products of that element.  A mis-mapped MFMA fragment, a row written
to the wrong ``perm`` slot or a column off by one misses this by orders of
magnitude; the shapes walk every partial block, the 16-row tile boundary, an
output row stride that is not 16-B aligned, all compile-time widths and one
run-time width.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

REL = 2.0 ** -8
ACC = 2.0 ** -20


def _cases():
    cases = []
    for sm in (False, True):
        # partial blocks at every waves-per-block setting (2, 4, 8)
        for b in (1, 7, 9, 17):
            cases.append((b, 26, 128, 512, sm))
        # F = 2, 3; 16 and 17 straddle the 16-row tile; 32 has no padded row
        for p, pad_to in ((1, 512), (2, 0), (15, 512), (16, 512), (31, 0)):
            cases.append((9, p, 128, pad_to, sm))
        # out_w = 351 + 128 = 479: rows of out / gout are 2-byte aligned only
        cases.append((17, 26, 128, 0, sm))
        # several blocks and a ragged tail at 8 waves per block
        cases.append((8 * 4 + 3, 26, 128, 512, sm))
        # the other compile-time widths, and 96 for the run-time-D kernels
        cases.append((9, 26, 32, 512, sm))
        cases.append((9, 26, 64, 0, sm))
        cases.append((9, 26, 256, 0, sm))
        cases.append((9, 26, 96, 512, sm))
    return cases


CASES = _cases()


def _id(case):
    b, p, d, pad_to, sm = case
    return f"B{b}-P{p}-D{d}-pad{pad_to}-{'sm' if sm else 'fm'}"


@functools.lru_cache(maxsize=None)
def _run(case):
    """Inputs, kernel results (CPU copies) and the float64 reference of a case."""
    from distributed_embeddings_amd.ops.dot_interact import dot_interact_packed
    b, p, d, pad_to, sm = case
    f = p + 1
    tri_n = f * (f - 1) // 2
    out_w = max(pad_to, tri_n + d)
    g = torch.Generator().manual_seed(1000 * b + 10 * p + d + pad_to + int(sm))
    bottom = torch.randn(b, d, generator=g).bfloat16()
    packed = torch.randn(p, b, d, generator=g).bfloat16()   # [P, B, D], worker order
    gout = torch.randn(b, out_w, generator=g).bfloat16()
    perm = torch.randperm(p, generator=g).to(torch.int32)
    if p >= 2 and torch.equal(perm, torch.arange(p, dtype=torch.int32)):
        perm = perm.roll(1)

    packed_in = packed.transpose(0, 1).contiguous() if sm else packed
    bottom_g = bottom.cuda().requires_grad_(True)
    packed_g = packed_in.cuda().requires_grad_(True)
    out = dot_interact_packed(packed_g, bottom_g, perm.cuda(), pad_to=pad_to,
                              sample_major=sm)
    out.backward(gout.cuda())
    torch.cuda.synchronize()
    gpacked = packed_g.grad.cpu()
    if sm:
        gpacked = gpacked.transpose(0, 1)                   # back to [P, B, D]

    # float64 reference from the same bf16 values
    feats = torch.cat([bottom.double().unsqueeze(1),
                       packed.double()[perm.long()].transpose(0, 1)], dim=1)
    gram = feats @ feats.transpose(1, 2)
    gram_abs = feats.abs() @ feats.abs().transpose(1, 2)
    ii, jj = torch.tril_indices(f, f, offset=-1)
    ref_out = torch.zeros(b, out_w, dtype=torch.float64)
    mag_out = torch.zeros(b, out_w, dtype=torch.float64)
    ref_out[:, :tri_n] = gram[:, ii, jj]
    mag_out[:, :tri_n] = gram_abs[:, ii, jj]
    ref_out[:, tri_n:tri_n + d] = bottom.double()

    gd = gout.double()
    gs = torch.zeros(b, f, f, dtype=torch.float64)
    gs[:, ii, jj] = gd[:, :tri_n]
    gs = gs + gs.transpose(1, 2)
    ref_gf = gs @ feats
    mag_gf = gs.abs() @ feats.abs()
    ref_gf[:, 0] += gd[:, tri_n:tri_n + d]
    mag_gf[:, 0] += gd[:, tri_n:tri_n + d].abs()
    return dict(tri_n=tri_n, out_w=out_w, perm=perm, bottom=bottom,
                out=out.detach().cpu(), gbottom=bottom_g.grad.cpu(),
                gpacked=gpacked, ref_out=ref_out, mag_out=mag_out,
                ref_gf=ref_gf, mag_gf=mag_gf)


def _check(name, got, ref, mag):
    err = (got.double() - ref).abs()
    bound = REL * ref.abs() + ACC * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, max (err - bound) {worst:.3e}, "
          f"elements over {(err > bound).sum().item()} of {err.numel()}")
    assert worst <= 0.0, f"{name}: {(err > bound).sum().item()} elements over the bound"


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_forward(case):
    r = _run(case)
    d, tri_n = case[2], r["tri_n"]
    assert r["out"].shape == (case[0], r["out_w"])
    _check("tril", r["out"][:, :tri_n], r["ref_out"][:, :tri_n],
           r["mag_out"][:, :tri_n])
    # the bottom part is a bit copy, the pad exactly zero
    assert torch.equal(r["out"][:, tri_n:tri_n + d], r["bottom"])
    assert torch.equal(r["out"][:, tri_n + d:],
                       torch.zeros_like(r["out"][:, tri_n + d:]))


@requires_gpu
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_packed_backward(case):
    r = _run(case)
    p = case[1]
    _check("gbottom", r["gbottom"], r["ref_gf"][:, 0], r["mag_gf"][:, 0])
    # feature f's gradient lands in packed row perm[f-1]
    perm = r["perm"].long()
    if p >= 2:
        assert not torch.equal(perm, torch.arange(p))
    ref = torch.empty(p, case[0], case[2], dtype=torch.float64)
    mag = torch.empty_like(ref)
    ref[perm] = r["ref_gf"][:, 1:].transpose(0, 1)
    mag[perm] = r["mag_gf"][:, 1:].transpose(0, 1)
    _check("gpacked", r["gpacked"], ref, mag)
