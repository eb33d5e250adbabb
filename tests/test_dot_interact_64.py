"""Interaction kernels for 33 <= F <= 64 against a float64 reference.

Same check as ``test_dot_interact_packed_shapes.py``, same bound: every
output element is one fp32 accumulation of exact bf16 x bf16 products rounded
once to bf16, so against a float64 reference from the same bf16 inputs

    |got - ref| <= 2**-8 * |ref| + 2**-20 * sum|terms|

holds element by element (at most 256 terms forward, at most 64 plus the
bottom gradient backward; both counts occur in that file already).  The
shapes walk the third and fourth 16-row tile rows, an odd output width, every
partial block, both compile-time widths and the run-time-D kernels.  The
other tests pin the dispatch: the raw bindings take F = 40, the public op does
not fall back to torch there, the cap is F = 64, and the backward bindings
check their shapes.
"""

import functools
import os
import subprocess
import sys

import pytest
import torch

gpu = pytest.mark.gpu
requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

REL = 2.0 ** -8
ACC = 2.0 ** -20


def _reference(feats, gout, out_w):
    """float64 forward / backward of bf16 ``feats [B, F, D]``, ``gout [B, out_w]``,
    each with the sum of absolute terms per element."""
    b, f, d = feats.shape
    tri_n = f * (f - 1) // 2
    x = feats.double()
    gram = x @ x.transpose(1, 2)
    gram_abs = x.abs() @ x.abs().transpose(1, 2)
    ii, jj = torch.tril_indices(f, f, offset=-1)
    ref_out = torch.zeros(b, out_w, dtype=torch.float64)
    mag_out = torch.zeros(b, out_w, dtype=torch.float64)
    ref_out[:, :tri_n] = gram[:, ii, jj]
    mag_out[:, :tri_n] = gram_abs[:, ii, jj]
    ref_out[:, tri_n:tri_n + d] = x[:, 0]
    gd = gout.double()
    gs = torch.zeros(b, f, f, dtype=torch.float64)
    gs[:, ii, jj] = gd[:, :tri_n]
    gs = gs + gs.transpose(1, 2)
    ref_gf = gs @ x
    mag_gf = gs.abs() @ x.abs()
    ref_gf[:, 0] += gd[:, tri_n:tri_n + d]
    mag_gf[:, 0] += gd[:, tri_n:tri_n + d].abs()
    return ref_out, mag_out, ref_gf, mag_gf


def _check(name, got, ref, mag, roundings=1):
    """The bound above for ``roundings == 1`` (the kernels).  The torch path's
    backward rounds to bf16 up to four times on the way to an element (the two
    bmm gradients, their sum, the bottom-concat gradient), each time a value no
    larger than sum|terms|: 2**-9 * sum|terms| per rounding."""
    err = (got.double() - ref).abs()
    bound = REL * ref.abs() + ACC * mag
    if roundings > 1:
        bound = roundings * 2.0 ** -9 * mag + ACC * mag
    worst = (err - bound).max().item()
    print(f"{name}: max err {err.max().item():.3e}, max (err - bound) {worst:.3e}, "
          f"elements over {(err > bound).sum().item()} of {err.numel()}")
    assert worst <= 0.0, f"{name}: {(err > bound).sum().item()} elements over the bound"


def _packed_cases():
    cases = []
    for sm in (False, True):
        # F = 33: one live row in the third tile row; F = 34 unpadded: odd
        # out_w = 689; F = 48 / 49: last row of the third, first of the fourth
        # tile row; F = 64: no padded row
        for p, pad_to in ((32, 704), (33, 0), (47, 1280), (48, 1344), (63, 2176)):
            cases.append((9, p, 128, pad_to, sm))
        # partial blocks at 1, 2 and 4 samples per block
        for b in (1, 3, 5):
            cases.append((b, 39, 128, 960, sm))
        # the other compile-time width, and run-time widths
        cases.append((9, 39, 32, 832, sm))
        cases.append((9, 39, 64, 0, sm))
        cases.append((9, 39, 256, 1088, sm))
        cases.append((9, 39, 96, 0, sm))
        # pad_to far above the width
        cases.append((9, 39, 128, 1536, sm))
    return cases


PACKED_CASES = _packed_cases()


def _packed_id(case):
    b, p, d, pad_to, sm = case
    return f"B{b}-P{p}-D{d}-pad{pad_to}-{'sm' if sm else 'fm'}"


def _packed_inputs(case):
    b, p, d, pad_to, sm = case
    f = p + 1
    out_w = max(pad_to, f * (f - 1) // 2 + d)
    g = torch.Generator().manual_seed(1000 * b + 10 * p + d + pad_to + int(sm))
    bottom = torch.randn(b, d, generator=g).bfloat16()
    packed = torch.randn(p, b, d, generator=g).bfloat16()   # [P, B, D], worker order
    gout = torch.randn(b, out_w, generator=g).bfloat16()
    perm = torch.randperm(p, generator=g).to(torch.int32)
    if torch.equal(perm, torch.arange(p, dtype=torch.int32)):
        perm = perm.roll(1)
    return bottom, packed, gout, perm, out_w


def _run_packed_uncached(case, device="cuda", dtype=torch.bfloat16):
    """Inputs, results (CPU copies) and the float64 reference of a packed case."""
    from distributed_embeddings_amd.ops.dot_interact import dot_interact_packed
    b, p, d, pad_to, sm = case
    bottom, packed, gout, perm, out_w = _packed_inputs(case)
    packed_in = packed.transpose(0, 1).contiguous() if sm else packed
    bottom_g = bottom.to(device, dtype).requires_grad_(True)
    packed_g = packed_in.to(device, dtype).requires_grad_(True)
    out = dot_interact_packed(packed_g, bottom_g, perm.to(device), pad_to=pad_to,
                              sample_major=sm)
    out.backward(gout.to(device, dtype))
    if device == "cuda":
        torch.cuda.synchronize()
    gpacked = packed_g.grad.cpu()
    if sm:
        gpacked = gpacked.transpose(0, 1)                   # back to [P, B, D]
    feats = torch.cat([bottom.unsqueeze(1),
                       packed[perm.long()].transpose(0, 1)], dim=1)
    ref_out, mag_out, ref_gf, mag_gf = _reference(feats, gout, out_w)
    return dict(tri_n=(p + 1) * p // 2, out_w=out_w, perm=perm, bottom=bottom,
                out=out.detach().cpu(), gbottom=bottom_g.grad.cpu(),
                gpacked=gpacked, ref_out=ref_out, mag_out=mag_out,
                ref_gf=ref_gf, mag_gf=mag_gf)


_run_packed = functools.lru_cache(maxsize=None)(_run_packed_uncached)


def _check_packed_forward(case, r):
    d, tri_n = case[2], r["tri_n"]
    assert r["out"].shape == (case[0], r["out_w"])
    _check("tril", r["out"][:, :tri_n], r["ref_out"][:, :tri_n],
           r["mag_out"][:, :tri_n])
    # the bottom part is a bit copy, the pad exactly zero
    assert torch.equal(r["out"][:, tri_n:tri_n + d], r["bottom"].to(r["out"].dtype))
    assert torch.equal(r["out"][:, tri_n + d:],
                       torch.zeros_like(r["out"][:, tri_n + d:]))


def _check_packed_backward(case, r, roundings=1):
    p = case[1]
    _check("gbottom", r["gbottom"], r["ref_gf"][:, 0], r["mag_gf"][:, 0], roundings)
    # feature f's gradient lands in packed row perm[f-1]
    perm = r["perm"].long()
    assert not torch.equal(perm, torch.arange(p))
    ref = torch.empty(p, case[0], case[2], dtype=torch.float64)
    mag = torch.empty_like(ref)
    ref[perm] = r["ref_gf"][:, 1:].transpose(0, 1)
    mag[perm] = r["mag_gf"][:, 1:].transpose(0, 1)
    _check("gpacked", r["gpacked"], ref, mag, roundings)


# --------------------------------------------------------------------------
# 1. packed shapes
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("case", PACKED_CASES, ids=_packed_id)
def test_packed_forward(case):
    _check_packed_forward(case, _run_packed(case))


@gpu
@requires_gpu
@pytest.mark.parametrize("case", PACKED_CASES, ids=_packed_id)
def test_packed_backward(case):
    _check_packed_backward(case, _run_packed(case))


# --------------------------------------------------------------------------
# 2. stacked layout
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _run_stacked(f, d, device="cuda"):
    from distributed_embeddings_amd.ops.dot_interact import dot_interact
    b = 5
    tri_n = f * (f - 1) // 2
    pad_to = ((tri_n + d + 63) // 64) * 64
    g = torch.Generator().manual_seed(100 * f + d)
    feats = torch.randn(b, f, d, generator=g).bfloat16()
    gout = torch.randn(b, pad_to, generator=g).bfloat16()
    leaves = [feats[:, i].contiguous().to(device).requires_grad_(True)
              for i in range(f)]
    out = dot_interact(leaves[1:], leaves[0], pad_to=pad_to)
    out.backward(gout.to(device))
    gfeats = torch.stack([x.grad.cpu() for x in leaves], dim=1)
    return feats, out.detach().cpu(), gfeats, _reference(feats, gout, pad_to)


@gpu
@requires_gpu
@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("f", (33, 48, 64))
def test_stacked(f, d):
    feats, out, gfeats, (ref_out, mag_out, ref_gf, mag_gf) = _run_stacked(f, d)
    tri_n = f * (f - 1) // 2
    _check("tril", out[:, :tri_n], ref_out[:, :tri_n], mag_out[:, :tri_n])
    assert torch.equal(out[:, tri_n:tri_n + d], feats[:, 0])
    assert torch.equal(out[:, tri_n + d:], torch.zeros_like(out[:, tri_n + d:]))
    _check("gfeats", gfeats, ref_gf, mag_gf)


# --------------------------------------------------------------------------
# 3. the kernels are what runs
# --------------------------------------------------------------------------

def _raw_inputs(f, d, b=4, extra=0):
    tri_n = f * (f - 1) // 2
    out_w = tri_n + d + extra
    g = torch.Generator().manual_seed(7 * f + d)
    feats = torch.randn(b, f, d, generator=g).bfloat16()
    gout = torch.randn(b, out_w, generator=g).bfloat16()
    return feats, gout, out_w


@gpu
@requires_gpu
def test_raw_bindings_take_f40():
    from distributed_embeddings_amd.ops import _backend
    ops = _backend.ops()
    f, d = 40, 128
    feats, gout, out_w = _raw_inputs(f, d, extra=12)
    tri_n = f * (f - 1) // 2
    ref_out, mag_out, ref_gf, mag_gf = _reference(feats, gout, out_w)
    perm = torch.arange(f - 1, dtype=torch.int32).roll(3)
    packed = torch.empty(f - 1, feats.shape[0], d, dtype=torch.bfloat16)
    packed[perm.long()] = feats[:, 1:].transpose(0, 1)
    bottom = feats[:, 0].contiguous()

    out = ops.dot_interact_fwd_packed(bottom.cuda(), packed.cuda(), perm.cuda(),
                                      out_w, False).cpu()
    _check("packed tril", out[:, :tri_n], ref_out[:, :tri_n], mag_out[:, :tri_n])
    gb, gp = ops.dot_interact_bwd_packed(gout.cuda(), bottom.cuda(),
                                         packed.cuda(), perm.cuda(), False)
    _check("packed gbottom", gb.cpu(), ref_gf[:, 0], mag_gf[:, 0])
    _check("packed gpacked", gp.cpu()[perm.long()].transpose(0, 1),
           ref_gf[:, 1:], mag_gf[:, 1:])

    out = ops.dot_interact_fwd(feats.cuda(), out_w).cpu()
    _check("stacked tril", out[:, :tri_n], ref_out[:, :tri_n], mag_out[:, :tri_n])
    gf = ops.dot_interact_bwd(gout.cuda(), feats.cuda()).cpu()
    _check("stacked gfeats", gf, ref_gf, mag_gf)


@gpu
@requires_gpu
def test_public_op_f40_does_not_fall_back(monkeypatch):
    from distributed_embeddings_amd.ops import dot_interact as mod

    def boom(*a, **k):
        raise AssertionError("torch fallback taken at F = 40")
    monkeypatch.setattr(mod, "_torch_dot_interact", boom)
    case = (6, 39, 128, 960, True)
    r = _run_packed_uncached(case)
    _check_packed_forward(case, r)
    _check_packed_backward(case, r)


@gpu
@requires_gpu
def test_dlrm_40_tables_takes_packed_kernels(monkeypatch):
    """A 40-table DLRM at world 1 goes through forward_packed and the kernel."""
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.ops import dot_interact as mod
    from distributed_embeddings_amd.models import dlrm as dlrm_mod

    def boom(*a, **k):
        raise AssertionError("torch fallback taken by the 40-table DLRM")
    monkeypatch.setattr(mod, "_torch_dot_interact", boom)
    calls = []
    real = dlrm_mod.dot_interact_packed

    def spy(packed, *a, **k):
        calls.append(tuple(packed.shape))
        return real(packed, *a, **k)
    monkeypatch.setattr(dlrm_mod, "dot_interact_packed", spy)

    torch.manual_seed(0)
    sizes = [50 + 3 * i for i in range(40)]
    model = DLRM(sizes, embedding_dim=64, num_numerical=13,
                 bottom_mlp_dims=[64, 64], top_mlp_dims=[64, 1]).cuda()
    b = 16
    num = torch.rand(b, 13, device="cuda")
    cats = [torch.randint(0, s, (b,), device="cuda") for s in sizes]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(num, cats)
    logits.float().sum().backward()
    torch.cuda.synchronize()
    assert len(calls) == 1 and sorted(calls[0]) == [16, 40, 64], calls
    assert torch.isfinite(logits).all()


# --------------------------------------------------------------------------
# 4. the cap
# --------------------------------------------------------------------------

@gpu
@requires_gpu
def test_f65_takes_torch_path_and_bindings_refuse():
    from distributed_embeddings_amd.ops import _backend
    ops = _backend.ops()
    case = (3, 64, 128, 0, False)
    r = _run_packed_uncached(case)
    # the torch path rounds the bf16 Gram matrix once, like the kernels; its
    # backward rounds more often (see _check)
    _check_packed_forward(case, r)
    _check_packed_backward(case, r, roundings=4)

    bottom, packed, gout, perm, out_w = _packed_inputs(case)
    feats = torch.cat([bottom.unsqueeze(1), packed.transpose(0, 1)], 1).contiguous()
    with pytest.raises(RuntimeError):
        ops.dot_interact_fwd_packed(bottom.cuda(), packed.cuda(), perm.cuda(),
                                    out_w, False)
    with pytest.raises(RuntimeError):
        ops.dot_interact_fwd(feats.cuda(), out_w)
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd_packed(gout.cuda(), bottom.cuda(), packed.cuda(),
                                    perm.cuda(), False)
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd(gout.cuda(), feats.cuda())
    # F > 32 needs D <= 256
    wide = torch.zeros(2, 40, 288, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.dot_interact_fwd(wide, 40 * 39 // 2 + 288)
    torch.cuda.synchronize()


@gpu
@requires_gpu
@pytest.mark.parametrize("f", (20, 40))
def test_backward_bindings_check_shapes(f):
    from distributed_embeddings_amd.ops import _backend
    ops = _backend.ops()
    b = 3
    tri_n = f * (f - 1) // 2
    perm = torch.arange(f - 1, dtype=torch.int32, device="cuda")

    def z(*shape):
        return torch.zeros(*shape, dtype=torch.bfloat16, device="cuda")
    # D % 32 != 0
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd(z(b, tri_n + 48), z(b, f, 48))
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd_packed(z(b, tri_n + 48), z(b, 48), z(f - 1, b, 48),
                                    perm, False)
    # gout narrower than tril + bottom, or with another batch
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd(z(b, tri_n + 63), z(b, f, 64))
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd_packed(z(b, tri_n + 63), z(b, 64), z(f - 1, b, 64),
                                    perm, False)
    with pytest.raises(RuntimeError):
        ops.dot_interact_bwd(z(b + 1, tri_n + 64), z(b, f, 64))
    # the exact width passes
    ops.dot_interact_bwd(z(b, tri_n + 64), z(b, f, 64))
    ops.dot_interact_bwd_packed(z(b, tri_n + 64), z(b, 64), z(f - 1, b, 64),
                                perm, False)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# 5. repeatability, 6. hipGraph
# --------------------------------------------------------------------------

@gpu
@requires_gpu
def test_bitwise_repeatable():
    case = (9, 63, 128, 2176, False)
    first = _run_packed_uncached(case)
    second = _run_packed_uncached(case)
    for k in ("out", "gbottom", "gpacked"):
        assert torch.equal(first[k].view(torch.int16), second[k].view(torch.int16)), k


@gpu
@requires_gpu
def test_graph_capture_replay():
    from distributed_embeddings_amd.ops import _backend
    ops = _backend.ops()
    b, p, d = 8, 39, 128
    out_w = 960
    g = torch.Generator().manual_seed(5)
    perm = torch.randperm(p, generator=g).to(torch.int32).cuda()

    def draw():
        return (torch.randn(b, d, generator=g).bfloat16().cuda(),
                torch.randn(p, b, d, generator=g).bfloat16().cuda(),
                torch.randn(b, out_w, generator=g).bfloat16().cuda())

    def step(bottom, packed, gout):
        out = ops.dot_interact_fwd_packed(bottom, packed, perm, out_w, False)
        gb, gp = ops.dot_interact_bwd_packed(gout, bottom, packed, perm, False)
        return out, gb, gp

    static = draw()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_res = step(*static)
    for _ in range(2):
        fresh = draw()
        for s, n in zip(static, fresh):
            s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        eager = step(*fresh)
        torch.cuda.synchronize()
        for name, a, e in zip(("out", "gbottom", "gpacked"), static_res, eager):
            assert torch.equal(a.view(torch.int16), e.view(torch.int16)), name


# --------------------------------------------------------------------------
# 7. samples-per-block override
# --------------------------------------------------------------------------

_CHILD = """
import importlib.util, sys, torch
sys.path.insert(0, sys.argv[2])
spec = importlib.util.spec_from_file_location("di64_cases", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
# D = 128 admits 1 and 2 samples per block, D = 64 also 4: partial blocks
for case in ((5, 63, 256, 2304, False), (5, 39, 128, 960, False),
             (5, 39, 64, 0, True)):
    r = mod._run_packed_uncached(case)
    mod._check_packed_forward(case, r)
    mod._check_packed_backward(case, r)
print("child ok")
"""


@gpu
@requires_gpu
@pytest.mark.parametrize("wpb", (2, 4, 8))
def test_samples_per_block_override(wpb):
    """F = 64, D = 256 admits one sample per block only (33 / 40 KB each): a
    launch that took DE_DI_WPB literally would ask for more LDS than a launch
    gets and fail; the child checks the results against the reference, and
    those of two narrower shapes that do run 2 and 4 samples per block."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, DE_DI_WPB=str(wpb))
    res = subprocess.run([sys.executable, "-c", _CHILD, os.path.abspath(__file__), root],
                         env=env, capture_output=True, text=True, timeout=120)
    print(res.stdout[-2000:], res.stderr[-2000:])
    assert res.returncode == 0 and "child ok" in res.stdout


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------

def test_gate_truth_table():
    from distributed_embeddings_amd.ops.dot_interact import kernel_shape_ok
    for f in (1, 2, 27, 32):
        for d in (32, 64, 128, 256, 288, 512):
            assert kernel_shape_ok(f, d), (f, d)      # as before: any D % 32 == 0
        for d in (16, 48, 100, 130):
            assert not kernel_shape_ok(f, d), (f, d)
    for f in (33, 40, 48, 49, 64):
        for d in (32, 64, 96, 128, 224, 256):
            assert kernel_shape_ok(f, d), (f, d)
        for d in (288, 512, 48, 100):
            assert not kernel_shape_ok(f, d), (f, d)
    for f in (65, 100):
        for d in (32, 128, 256):
            assert not kernel_shape_ok(f, d), (f, d)


@pytest.mark.parametrize("sm", (False, True), ids=("fm", "sm"))
def test_public_op_f40_cpu(sm):
    # the bf16 values held in fp32 CPU tensors take the torch path, which then
    # sums the exact products in fp32 and never rounds to bf16: same bound
    case = (4, 39, 64, 896, sm)
    r = _run_packed_uncached(case, device="cpu", dtype=torch.float32)
    _check_packed_forward(case, r)
    _check_packed_backward(case, r)
