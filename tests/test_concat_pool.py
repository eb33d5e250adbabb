"""Fused concat + average pool (ops/concat_pool.py, csrc/concat_pool.hip).

The reference is the formula written out in float64, every window sliced
with its true length (not ``avg_pool1d``).  Bounds, with the project's usual
factor 2 over the fp32 roundoff 2^-24:

* pooled columns: a window of S terms summed in fp32, one division, one
  rounding: ``|y - y*| <= 2^-8 |y*| + S 2^-23 sum|x| / cnt`` for bf16 out,
  ``(S + 1) 2^-23 sum|x| / cnt`` for fp32 out;
* input gradients: one division, one rounding: ``2^-8 |g / cnt|`` for bf16,
  ``2^-23 |g / cnt|`` for fp32;
* numerical columns and their gradient: bit-equal to ``.to(dtype)``;
* ``stride == 1``: bit-equal to ``torch.cat``; two calls: bit-equal.
"""

import pytest
import torch

from distributed_embeddings_amd.ops import concat_pool
from distributed_embeddings_amd.ops.concat_pool import concat_avg_pool

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

ROWS = 32   # samples per block tile (CP_ROWS)
# A block's span is min(64, 1024 bytes / S) output columns, a multiple of 8
# when above 8: at most 512 (bf16) or 256 (fp32) concatenated columns.
WIDTHS = {
    # 1128 (+ 4) columns, more than two spans at every stride; windows of 7,
    # 30 and 75 straddle the inputs and leave a partial last window
    "wide": [8, 16, 128, 32, 64, 8, 8, 128, 64, 16, 8, 128, 128, 64, 32, 8,
             64, 128, 16, 32, 8, 16, 8, 16],
    "narrow": [8, 16, 8],       # 32 columns: below one span
}
# 75: a span of 6 (bf16) or 3 (fp32) windows is 450 or 225 columns, so a
# 16-byte chunk straddles the span edges; spans of 8k windows are aligned
STRIDES = [1, 2, 7, 8, 30, 75]


def reference(inputs, numerical, stride):
    """(out, sum|x|/cnt per pooled column, cnt per pooled column), float64."""
    x = torch.cat([t.double() for t in inputs], dim=1)
    wins = [x[:, c:c + stride] for c in range(0, x.shape[1], stride)]
    pooled = torch.stack([w.sum(1) / w.shape[1] for w in wins], dim=1)
    mag = torch.stack([w.abs().sum(1) / w.shape[1] for w in wins], dim=1)
    cnt = torch.tensor([w.shape[1] for w in wins], dtype=torch.float64,
                       device=x.device)
    if numerical is not None:
        pooled = torch.cat([pooled, numerical.double()], dim=1)
    return pooled, mag, cnt


def make_inputs(widths, b, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(b, w, generator=g).to(dtype).to(device)
            .requires_grad_() for w in widths]


def check_against_reference(inputs, numerical, stride, out_dtype):
    out = concat_avg_pool(inputs, numerical, stride, out_dtype=out_dtype)
    want, mag, cnt = reference(inputs, numerical, stride)
    wp = mag.shape[1]
    assert out.dtype == out_dtype and out.shape == want.shape
    if out_dtype == torch.bfloat16:
        bound = 2.0 ** -8 * want[:, :wp].abs() + stride * 2.0 ** -23 * mag
    else:
        bound = (stride + 1) * 2.0 ** -23 * mag
    err = (out[:, :wp].double() - want[:, :wp]).abs()
    assert bool((err <= bound).all()), (err - bound).max()
    if numerical is not None:
        assert torch.equal(out[:, wp:], numerical.detach().to(out_dtype))
    if stride == 1 and out_dtype == inputs[0].dtype:
        assert torch.equal(out[:, :wp], torch.cat(inputs, dim=1))
    assert torch.equal(out, concat_avg_pool(inputs, numerical, stride,
                                            out_dtype=out_dtype))

    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)
                       ).to(out_dtype).to(out.device)
    leaves = inputs + ([numerical] if numerical is not None
                       and numerical.requires_grad else [])
    grads = torch.autograd.grad(out, leaves, gout)
    eps = 2.0 ** -8 if inputs[0].dtype == torch.bfloat16 else 2.0 ** -23
    begin = 0
    for t, gin in zip(inputs, grads):
        col = torch.arange(begin, begin + t.shape[1], device=out.device) // stride
        exp = gout.double()[:, col] / cnt[col]
        assert gin.dtype == t.dtype and gin.is_contiguous()
        err = (gin.double() - exp).abs()
        assert bool((err <= eps * exp.abs()).all()), (begin, err.max())
        begin += t.shape[1]
    if len(leaves) > len(inputs):
        assert torch.equal(grads[-1], gout[:, wp:].to(numerical.dtype))
    return grads


# ---------------------------------------------------------------------------
# CPU: the fallback
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("stride", [1, 4, 7])
def test_cpu_matches_formula_and_composition(stride):
    g = torch.Generator().manual_seed(stride)
    inputs = [torch.randn(5, w, generator=g, dtype=torch.float64)
              for w in (3, 8, 11)]                 # 22 columns
    num = torch.randn(5, 3, generator=g, dtype=torch.float64)
    want, _, _ = reference(inputs, num, stride)
    got = concat_avg_pool(inputs, num, stride)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-14)
    row = torch.arange(1, 12, dtype=torch.float64).reshape(1, 11)
    assert concat_avg_pool([row], None, 4).tolist() == [[2.5, 6.5, 10.0]]

    f32 = [t.float() for t in inputs]
    x = torch.cat(f32, dim=1)
    x = torch.nn.functional.avg_pool1d(x.unsqueeze(1), stride, stride=stride,
                                       ceil_mode=True).squeeze(1)
    assert torch.equal(concat_avg_pool(f32, num.float(), stride),
                       torch.cat([x, num.float()], dim=1))


# ---------------------------------------------------------------------------
# GPU: the kernels
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("shape", sorted(WIDTHS))
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_kernels_match_reference(dtype, stride, shape):
    widths = list(WIDTHS[shape])
    if dtype == torch.float32:
        widths.insert(3, 4)      # 1132 or 36 columns: a partial window at 8
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    for b in (1, ROWS + 1, 2 * ROWS + 6):
        inputs = make_inputs(widths, b, dtype, "cuda", seed=b)
        assert concat_pool.fused_ok(inputs, None, stride)
        check_against_reference(inputs, None, stride, dtype)
        # odd row widths: the output rows are not 16-byte aligned
        num3 = torch.randn(b, 3, device="cuda", requires_grad=True)
        check_against_reference(inputs, num3, stride, dtype)
        num13 = torch.randn(b, 13, device="cuda").to(other)
        check_against_reference(inputs, num13, stride, other)


@pytest.mark.gpu
@requires_gpu
def test_more_inputs_than_one_launch():
    """284 inputs against 224 descriptors per launch: spans of 448 columns at
    stride 7, so the first launch ends at column 1792, inside the 32-wide
    input that begins at 1784 and goes into both launches."""
    inputs = make_inputs([8] * 223 + [32] + [8] * 60, 5, torch.bfloat16, "cuda")
    num = torch.randn(5, 3, device="cuda")
    check_against_reference(inputs, num, 7, torch.bfloat16)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", ["noncontiguous", "w12"])
def test_guard_takes_the_composition(case):
    inputs = make_inputs([16, 8, 32], 9, torch.bfloat16, "cuda")
    if case == "noncontiguous":
        inputs[1] = make_inputs([16], 9, torch.bfloat16, "cuda")[0][:, ::2]
    else:
        inputs[1] = make_inputs([12], 9, torch.bfloat16, "cuda")[0]
    num = torch.randn(9, 3, device="cuda")
    assert not concat_pool.fused_ok(inputs, num, 7)
    x = torch.cat(inputs, dim=1)
    x = torch.nn.functional.avg_pool1d(x.unsqueeze(1), 7, stride=7,
                                       ceil_mode=True).squeeze(1)
    got = concat_avg_pool(inputs, num, 7)
    assert got.dtype == torch.bfloat16        # the kernels' dtype, unpromoted
    assert torch.equal(got, torch.cat([x, num.bfloat16()], dim=1))


@pytest.mark.gpu
@requires_gpu
def test_capture_replays_on_new_contents():
    widths, b, stride = WIDTHS["wide"], ROWS + 1, 7
    static = make_inputs(widths, b, torch.bfloat16, "cuda", seed=1)
    num = torch.randn(b, 3, device="cuda")
    gout = torch.randn(b, -(-sum(widths) // stride) + 3, device="cuda"
                       ).bfloat16()

    def run():
        out = concat_avg_pool(static, num, stride)
        return out, torch.autograd.grad(out, static, gout)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                        # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = run()
    for seed in (2, 3):
        with torch.no_grad():
            for t, new in zip(static, make_inputs(widths, b, torch.bfloat16,
                                                  "cuda", seed=seed)):
                t.copy_(new)
            num.copy_(torch.randn(b, 3, device="cuda"))
            gout.copy_(torch.randn(gout.shape, device="cuda"))
        graph.replay()
        want_out, want_grads = run()
        assert torch.equal(out, want_out)
        for got, want in zip(grads, want_grads):
            assert torch.equal(got, want)


@pytest.mark.gpu
@requires_gpu
def test_model_route_on_equals_off(monkeypatch):
    """SyntheticModel under bf16 autocast, kernels against the composition.

    Both routes sum a window in fp32 and round the mean to bf16 once, so a
    pooled column differs by one bf16 rounding at most, 2^-8 relative.  To
    first order that and the bf16 rounding of each of the three Linear
    outputs add up to 4 * 2^-8 = 2^-6 of the magnitude of the terms summed;
    the backward through the same layers doubles it for the weight gradient.
    ``allclose`` with rtol = atol/max|ref| = 2^-6 (logits) and 2^-5 (gradient).
    """
    from distributed_embeddings_amd.models.config import EmbeddingConfig, ModelConfig
    from distributed_embeddings_amd.models.synthetic import (SyntheticModel,
                                                             expand_tables)
    from distributed_embeddings_amd.utils.input_gen import make_batch
    cfg = ModelConfig(
        name="unit",
        embedding_configs=[EmbeddingConfig(2, [1, 3], 50, 8, True),
                           EmbeddingConfig(3, [1], 80, 16, False)],
        mlp_sizes=[16, 8], num_numerical_features=4, interact_stride=7)
    torch.manual_seed(11)
    with torch.device("cuda"):
        model = SyntheticModel(cfg)
    tables, input_map, hotness = expand_tables(cfg)
    gi = torch.Generator().manual_seed(13)
    cats = [c.cuda() for c in make_batch([tables[t][0] for t in input_map],
                                         hotness, 40, generator=gi,
                                         keep_hot_dim=True)]
    num = torch.rand(40, 4, generator=gi).cuda()

    calls = []
    real = concat_pool._ConcatAvgPool.apply
    monkeypatch.setattr(concat_pool._ConcatAvgPool, "apply",
                        lambda *a: calls.append(1) or real(*a))
    results = []
    for flag in ("1", "0"):
        monkeypatch.setenv("DE_FUSED_POOL", flag)
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            logits = model(num, cats)
        logits.float().sum().backward()
        first = next(m for m in model.mlp.modules()
                     if isinstance(m, torch.nn.Linear))
        results.append((logits.detach().float(), first.weight.grad.float()))
    assert len(calls) == 1
    for (got, want), tol in zip(zip(*results), (2.0 ** -6, 2.0 ** -5)):
        assert torch.allclose(got, want, rtol=tol,
                              atol=tol * float(want.abs().max()))
