"""Stochastic rounding of the fused optimizers' writes to bf16 tables.

A finite fp32 x with bit pattern u is stored as the bf16 (u + r) >> 16, with
16 bits r = r(seed, step, o) that depend on the element's table offset
o = row * width + col and on nothing else:

    key = mix64(seed ^ mix64(step))
    h   = mix64(key + (o >> 2))
    r   = (h >> (16 * (o & 3))) & 0xFFFF

The Python reference (ops.embedding_lookup) implements this; the HIP kernels
are held to it bit for bit wherever fp32 arithmetic is exact, and to derived
bounds elsewhere.

The exact case: table entries k/64 with |k| <= 128 (bf16-exact), upstream
gradients integers in [-3, 3], per-id weights in {0.5, 1, 2}, combiner sum,
lr = 2**-12.  Every partial sum of the gradient is a multiple of 1/2 below
2**11 and w - lr * G a multiple of 2**-13 below 4 in magnitude: exact in fp32
in any summation order, fused multiply-add or not.  A stochastically rounded
multiple of 2**-13 is one again, so further steps stay exact.
"""

import functools
import math

import pytest
import torch

from conftest import run_distributed
from test_gpu import (_HELPER_ROWS, _HELPER_VOCAB, _HELPER_WIDTHS,
                      _assert_within, _dense_grad_ref, _helper_case,
                      _helper_dense, _terms_atol)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")

_LR = 2.0 ** -12
_M64 = (1 << 64) - 1


def _bits(t):
    """bf16 tensor -> its bit patterns as int64 in [0, 65536)."""
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _table_offsets(vocab, width):
    return torch.arange(vocab * width, dtype=torch.int64).view(vocab, width)


def _sr_table(x32, seed, step):
    """Reference rounding of a whole fp32 [vocab, width] table."""
    from distributed_embeddings_amd.ops.embedding_lookup import (
        _stochastic_round_bf16_ref)
    return _stochastic_round_bf16_ref(x32, seed, step,
                                      _table_offsets(*x32.shape))


# --------------------------------------------------------------------------
# 1. the reference itself (CPU)
# --------------------------------------------------------------------------

def _mix64(k):
    k = (k + 0x9E3779B97F4A7C15) & _M64
    k = ((k ^ (k >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    k = ((k ^ (k >> 27)) * 0x94D049BB133111EB) & _M64
    return k ^ (k >> 31)


def test_reference_bits_match_the_written_definition():
    """The hash, written out a second time on Python ints."""
    from distributed_embeddings_amd.ops.embedding_lookup import (
        stochastic_rounding_bits)
    offsets = torch.tensor([0, 1, 2, 3, 4, 7, 4097, (1 << 33) + 2,
                            (1 << 40) + 3])
    for seed, step in ((0, 0), (12345, 7), (-5, 1 << 40)):
        key = _mix64((seed & _M64) ^ _mix64(step & _M64))
        want = [(_mix64((key + (o >> 2)) & _M64) >> (16 * (o & 3))) & 0xFFFF
                for o in offsets.tolist()]
        got = stochastic_rounding_bits(seed, step, offsets)
        assert got.tolist() == want
    # one hash serves four neighbours: its 16-bit fields differ
    r = stochastic_rounding_bits(3, 0, torch.arange(4))
    assert len(set(r.tolist())) > 1


def _special_values():
    return torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"),
                         1.0, -2.5, 0.0078125, -96.0, 3.3895e38],
                        dtype=torch.float32)


def test_reference_keeps_representable_and_special_values():
    from distributed_embeddings_amd import stochastic_round_bf16
    x = _special_values()
    # +-0, +-inf, the canonical NaN 0x7fc00000, four bf16 values, and the
    # largest finite fp32 values' neighbourhood, which may round to inf
    want = [0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x3F80, 0xC020, 0x3C00,
            0xC2C0]
    for seed, step, base in ((0, 0, 0), (99, 3, 5)):
        got = stochastic_round_bf16(x, seed, step, base)
        assert got.dtype == torch.bfloat16
        assert _bits(got)[:9].tolist() == want
        assert int(_bits(got)[9]) in (0x7F7E, 0x7F7F)
    # a bf16 value of any size never moves
    g = torch.Generator().manual_seed(1)
    y = (torch.randn(4096, generator=g)
         * torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20]).repeat(4096)[:4096])
    y = y.to(torch.bfloat16).float()
    assert _same_bits(stochastic_round_bf16(y, 7, 1, 3), y.to(torch.bfloat16))


def test_reference_picks_a_neighbour_and_is_odd():
    from distributed_embeddings_amd import stochastic_round_bf16
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(6000, generator=g)
         * torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20]).repeat(2000))
    got = _bits(stochastic_round_bf16(x, 11, 4, 9))
    u = x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    down = u >> 16            # towards zero
    assert bool(((got == down) | (got == down + 1)).all())
    assert bool((got == down).any()) and bool((got == down + 1).any())
    # away from zero exactly when r + low16 carries
    from distributed_embeddings_amd.ops.embedding_lookup import (
        stochastic_rounding_bits)
    r = stochastic_rounding_bits(11, 4, torch.arange(6000) + 9)
    assert torch.equal(got - down, ((u & 0xFFFF) + r) >> 16)
    # SR(-x) == -SR(x) for equal bits
    neg = _bits(stochastic_round_bf16(-x, 11, 4, 9))
    assert torch.equal(neg, got ^ 0x8000)


def test_reference_is_unbiased_binomial():
    """x = 1 + 2**-9 has fraction exactly 1/4: over 65536 offsets the count
    rounded up is Binomial(65536, 1/4), sigma = sqrt(65536 / 4 * 3 / 4)."""
    from distributed_embeddings_amd import stochastic_round_bf16
    x = torch.full((65536,), 1.0 + 2.0 ** -9)
    sigma = math.sqrt(65536 * 0.25 * 0.75)
    for seed, step in ((0, 0), (1, 0), (1, 1)):
        got = stochastic_round_bf16(x, seed, step).float()
        assert bool(((got == 1.0) | (got == 1.0 + 2.0 ** -7)).all())
        ups = int((got > 1.0).sum())
        print(f"seed {seed} step {step}: {ups} up, "
              f"{(ups - 16384) / sigma:+.2f} sigma")
        assert abs(ups - 16384) < 6 * sigma


# --------------------------------------------------------------------------
# 2. the op against the reference (GPU)
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
def test_op_matches_reference_bitwise():
    from distributed_embeddings_amd import stochastic_round_bf16
    n = 4099  # no multiple of 4, more than one block
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(n, generator=g)
         * torch.tensor([2.0 ** -20, 1.0, 2.0 ** 20]).repeat(n)[:n])
    special = torch.cat([_special_values(), torch.tensor([1e-40, -1e-40])])
    pos = torch.randperm(n, generator=g)[:3 * special.numel()]
    x[pos] = special.repeat(3)
    for seed, step, base in ((0, 0, 0), (12345, 7, 4097),
                             (-5, 1 << 40, (1 << 33) + 2)):
        want = stochastic_round_bf16(x, seed, step, base)
        got = stochastic_round_bf16(x.cuda(), seed, step, base)
        assert got.is_cuda and got.dtype == torch.bfloat16
        for i in (_bits(got) != _bits(want)).nonzero().flatten().tolist():
            print(f"element {i}: x {int(x[i].view(torch.int32)) & 0xFFFFFFFF:#x} "
                  f"got {int(_bits(got)[i]):#x} want {int(_bits(want)[i]):#x}")
        assert torch.equal(got.cpu().view(torch.int16),
                           want.view(torch.int16)), (seed, step, base)
        assert not _same_bits(want, x.to(torch.bfloat16))


# --------------------------------------------------------------------------
# 3. exact fused SGD over every tiling
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_case(width):
    """(table fp32 [50, width] bf16-exact, upstream grad [37, width],
    per-id weights [nnz])."""
    case = _helper_case()
    g = torch.Generator().manual_seed(1000 + width)
    table = torch.randint(-128, 129, (_HELPER_VOCAB, width),
                          generator=g).float() / 64
    up = torch.randint(-3, 4, (_HELPER_ROWS, width), generator=g).float()
    choice = torch.randint(0, 3, (case["ids_hot"].numel(),), generator=g)
    per_id_w = torch.tensor([0.5, 1.0, 2.0])[choice]
    assert torch.equal(table, table.to(torch.bfloat16).float())
    return table, up, per_id_w


def _exact_dense_grad(up, per_id_w):
    """float64 [vocab, width] summed gradient of the sum combiner."""
    case = _helper_case()
    rows = up.double()[case["row_of"]]
    if per_id_w is not None:
        rows = rows * per_id_w.double().unsqueeze(1)
    dense = torch.zeros(_HELPER_VOCAB, up.shape[1], dtype=torch.float64)
    return dense.index_add_(0, case["ids_hot"], rows)


def _exact_step(w_bf16, grad64):
    """fp32 w - lr * G, after checking that fp32 holds it exactly."""
    new64 = w_bf16.double() - _LR * grad64
    new32 = new64.float()
    assert torch.equal(new32.double(), new64)
    assert float(new64.abs().max()) < 8
    return new32


def _make_sgd_layer(table, device, seed, stochastic_rounding=True):
    from distributed_embeddings_amd import Embedding
    emb = Embedding(table.shape[0], table.shape[1], combiner="sum",
                    dtype=torch.bfloat16).to(device)
    with torch.no_grad():
        emb.weight.copy_(table)
    emb.enable_fused_optimizer("sgd", _LR,
                               stochastic_rounding=stochastic_rounding,
                               seed=seed)
    return emb


def _fused_inputs(dev, up, per_id_w, grad_bf16):
    case = _helper_case()
    return (case["ids_hot"].to(dev), case["splits"].to(dev),
            None if per_id_w is None else per_id_w.to(dev),
            up.to(device=dev,
                  dtype=torch.bfloat16 if grad_bf16 else torch.float32))


def _fused_step(emb, ids, splits, per_id_w, up):
    out = emb.csr_lookup(ids, splits, "sum", up.dtype, per_id_w)
    assert out.dtype == up.dtype
    out.backward(up)


def _check_exact_fused_sgd(device, width, grad_bf16, weighted):
    case = _helper_case()
    table, up, per_id_w = _exact_case(width)
    if not weighted:
        per_id_w = None
    seed, step0 = 424242 + width, 5
    emb = _make_sgd_layer(table, device, seed)
    assert emb._fused_sr.dtype == torch.int64
    assert emb._fused_sr.tolist() == [seed, 0]
    with torch.no_grad():
        emb._fused_sr[1] = step0
    touched = torch.bincount(case["ids_hot"], minlength=_HELPER_VOCAB) > 0
    assert touched.any() and not touched.all()
    grad64 = _exact_dense_grad(up, per_id_w)
    inputs = _fused_inputs(device, up, per_id_w, grad_bf16)
    w = table.to(torch.bfloat16)
    for k in range(2):
        new32 = _exact_step(w, grad64)
        want = _sr_table(new32, seed, step0 + k)
        rne = new32.to(torch.bfloat16)
        # the inputs can tell the two roundings apart
        assert int((_bits(want) != _bits(rne)).sum()) > 0
        _fused_step(emb, *inputs)
        got = emb.weight.detach().cpu()
        assert emb.weight.grad is None
        assert _same_bits(got[~touched], w[~touched]), "untouched rows moved"
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, (f"step {k} w{width} bf16 grad {grad_bf16} weighted "
                          f"{weighted}: {bad} elements differ, "
                          f"{int((_bits(got) != _bits(rne)).sum())} from RNE")
        assert emb._fused_sr.tolist() == [seed, step0 + k + 1]
        w = want


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("grad_bf16", [False, True])
def test_exact_fused_sgd_cpu(grad_bf16, weighted):
    _check_exact_fused_sgd("cpu", 16, grad_bf16, weighted)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("grad_bf16", [False, True])
@pytest.mark.parametrize("width", _HELPER_WIDTHS)
def test_exact_fused_sgd_gpu(width, grad_bf16, weighted):
    """Narrow and wide tilings, one and two column passes, and the 300-long
    segment through scratch + finalize all give an element the same bits."""
    _check_exact_fused_sgd("cuda", width, grad_bf16, weighted)


def test_no_update_does_not_advance_the_counter():
    """An apply without ids launches nothing; the CPU path mirrors that."""
    table = _exact_case(16)[0]
    emb = _make_sgd_layer(table, "cpu", 9)
    empty = torch.zeros(0, dtype=torch.long)
    out = emb.csr_lookup(empty, torch.zeros(4, dtype=torch.long), "sum")
    out.backward(torch.ones(3, 16))
    assert emb._fused_sr.tolist() == [9, 0]
    assert _same_bits(emb.weight, table.to(torch.bfloat16))


@pytest.mark.gpu
@requires_gpu
def test_no_update_does_not_advance_the_counter_gpu():
    table = _exact_case(16)[0]
    emb = _make_sgd_layer(table, "cuda", 9)
    empty = torch.zeros(0, dtype=torch.long, device="cuda")
    out = emb.csr_lookup(empty, torch.zeros(4, dtype=torch.long,
                                            device="cuda"), "sum")
    out.backward(torch.ones(3, 16, device="cuda"))
    assert emb._fused_sr.tolist() == [9, 0]
    assert _same_bits(emb.weight, table.to(torch.bfloat16))


def test_ops_refuse_fp32_weight_and_bad_sr():
    from distributed_embeddings_amd.ops.embedding_lookup import (
        csr_lookup_fused_optimizer)
    case = _helper_case()
    lr = torch.tensor([_LR])
    empty = torch.empty(0)
    sr = torch.tensor([1, 0])
    w32 = _exact_case(16)[0].clone().requires_grad_(True)
    with pytest.raises(ValueError):
        csr_lookup_fused_optimizer(w32, case["ids_hot"], case["splits"], "sum",
                                   lr, empty, False, 0.0, None, None, sr)
    wbf = _exact_case(16)[0].to(torch.bfloat16).requires_grad_(True)
    for bad in (torch.tensor([1, 0], dtype=torch.int32), torch.tensor([1])):
        with pytest.raises(ValueError):
            csr_lookup_fused_optimizer(wbf, case["ids_hot"], case["splits"],
                                       "sum", lr, empty, False, 0.0, None,
                                       None, bad)


@pytest.mark.gpu
@requires_gpu
def test_extension_refuses_fp32_weight():
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    table, up, _ = _exact_case(16)
    sr = torch.tensor([1, 0], device="cuda")
    lr = torch.tensor([_LR], device="cuda")
    empty = torch.empty(0, device="cuda")
    ids, splits = case["ids_hot"].cuda(), case["splits"].cuda()
    with pytest.raises(RuntimeError):
        ext.csr_fused_optimizer_apply(table.cuda(), empty, ids, splits,
                                      up.cuda(), lr, False, False, 0.0, None,
                                      sr)
    uniq = torch.unique(case["ids_hot"]).cuda()
    rows = torch.zeros(uniq.numel(), 16, device="cuda")
    with pytest.raises(RuntimeError):
        ext.sparse_row_update(table.cuda(), empty, uniq, rows, _LR, 0.0,
                              False, sr)
    assert sr.tolist() == [1, 0]


# --------------------------------------------------------------------------
# 4. graph replay draws fresh bits
# --------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
def test_graph_replay_advances_the_device_counter():
    width, seed = 64, 77
    table, up, per_id_w = _exact_case(width)
    emb = _make_sgd_layer(table, "cuda", seed)
    grad64 = _exact_dense_grad(up, per_id_w)
    inputs = _fused_inputs("cuda", up, per_id_w, False)  # before the capture

    def step():
        _fused_step(emb, *inputs)

    for _ in range(3):  # warm up on the capture's own (single) stream
        step()
    torch.cuda.synchronize()
    k = int(emb._fused_sr[1])
    assert k == 3
    w = emb.weight.detach().cpu().clone()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    torch.cuda.synchronize()
    assert _same_bits(emb.weight, w), "capture ran the step"
    assert int(emb._fused_sr[1]) == k
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    stuck = w
    for i in range(3):
        w = _sr_table(_exact_step(w, grad64), seed, k + i)
        stuck = _sr_table(_exact_step(stuck, grad64), seed, k)
    assert not _same_bits(w, stuck)  # a host-side counter would show
    assert _same_bits(emb.weight, w)
    assert emb._fused_sr.tolist() == [seed, k + 3]


# --------------------------------------------------------------------------
# 5. Adagrad and row-wise Adagrad: bounds
# --------------------------------------------------------------------------

def _bf16_order(t):
    """bf16 tensor -> integers ordered like the values (-0 == +0 == 0)."""
    b = _bits(t)
    mag = b & 0x7FFF
    return torch.where(b >= 0x8000, -mag, mag)


def _bf16_from_order(k):
    b = torch.where(k < 0, 0x8000 | (-k), k)
    b = torch.where(b >= 0x8000, b - 0x10000, b).to(torch.int16)
    return b.view(torch.bfloat16)


def _bf16_floor(y):
    """Largest bf16 <= y (float64, finite, far from overflow)."""
    t = y.to(torch.bfloat16)
    down = _bf16_from_order(_bf16_order(t) - 1)
    return torch.where(t.double() <= y, t.double(), down.double())


def _bf16_ceil(y):
    t = y.to(torch.bfloat16)
    up = _bf16_from_order(_bf16_order(t) + 1)
    return torch.where(t.double() >= y, t.double(), up.double())


def test_bf16_floor_and_ceil():
    y = torch.tensor([1.0, 1.001, -1.001, 0.0, 1e-3, -300.7, 1.0 + 2.0 ** -7],
                     dtype=torch.float64)
    lo, hi = _bf16_floor(y), _bf16_ceil(y)
    assert bool((lo <= y).all()) and bool((y <= hi).all())
    assert lo.tolist()[:3] == [1.0, 1.0, -(1.0 + 2.0 ** -7)]
    assert hi.tolist()[:3] == [1.0, 1.0 + 2.0 ** -7, -1.0]
    for v in (lo, hi):
        assert torch.equal(v, v.to(torch.bfloat16).double())


def _adagrad_step(w0, g, rowwise, lr, eps):
    """One step from state 1 in g's precision on the dense summed grad."""
    if rowwise:
        st = 1.0 + (g * g).mean(dim=1)
        return w0.to(g.dtype) - lr * g / (st.sqrt() + eps).unsqueeze(1), st
    st = 1.0 + g * g
    return w0.to(g.dtype) - lr * g / (st.sqrt() + eps), st


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("method", ["adagrad", "rowwise_adagrad"])
def test_adagrad_within_bounds(method, combiner):
    """Every stored weight lies between the bf16 neighbours of the float64
    result widened by the summation bound of test_gpu.py, and rounding
    touches the weights only: the state is the round-to-nearest run's, bit
    for bit.  (The hot row's three chunk sums of 128, 128 and 44 terms meet
    in fp32 scratch by atomicAdd; measured on the MI355X, the two calls of
    one case left that row's state bitwise equal in all 72 cases.)"""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"], case["splits"].cuda()
    rowwise = method == "rowwise_adagrad"
    lr_v = 0.125
    lr = torch.tensor([lr_v], device="cuda")
    eps = float(torch.tensor(1e-10, dtype=torch.float32))
    atol = _terms_atol(torch.bincount(ids, minlength=_HELPER_VOCAB))
    touched = torch.bincount(ids, minlength=_HELPER_VOCAB) > 0
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        w0 = table.to(torch.bfloat16)
        ones = torch.ones(_HELPER_VOCAB if rowwise
                          else (_HELPER_VOCAB, width))
        for gdt in (torch.float32, torch.bfloat16):
            gq = grad.to(gdt)
            g64 = _dense_grad_ref(gq, ids, case, combiner, torch.float64)
            g32 = _dense_grad_ref(gq, ids, case, combiner, torch.float32)
            x64, _ = _adagrad_step(w0, g64, rowwise, lr_v, eps)
            w32, _ = _adagrad_step(w0, g32, rowwise, lr_v, eps)
            tag = f"{method} {combiner} w{width} {gdt}"
            _assert_within(f"cpu fp32 weight {tag}", w32, x64, atol)
            lo, hi = _bf16_floor(x64 - atol), _bf16_ceil(x64 + atol)
            w_rne, st_rne = w0.cuda(), ones.cuda()
            ext.csr_fused_optimizer_apply(w_rne, st_rne, ids.cuda(), splits,
                                          gq.cuda(), lr, combiner == "mean",
                                          True, eps)
            w, st = w0.cuda(), ones.cuda()
            sr = torch.tensor([31 + width, 2], device="cuda")
            ext.csr_fused_optimizer_apply(w, st, ids.cuda(), splits,
                                          gq.cuda(), lr, combiner == "mean",
                                          True, eps, None, sr)
            got = w.cpu().double()
            below, above = int((got < lo).sum()), int((got > hi).sum())
            print(f"{tag}: {below} below, {above} above, "
                  f"{int((_bits(w) != _bits(w_rne)).sum())} differ from RNE")
            assert below == 0 and above == 0, tag
            differ = (st != st_rne).sum(dim=-1).nonzero().flatten().tolist()
            print(f"{tag}: rows whose state differs from RNE: {differ}")
            assert torch.equal(st, st_rne), f"state {tag}"
            assert _same_bits(w[~touched.cuda()], w0[~touched])
            assert not _same_bits(w, w_rne), f"{tag}: rounding stayed RNE"
            assert sr.tolist() == [31 + width, 3]


# --------------------------------------------------------------------------
# 6. drift: the reason for the feature
# --------------------------------------------------------------------------

_DRIFT_VOCAB = _DRIFT_WIDTH = 64
_DRIFT_STEPS = 256
# Per step the rounding error is at most half an ulp in magnitude, so its
# standard deviation is at most half of the 2**-7 ulp of [1, 2): 2**-8.
# Steps and elements are independent: sigma(mean) <= 2**-8 * sqrt(256) /
# sqrt(4096) = 2**-10.
_DRIFT_BOUND = 6 * 2.0 ** -8 * math.sqrt(_DRIFT_STEPS) / math.sqrt(
    _DRIFT_VOCAB * _DRIFT_WIDTH)


def _drift_layer(device, method, lr, dtype, stochastic_rounding):
    from distributed_embeddings_amd import Embedding
    emb = Embedding(_DRIFT_VOCAB, _DRIFT_WIDTH, combiner="sum",
                    dtype=dtype).to(device)
    with torch.no_grad():
        emb.weight.fill_(1.0)
    emb.enable_fused_optimizer(method, lr,
                               stochastic_rounding=stochastic_rounding,
                               seed=2024 if stochastic_rounding else None)
    return emb


def _drift_run(emb, grad_value):
    dev = emb.weight.device
    ids = torch.arange(_DRIFT_VOCAB, device=dev).view(-1, 1)  # each id once
    up = torch.full((_DRIFT_VOCAB, _DRIFT_WIDTH), grad_value, device=dev)
    for _ in range(_DRIFT_STEPS):
        emb(ids).backward(up)
    return emb.weight.detach().float().cpu()


def _check_sgd_drift(device):
    assert _DRIFT_BOUND == 6 * 2.0 ** -10
    sr = _drift_layer(device, "sgd", 1.0, torch.bfloat16, True)
    w = _drift_run(sr, 2.0 ** -10)  # lr * g = 2**-10: the answer is 0.75
    err = abs(float(w.double().mean()) - 0.75)
    print(f"sgd {device}: mean error {err:.3e}, bound {_DRIFT_BOUND:.3e}")
    assert err < _DRIFT_BOUND
    assert int(sr._fused_sr[1]) == _DRIFT_STEPS
    rne = _drift_layer(device, "sgd", 1.0, torch.bfloat16, False)
    w_rne = _drift_run(rne, 2.0 ** -10)
    # the case the feature exists for: nearest-even drops every update
    assert bool((w_rne == 1.0).all())


def test_sgd_drift_cpu():
    _check_sgd_drift("cpu")


@pytest.mark.gpu
@requires_gpu
def test_sgd_drift_gpu():
    _check_sgd_drift("cuda")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("method", ["adagrad", "rowwise_adagrad"])
def test_adagrad_drift_gpu(method):
    """Fixed ids and upstream grad: the state does not depend on the weights,
    so step t moves every weight by lr / sqrt(t) whatever was stored before;
    with lr = 2**-7 the weights stay inside (0.5, 1], below the ulp the bound
    is derived for.  The bf16 table's mean follows the fp32 table's."""
    lr, g = 2.0 ** -7, 0.5
    w_sr = _drift_run(_drift_layer("cuda", method, lr, torch.bfloat16, True),
                      g)
    w_32 = _drift_run(_drift_layer("cuda", method, lr, torch.float32, False),
                      g)
    assert float(w_32.min()) > 0.5 and float(w_32.max()) < 1.0
    err = abs(float(w_sr.double().mean()) - float(w_32.double().mean()))
    print(f"{method}: fp32 mean {float(w_32.mean()):.6f}, mean error "
          f"{err:.3e}, bound {_DRIFT_BOUND:.3e}")
    assert err < _DRIFT_BOUND


# --------------------------------------------------------------------------
# 7. SparseEmbeddingOptimizer
# --------------------------------------------------------------------------

def _check_sparse_optimizer(device, width):
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    from distributed_embeddings_amd.ops.embedding_lookup import (mix64_int,
                                                                 to_int64)
    case = _helper_case()
    table, up, per_id_w = _exact_case(width)
    rg = Ragged(case["ids_hot"].to(device), case["splits"].to(device),
                per_id_w.to(device))
    g32 = torch.Generator().manual_seed(8)
    t32 = torch.randn(_HELPER_VOCAB, width, generator=g32)
    # the lookup hands the optimizer the summed gradient in the table's
    # dtype: G rounded to bf16, still a short multiple of 1/2
    grad64 = _exact_dense_grad(up, per_id_w).to(torch.bfloat16).double()

    def make(stochastic_rounding):
        bf = Embedding(_HELPER_VOCAB, width, combiner="sum",
                       dtype=torch.bfloat16).to(device)
        fp = Embedding(_HELPER_VOCAB, width, combiner="sum").to(device)
        with torch.no_grad():
            bf.weight.copy_(table)
            fp.weight.copy_(t32)
        opt = SparseEmbeddingOptimizer(
            [fp.weight, bf.weight], lr=_LR, method="sgd",
            stochastic_rounding=stochastic_rounding, seed=606)
        return bf, fp, opt

    def step(bf, fp, opt):
        opt.zero_grad()
        bf(rg).backward(up.to(device=device, dtype=torch.bfloat16))
        fp(rg).backward(up.to(device))
        opt.step()

    bf, fp, opt = make(True)
    bf0, fp0, opt0 = make(False)
    step(bf, fp, opt)
    step(bf0, fp0, opt0)
    sr = opt.state[bf.weight]["sr"]
    assert sr.dtype == torch.int64 and sr.device == bf.weight.device
    seed = to_int64(mix64_int(mix64_int(606) ^ 1))  # second param
    assert sr.tolist() == [seed, 1]
    assert "sr" not in opt.state[fp.weight]
    assert "sr" not in opt0.state[bf0.weight]
    assert torch.equal(fp.weight, fp0.weight), "fp32 param changed"
    assert not torch.equal(fp.weight.detach().cpu(), t32)
    w = table.to(torch.bfloat16)
    new32 = _exact_step(w, grad64)
    want = _sr_table(new32, seed, 0)
    assert not _same_bits(want, new32.to(torch.bfloat16))
    assert _same_bits(bf0.weight, new32.to(torch.bfloat16))
    assert _same_bits(bf.weight, want)

    # a fresh optimizer that loads the state continues the stream
    opt2 = SparseEmbeddingOptimizer(
        [fp.weight, bf.weight], lr=_LR, method="sgd",
        stochastic_rounding=True, seed=1)
    opt2.load_state_dict(opt.state_dict())
    sr2 = opt2.state[bf.weight]["sr"]
    assert sr2.dtype == torch.int64 and sr2.tolist() == [seed, 1]
    assert sr2.device == bf.weight.device
    step(bf, fp, opt2)
    new32 = _exact_step(want, grad64)
    assert not _same_bits(_sr_table(new32, seed, 1),
                          _sr_table(new32, seed, 0))
    assert _same_bits(bf.weight, _sr_table(new32, seed, 1))
    assert opt2.state[bf.weight]["sr"].tolist() == [seed, 2]


def test_sparse_optimizer_cpu():
    _check_sparse_optimizer("cpu", 16)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("width", [16, 68, 130])
def test_sparse_optimizer_gpu(width):
    """sparse_row_update gives a wave one row: one, two and three column
    passes."""
    _check_sparse_optimizer("cuda", width)


# --------------------------------------------------------------------------
# 8. layer and distributed plumbing (CPU, gloo)
# --------------------------------------------------------------------------

def test_layer_buffer_and_errors():
    from distributed_embeddings_amd import Embedding
    emb = Embedding(10, 4, combiner="sum", dtype=torch.bfloat16)
    emb.weight.de_local = True
    emb.enable_fused_optimizer("adagrad", 0.1)
    assert "_fused_sr" not in emb.state_dict()  # off by default
    emb.enable_fused_optimizer("adagrad", 0.1, stochastic_rounding=True,
                               seed=5)
    assert emb._fused_sr.tolist() == [5, 0]
    assert emb._fused_sr.de_local is True and emb._fused_state.de_local is True
    assert emb.state_dict()["_fused_sr"].tolist() == [5, 0]
    emb.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True, seed=6)
    assert emb._fused_sr.tolist() == [6, 0]  # replaced
    emb.enable_fused_optimizer("sgd", 0.1)
    assert getattr(emb, "_fused_sr", None) is None
    assert "_fused_sr" not in emb.state_dict()
    # seed=None follows torch.manual_seed
    seeds = []
    for _ in range(2):
        torch.manual_seed(3)
        emb.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)
        seeds.append(int(emb._fused_sr[0]))
    emb.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)
    assert seeds[0] == seeds[1] != int(emb._fused_sr[0])
    # a resumed run continues the stream
    emb._fused_sr[1] = 41
    other = Embedding(10, 4, combiner="sum", dtype=torch.bfloat16)
    other.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True, seed=0)
    other.load_state_dict(emb.state_dict())
    assert other._fused_sr.tolist() == [int(emb._fused_sr[0]), 41]

    fp32 = Embedding(10, 4, combiner="sum")
    with pytest.raises(ValueError):
        fp32.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)
    assert getattr(fp32, "_fused_lr", None) is None
    q = Embedding(10, 4, combiner="sum", dtype=torch.bfloat16).quantize_()
    with pytest.raises(RuntimeError):
        q.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)


_DIST_SIZES = [8, 400, 900]


def _dist_model(dtype=torch.bfloat16):
    import distributed_embeddings_amd as de
    # table 0 data-parallel, table 1 column-sliced, table 2 row-sliced
    model = de.DistributedEmbedding(
        [de.TableConfig(s, 16, "sum") for s in _DIST_SIZES],
        data_parallel_threshold=8 * 16, row_slice_threshold=900 * 16,
        column_slice_threshold=400 * 16 - 1, table_dtype=dtype)
    g = torch.Generator().manual_seed(4)
    model.set_weights([torch.randn(s, 16, generator=g).numpy()
                       for s in _DIST_SIZES])
    return model


def _dist_train(rank, seed):
    model = _dist_model()
    model.enable_fused_optimizer("sgd", 2.0 ** -6, stochastic_rounding=True,
                                 seed=seed)
    g = torch.Generator().manual_seed(100 + rank)
    for _ in range(2):
        xs = [torch.randint(0, s, (6, 3), generator=g) for s in _DIST_SIZES]
        sum((o.float() * o.float()).sum() for o in model(xs)).backward()
    fused = list(model.col_layers) + list(model.row_layers)
    return model, [torch.cat([lyr.weight.detach().float().reshape(-1)
                              for lyr in fused])]


def _dist_plumbing_worker(rank, world):
    model, w_a = _dist_train(rank, 11)
    plan = model.strategy
    assert plan.dp_table_ids and plan.col_table_ids and plan.row_table_ids
    fused = list(model.col_layers) + list(model.row_layers)
    assert fused and len(model.dp_layers) == 1
    keys = [k for k in model.state_dict() if k.endswith("_fused_sr")]
    assert len(keys) == len(fused)
    for lyr in model.dp_layers:  # sparse grads, no fused optimizer, no buffer
        assert getattr(lyr, "_fused_lr", None) is None
        assert getattr(lyr, "_fused_sr", None) is None
    seeds = []
    for lyr in fused:
        assert lyr._fused_lr is not None
        assert lyr._fused_sr.dtype == torch.int64
        assert int(lyr._fused_sr[1]) == 2  # two applied updates
        assert lyr._fused_sr.de_local == lyr._fused_state.de_local
        seeds.append(int(lyr._fused_sr[0]))
    _, w_a2 = _dist_train(rank, 11)
    _, w_b = _dist_train(rank, 12)
    same = all(torch.equal(x, y) for x, y in zip(w_a, w_a2))
    differ = any(not torch.equal(x, y) for x, y in zip(w_a, w_b))

    fp32 = _dist_model(torch.float32)
    try:
        fp32.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)
        fp32_raises = False
    except ValueError:
        fp32_raises = True
    quant = _dist_model().quantize_()
    try:
        quant.enable_fused_optimizer("sgd", 0.1, stochastic_rounding=True)
        quant_raises = False
    except RuntimeError:
        quant_raises = True
    return dict(seeds=seeds, same=same, differ=differ,
                fp32_raises=fp32_raises, quant_raises=quant_raises)


@pytest.mark.parametrize("world", [1, 2])
def test_distributed_plumbing(world):
    results = run_distributed(_dist_plumbing_worker, world=world)
    seeds = [s for r in results for s in r["seeds"]]
    assert len(seeds) >= 2
    assert len(set(seeds)) == len(seeds), "two shards share a bit stream"
    for r in results:
        assert r["same"], "one seed, two runs, different weights"
        assert r["differ"], "two seeds, the same weights"
        assert r["fp32_raises"] and r["quant_raises"]
