"""Lazy Adam in the fused embedding optimizers.

For step t (1 for the first applied update) and every unique in-range id u of
the step, with G[u] the fp32 sum of that id's gradient rows:

    m[u] = b1*m[u] + (1-b1)*G[u]
    v[u] = b2*v[u] + (1-b2)*G[u]^2
    a_t  = lr * sqrt(1 - b2^t) / (1 - b1^t)
    w[u] = w[u] - a_t * m[u] / (sqrt(v[u]) + eps)

Rows whose id does not occur keep w, m and v bit for bit.  This is
torch.optim.SparseAdam's update: the CPU tests hold the Python paths to
SparseAdam itself at the project's CPU bound (rtol 1e-5, atol 1e-6: both
sides consume the same fp32 G, only the op order differs), the GPU tests hold
the HIP kernels to the formula in float64 on the case test_gpu.py builds for
the shared gather-reduce helpers.

GPU tolerances (derived, not tuned), per element, with tol_G =
_terms_atol(counts) the summation bound of test_gpu.py (1e-4 up to 7 terms,
1e-3 up to 300) and 1e-6 for the handful of fp32 roundings of values of size
O(1) (ulp 1.2e-7 at 1, 4.8e-7 at 4):

    tol_m = (1-b1) * tol_G + 1e-6
    tol_v = (1-b2) * 2 |G_ref| * tol_G + 1e-6
    tol_w = a_t * (tol_m / sqrt(v_lo) + |m_ref| * tol_v / (2 v_lo^1.5))
            + 1e-6  (+ 2^-8 |w_ref| where the table is bf16: one rounding)

tol_w is the first-order propagation of tol_m and tol_v through
a_t * m / (sqrt(v) + eps): |d/dm| = a_t / (sqrt(v) + eps) <= a_t / sqrt(v_lo)
and |d/dv| = a_t |m| / (2 sqrt(v) (sqrt(v) + eps)^2) <= a_t |m| /
(2 v_lo^1.5).  The well-conditioned tests prefill v with U[0.01, 1], so
v >= b2 * 0.01 = v_lo after the step.  The second-order terms are smaller by
tol_v / v_lo < 3e-3.

From a zero state the first step is sign-like, w - lr*sqrt(1-b2)*G /
(sqrt(1-b2)*|G| + eps), and no lower bound on v exists; with eps = 1e-3 it is
Lipschitz in G with constant lr*sqrt(1-b2)/eps, and tol_w = that constant *
tol_G + 1e-6.
"""

import math

import pytest
import torch

from conftest import run_distributed
from test_gpu import (_HELPER_VOCAB, _HELPER_WIDTHS, _assert_within,
                      _dense_grad_ref, _helper_case, _helper_dense,
                      _terms_atol)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")

_B1, _B2 = 0.9, 0.999
_LR = 0.125
_V_LO = _B2 * 0.01


def _a_t(lr, t, b1=_B1, b2=_B2):
    return lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def _adam_step(w0, m0, v0, g, touched, lr, eps, t, b1=_B1, b2=_B2):
    """The definition in g's precision on a dense [vocab, width] summed grad;
    rows outside `touched` come back as they went in."""
    dt = g.dtype
    w0, m0, v0 = w0.to(dt), m0.to(dt), v0.to(dt)
    m = b1 * m0 + (1 - b1) * g
    v = b2 * v0 + (1 - b2) * g * g
    w = w0 - _a_t(lr, t, b1, b2) * m / (v.sqrt() + eps)
    keep = ~touched.unsqueeze(1)
    return (torch.where(keep, w0, w), torch.where(keep, m0, m),
            torch.where(keep, v0, v))


def _tols(g_ref, m_ref, tol_g, a_t, v_lo=_V_LO):
    """(tol_m, tol_v, tol_w) of the module docstring, without the bf16 term."""
    tol_m = (1 - _B1) * tol_g + 1e-6
    tol_v = (1 - _B2) * 2 * g_ref.abs() * tol_g + 1e-6
    tol_w = a_t * (tol_m / math.sqrt(v_lo)
                   + m_ref.abs() * tol_v / (2 * v_lo ** 1.5)) + 1e-6
    return tol_m, tol_v, tol_w


def _prefill(width):
    """m = 0.1 N(0,1), v = U[0.01, 1], as one [2, vocab, width] state."""
    g = torch.Generator().manual_seed(900 + width)
    m = 0.1 * torch.randn(_HELPER_VOCAB, width, generator=g)
    v = 0.01 + 0.99 * torch.rand(_HELPER_VOCAB, width, generator=g)
    return torch.stack([m, v]).contiguous()


# --------------------------------------------------------------------------
# CPU
# --------------------------------------------------------------------------

_CPU = dict(rtol=1e-5, atol=1e-6)


def _ragged_batch(gen, rows, vocab, weighted):
    from distributed_embeddings_amd import Ragged
    lengths = torch.randint(0, 5, (rows,), generator=gen)
    lengths[0] = 4
    values = torch.randint(0, vocab, (int(lengths.sum()),), generator=gen)
    values[:2] = 1  # one id twice in one bag
    w = (torch.rand(values.numel(), generator=gen) + 0.5) if weighted else None
    return Ragged.from_row_lengths(values, lengths, w)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_fused_layer_cpu_matches_sparse_adam(combiner, weighted, seed):
    from distributed_embeddings_amd import Embedding
    vocab, width, rows, lr, eps = 30, 6, 9, 0.01, 1e-8
    emb = Embedding(vocab, width, combiner=combiner)
    twin = Embedding(vocab, width, combiner=combiner)
    with torch.no_grad():
        twin.weight.copy_(emb.weight)
    emb.enable_fused_optimizer("lazy_adam", lr, eps)
    assert emb._fused_state.shape == (2, vocab, width)
    assert emb._fused_state.dtype == torch.float32
    assert emb._fused_step.dtype == torch.int64
    assert emb._fused_step.tolist() == [0]
    opt = torch.optim.SparseAdam(twin.parameters(), lr=lr, eps=eps)
    gen = torch.Generator().manual_seed(77)
    coef = torch.randn(rows, width, generator=gen)
    w0 = emb.weight.detach().clone()
    for _ in range(5):
        rg = _ragged_batch(gen, rows, vocab, weighted)
        (emb(rg) * coef).sum().backward()
        opt.zero_grad()
        (twin(rg) * coef).sum().backward()
        assert twin.weight.grad.is_sparse
        opt.step()
        assert emb.weight.grad is None
    assert not torch.equal(emb.weight.detach(), w0)
    st = opt.state[twin.weight]
    assert torch.allclose(emb.weight.detach(), twin.weight.detach(), **_CPU)
    assert torch.allclose(emb._fused_state[0], st["exp_avg"], **_CPU)
    assert torch.allclose(emb._fused_state[1], st["exp_avg_sq"], **_CPU)
    assert emb._fused_step.tolist() == [5]


def test_sparse_optimizer_cpu_matches_sparse_adam(seed):
    from distributed_embeddings_amd import Embedding, SparseEmbeddingOptimizer
    vocab, width, rows, lr, eps = 30, 6, 9, 0.01, 1e-8
    emb = Embedding(vocab, width, combiner="sum")
    twin = Embedding(vocab, width, combiner="sum")
    dense = torch.nn.Linear(width, 2)
    with torch.no_grad():
        twin.weight.copy_(emb.weight)
    opt = SparseEmbeddingOptimizer(
        list(emb.parameters()) + list(dense.parameters()), lr=lr,
        method="lazy_adam", eps=eps, betas=(_B1, _B2))
    ref = torch.optim.SparseAdam(twin.parameters(), lr=lr, eps=eps)
    gen = torch.Generator().manual_seed(78)
    coef = torch.randn(rows, 2, generator=gen)
    d_w = dense.weight.detach().double().clone()
    d_m, d_v = torch.zeros_like(d_w), torch.zeros_like(d_w)
    everything = torch.ones(2, dtype=torch.bool)
    for t in range(1, 6):
        rg = _ragged_batch(gen, rows, vocab, False)
        opt.zero_grad()
        out = emb(rg)
        (dense(out) * coef).sum().backward()
        up = coef @ dense.weight.detach()
        d_g = (coef.t() @ out.detach()).double()
        opt.step()
        ref.zero_grad()
        (twin(rg) * up).sum().backward()
        ref.step()
        # the dense-grad param takes the same formula over all elements
        d_w, d_m, d_v = _adam_step(d_w, d_m, d_v, d_g, everything, lr, eps, t)
        assert torch.allclose(dense.weight.detach().double(), d_w, **_CPU)
    assert torch.allclose(emb.weight.detach(), twin.weight.detach(), **_CPU)
    st, st_ref = opt.state[emb.weight], ref.state[twin.weight]
    assert st["exp_avgs"].shape == (2, vocab, width)
    assert st["exp_avgs"].dtype == torch.float32
    assert torch.allclose(st["exp_avgs"][0], st_ref["exp_avg"], **_CPU)
    assert torch.allclose(st["exp_avgs"][1], st_ref["exp_avg_sq"], **_CPU)
    assert st["step"] == 5
    d_st = opt.state[dense.weight]
    assert torch.allclose(d_st["exp_avgs"][0].double(), d_m, **_CPU)
    assert torch.allclose(d_st["exp_avgs"][1].double(), d_v, **_CPU)

    # state_dict round trip: the next step equals the uninterrupted run's
    emb2 = Embedding(vocab, width, combiner="sum")
    dense2 = torch.nn.Linear(width, 2)
    emb2.load_state_dict(emb.state_dict())
    dense2.load_state_dict(dense.state_dict())
    opt2 = SparseEmbeddingOptimizer(
        list(emb2.parameters()) + list(dense2.parameters()), lr=lr,
        method="lazy_adam", eps=eps, betas=(_B1, _B2))
    opt2.load_state_dict(opt.state_dict())
    rg = _ragged_batch(gen, rows, vocab, False)
    for e, d, o in ((emb, dense, opt), (emb2, dense2, opt2)):
        o.zero_grad()
        (d(e(rg)) * coef).sum().backward()
        o.step()
    assert opt2.state[emb2.weight]["step"] == 6
    assert torch.equal(emb2.weight.detach(), emb.weight.detach())
    assert torch.equal(dense2.weight.detach(), dense.weight.detach())
    assert torch.equal(opt2.state[emb2.weight]["exp_avgs"], st["exp_avgs"])


def test_sparse_optimizer_cpu_bf16_stochastic_rounding(seed):
    """bf16 table: fp32 moments, and with stochastic rounding they are the
    nearest-even run's bit for bit while the weights differ."""
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    rg = Ragged.from_lists([[1, 1, 3], [1, 5], [7, 3]])
    up = torch.linspace(0.5, 1.5, 12).view(3, 4).bfloat16()
    runs = []
    for sr in (False, True):
        torch.manual_seed(3)
        emb = Embedding(10, 4, combiner="sum", dtype=torch.bfloat16)
        opt = SparseEmbeddingOptimizer(emb.parameters(), lr=2.0 ** -9,
                                       method="lazy_adam", eps=1e-8,
                                       stochastic_rounding=sr, seed=5)
        for _ in range(4):
            opt.zero_grad()
            emb(rg).backward(up)
            opt.step()
        st = opt.state[emb.weight]
        assert st["exp_avgs"].dtype == torch.float32 and st["step"] == 4
        if sr:
            assert st["sr"].tolist()[1] == 4
        runs.append((emb.weight.detach().clone(), st["exp_avgs"].clone()))
    assert torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], runs[1][0])


def test_untouched_rows_validation_and_resume(seed):
    from distributed_embeddings_amd import Embedding, Ragged
    vocab, width, lr, eps = 10, 4, 0.01, 1e-8
    emb = Embedding(vocab, width, combiner="sum")
    emb.enable_fused_optimizer("lazy_adam", lr, eps)
    up = torch.linspace(0.5, 1.5, 3 * width).view(3, width)
    # out-of-range ids (-1, 10, 2**40) are ignored
    first = Ragged(torch.tensor([1, -1, 3, 10, 1, 7, 1 << 40]),
                   torch.tensor([0, 3, 5, 7]))
    second = Ragged.from_lists([[1, 7], [5, 5, 5], [2]])
    for rg, touched_ids in ((first, [1, 3, 7]), (second, [1, 2, 5, 7])):
        w_b = emb.weight.detach().clone()
        st_b = emb._fused_state.clone()
        emb(rg).backward(up)
        touched = torch.zeros(vocab, dtype=torch.bool)
        touched[touched_ids] = True
        # no decay: untouched rows keep w, m and v bit for bit
        assert torch.equal(emb.weight.detach()[~touched], w_b[~touched])
        assert torch.equal(emb._fused_state[:, ~touched], st_b[:, ~touched])
        assert bool((emb.weight.detach()[touched] != w_b[touched]).all())
        assert bool((emb._fused_state[1][touched] > st_b[1][touched]).all())
    assert emb._fused_step.tolist() == [2]

    # an empty batch changes nothing and does not advance the step
    w_b, st_b = emb.weight.detach().clone(), emb._fused_state.clone()
    empty = Ragged(torch.zeros(0, dtype=torch.long),
                   torch.zeros(4, dtype=torch.long))
    emb(empty).backward(up)
    assert torch.equal(emb.weight.detach(), w_b)
    assert torch.equal(emb._fused_state, st_b)
    assert emb._fused_step.tolist() == [2]

    # resume: state_dict -> fresh layer -> the next step is bit-identical
    assert "_fused_step" in emb.state_dict()
    other = Embedding(vocab, width, combiner="sum")
    other.enable_fused_optimizer("lazy_adam", lr, eps)
    other.load_state_dict(emb.state_dict())
    assert other._fused_step.tolist() == [2]
    emb(first).backward(up)
    other(first).backward(up)
    assert other._fused_step.tolist() == [3]
    assert torch.equal(other.weight.detach(), emb.weight.detach())
    assert torch.equal(other._fused_state, emb._fused_state)

    emb.enable_fused_optimizer("sgd", lr)
    assert "_fused_step" not in emb._buffers
    assert "_fused_step" not in emb.state_dict()
    assert emb._fused_state.numel() == 0
    with pytest.raises(ValueError):
        emb.enable_fused_optimizer("lazy_adam", lr, betas=(1.0, 0.9))
    with pytest.raises(ValueError):
        emb.enable_fused_optimizer("lazy_adam", lr, betas=(0.9, -0.1))
    with pytest.raises(ValueError):
        emb.enable_fused_optimizer("adam", lr)


def _twin_tables(sizes, width, combiners, weights, lr, eps):
    from distributed_embeddings_amd import Embedding
    twins = []
    for size, comb, w in zip(sizes, combiners, weights):
        e = Embedding(size, width, combiner=comb)
        with torch.no_grad():
            e.weight.copy_(w)
        e.enable_fused_optimizer("lazy_adam", lr, eps)
        twins.append(e)
    return twins


def test_distributed_embedding_world1_matches_twin():
    import distributed_embeddings_amd as de
    sizes, width, combiners, lr, eps = [40, 30], 8, ["sum", "mean"], 0.01, 1e-8
    g = torch.Generator().manual_seed(5)
    weights = [torch.randn(s, width, generator=g) for s in sizes]
    model = de.DistributedEmbedding(
        [de.TableConfig(s, width, c) for s, c in zip(sizes, combiners)])
    model.set_weights([w.numpy() for w in weights])
    model.enable_fused_optimizer("lazy_adam", lr, eps, betas=(0.8, 0.99))
    fused = [lyr for lyr in list(model.col_layers) + list(model.row_layers)
             if getattr(lyr, "_fused_lr", None) is not None]
    assert fused
    for lyr in fused:
        assert lyr._fused_state.shape == (2,) + tuple(lyr.weight.shape)
        assert lyr._fused_betas == (0.8, 0.99)
    twins = _twin_tables(sizes, width, combiners, weights, lr, eps)
    for e in twins:
        e.enable_fused_optimizer("lazy_adam", lr, eps, betas=(0.8, 0.99))
    for _ in range(3):
        xs = [torch.randint(0, 6, (8, 3), generator=g) for _ in sizes]
        sum((o * o).sum() for o in model(xs)).backward()
        sum(e(x).square().sum() for e, x in zip(twins, xs)).backward()
    for lyr in fused:
        assert lyr._fused_step.tolist() == [3]
    for got, e, w in zip(model.get_weights(), twins, weights):
        assert not torch.equal(e.weight.detach(), w)
        assert torch.allclose(torch.as_tensor(got), e.weight.detach(), **_CPU)


# each rank's four samples hit both row shards, and ids 5 and 300 occur on
# both ranks: the owning shard has to see one summed row
_W2_IDS = [5, 5, 300, 3, 5, 300, 399, 210]
_W2_VOCAB, _W2_WIDTH, _W2_LR, _W2_EPS = 400, 16, 0.01, 1e-8


def _w2_coef():
    return (torch.arange(1, len(_W2_IDS) + 1).float().unsqueeze(1)
            * torch.linspace(0.5, 1.5, _W2_WIDTH).unsqueeze(0))


def _w2_table():
    return torch.randn(_W2_VOCAB, _W2_WIDTH,
                       generator=torch.Generator().manual_seed(9))


def _world2_worker(rank, world, sliced):
    import distributed_embeddings_amd as de
    kwargs = ({"row_slice_threshold": 1} if sliced == "row" else
              {"column_slice_threshold": _W2_VOCAB * _W2_WIDTH - 1})
    model = de.DistributedEmbedding([de.TableConfig(_W2_VOCAB, _W2_WIDTH)],
                                    **kwargs)
    if sliced == "row":
        assert len(model.row_layers) == 1 and not len(model.col_layers)
        shard = (_W2_VOCAB // 2, _W2_WIDTH)
    else:
        assert len(model.col_layers) == 1 and not len(model.row_layers)
        shard = (_W2_VOCAB, _W2_WIDTH // 2)
    model.set_weights([_w2_table().numpy()])
    model.enable_fused_optimizer("lazy_adam", _W2_LR, _W2_EPS)
    lyr = (list(model.row_layers) + list(model.col_layers))[0]
    assert lyr._fused_state.shape == (2,) + shard
    ids, coef = torch.tensor(_W2_IDS), _w2_coef()
    sl = slice(rank * 4, (rank + 1) * 4)
    for _ in range(3):
        (model([ids[sl]])[0] * coef[sl]).sum().backward()
    assert lyr._fused_step.tolist() == [3]
    return torch.as_tensor(model.get_weights(all_ranks=True)[0])


@pytest.mark.parametrize("sliced", ["row", "column"])
def test_sliced_world2_matches_twin(sliced):
    """Lazy Adam is element-wise, so a sliced table trains like the whole."""
    from distributed_embeddings_amd import Embedding
    results = run_distributed(_world2_worker, world=2, args=(sliced,))
    twin = Embedding(_W2_VOCAB, _W2_WIDTH)
    with torch.no_grad():
        twin.weight.copy_(_w2_table())
    twin.enable_fused_optimizer("lazy_adam", _W2_LR, _W2_EPS)
    for _ in range(3):
        (twin(torch.tensor(_W2_IDS)) * _w2_coef()).sum().backward()
    assert not torch.equal(twin.weight.detach(), _w2_table())
    for got in results:
        assert torch.allclose(got, twin.weight.detach(), **_CPU)


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------

def _apply(ext, w, state, step, ids, splits, grad, lr, combiner, eps, sr=None):
    ext.csr_fused_optimizer_apply(w, state, ids, splits, grad, lr,
                                  combiner == "mean", False, eps, None, sr,
                                  adam_step=step, beta1=_B1, beta2=_B2)


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_fused_update_vs_fp64(combiner):
    """One apply at t = 5 from a well-conditioned state, every tiling, the
    300-long segment through scratch + finalize; bounds in the module
    docstring."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"], case["splits"].cuda()
    counts = torch.bincount(ids, minlength=_HELPER_VOCAB)
    touched = counts > 0
    assert touched.any() and not touched.all()
    tol_g = _terms_atol(counts)
    lr = torch.tensor([_LR], device="cuda")
    eps, a_t = 1e-8, _a_t(_LR, 5)
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        st0 = _prefill(width)
        for wdt in (torch.float32, torch.bfloat16):
            for gdt in (torch.float32, torch.bfloat16):
                w0, gq = table.to(wdt), grad.to(gdt)
                g64 = _dense_grad_ref(gq, ids, case, combiner, torch.float64)
                g32 = _dense_grad_ref(gq, ids, case, combiner, torch.float32)
                w_ref, m_ref, v_ref = _adam_step(w0, st0[0], st0[1], g64,
                                                 touched, _LR, eps, 5)
                assert float(v_ref[touched].min()) >= _V_LO
                tol_m, tol_v, tol_w = _tols(g64, m_ref, tol_g, a_t)
                if wdt == torch.bfloat16:
                    tol_w = tol_w + 2.0 ** -8 * w_ref.abs()
                tag = f"{combiner} w{width} {wdt} {gdt}"
                w32, m32, v32 = _adam_step(w0, st0[0], st0[1], g32, touched,
                                           _LR, eps, 5)
                _assert_within(f"cpu fp32 w {tag}", w32, w_ref, tol_w)
                _assert_within(f"cpu fp32 m {tag}", m32, m_ref, tol_m)
                _assert_within(f"cpu fp32 v {tag}", v32, v_ref, tol_v)
                w, state = w0.cuda(), st0.cuda()
                step = torch.tensor([4], device="cuda")
                _apply(ext, w, state, step, ids.cuda(), splits, gq.cuda(), lr,
                       combiner, eps)
                assert step.tolist() == [5]
                _assert_within(f"w {tag}", w.float(), w_ref, tol_w)
                _assert_within(f"m {tag}", state[0], m_ref, tol_m)
                _assert_within(f"v {tag}", state[1], v_ref, tol_v)
                assert torch.equal(w.cpu()[~touched], w0[~touched])
                assert torch.equal(state.cpu()[:, ~touched], st0[:, ~touched])


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_first_step_from_zero_state(combiner):
    """t = 1 from m = v = 0: sign-like, so eps = 1e-3 and the Lipschitz bound
    of the module docstring."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"], case["splits"].cuda()
    counts = torch.bincount(ids, minlength=_HELPER_VOCAB)
    touched = counts > 0
    tol_g = _terms_atol(counts)
    lr = torch.tensor([_LR], device="cuda")
    eps = 1e-3
    lipschitz = _LR * math.sqrt(1 - _B2) / eps
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        zeros = torch.zeros(2, _HELPER_VOCAB, width)
        for gdt in (torch.float32, torch.bfloat16):
            gq = grad.to(gdt)
            g64 = _dense_grad_ref(gq, ids, case, combiner, torch.float64)
            g32 = _dense_grad_ref(gq, ids, case, combiner, torch.float32)
            w_ref, m_ref, v_ref = _adam_step(table, zeros[0], zeros[1], g64,
                                             touched, _LR, eps, 1)
            tol_m = (1 - _B1) * tol_g + 1e-6
            tol_v = (1 - _B2) * 2 * g64.abs() * tol_g + 1e-6
            tol_w = lipschitz * tol_g + 1e-6
            tag = f"{combiner} w{width} {gdt}"
            w32, m32, v32 = _adam_step(table, zeros[0], zeros[1], g32, touched,
                                       _LR, eps, 1)
            _assert_within(f"cpu fp32 w {tag}", w32, w_ref, tol_w)
            w, state = table.cuda(), zeros.cuda()
            step = torch.zeros(1, dtype=torch.int64, device="cuda")
            _apply(ext, w, state, step, ids.cuda(), splits, gq.cuda(), lr,
                   combiner, eps)
            assert step.tolist() == [1]
            _assert_within(f"w {tag}", w, w_ref, tol_w)
            _assert_within(f"m {tag}", state[0], m_ref, tol_m)
            _assert_within(f"v {tag}", state[1], v_ref, tol_v)
            assert torch.equal(w.cpu()[~touched], table[~touched])
            assert bool((state.cpu()[:, ~touched] == 0).all())


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_stochastic_rounding_within_bounds(combiner):
    """bf16 tables: every stored weight lies between the bf16 neighbours of
    the float64 result widened by tol_w, and rounding touches the weights
    only: m and v are the nearest-even run's, bit for bit."""
    from distributed_embeddings_amd.ops import _backend
    from test_stochastic_rounding import (_bf16_ceil, _bf16_floor, _bits,
                                          _same_bits)
    ext = _backend.ops()
    case = _helper_case()
    ids, splits = case["ids_hot"], case["splits"].cuda()
    counts = torch.bincount(ids, minlength=_HELPER_VOCAB)
    touched = counts > 0
    tol_g = _terms_atol(counts)
    lr = torch.tensor([_LR], device="cuda")
    eps, a_t = 1e-8, _a_t(_LR, 5)
    for width in _HELPER_WIDTHS:
        table, grad = _helper_dense(width)
        w0, st0 = table.to(torch.bfloat16), _prefill(width)
        for gdt in (torch.float32, torch.bfloat16):
            gq = grad.to(gdt)
            g64 = _dense_grad_ref(gq, ids, case, combiner, torch.float64)
            x64, m_ref, _ = _adam_step(w0, st0[0], st0[1], g64, touched, _LR,
                                       eps, 5)
            tol_w = _tols(g64, m_ref, tol_g, a_t)[2]
            lo, hi = _bf16_floor(x64 - tol_w), _bf16_ceil(x64 + tol_w)
            tag = f"{combiner} w{width} {gdt}"
            w_rne, st_rne = w0.cuda(), st0.cuda()
            step_rne = torch.tensor([4], device="cuda")
            _apply(ext, w_rne, st_rne, step_rne, ids.cuda(), splits, gq.cuda(),
                   lr, combiner, eps)
            w, st = w0.cuda(), st0.cuda()
            step = torch.tensor([4], device="cuda")
            sr = torch.tensor([31 + width, 2], device="cuda")
            _apply(ext, w, st, step, ids.cuda(), splits, gq.cuda(), lr,
                   combiner, eps, sr)
            got = w.cpu().double()
            below, above = int((got < lo).sum()), int((got > hi).sum())
            print(f"{tag}: {below} below, {above} above, "
                  f"{int((_bits(w) != _bits(w_rne)).sum())} differ from RNE")
            assert below == 0 and above == 0, tag
            assert torch.equal(st, st_rne), f"state {tag}"
            assert _same_bits(w[~touched.cuda()], w0[~touched])
            assert not _same_bits(w, w_rne), f"{tag}: rounding stayed RNE"
            assert sr.tolist() == [31 + width, 3]
            assert step.tolist() == [5] and step_rne.tolist() == [5]


@pytest.mark.gpu
@requires_gpu
def test_row_update_vs_fp64():
    """sparse_row_update at t = 5.  The rows handed in are the kernel's exact
    input, so tol_G = 0 and only the 1e-6 rounding terms remain."""
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    case = _helper_case()
    uniq = torch.unique(case["ids_hot"])
    uniq = uniq[torch.randperm(uniq.numel(),
                               generator=torch.Generator().manual_seed(1))]
    touched = torch.bincount(case["ids_hot"], minlength=_HELPER_VOCAB) > 0
    eps, a_t = 1e-8, _a_t(_LR, 5)
    for width in (16, 68, 130):
        table, grad = _helper_dense(width)
        st0 = _prefill(width)
        g32 = _dense_grad_ref(grad, case["ids_hot"], case, "sum",
                              torch.float32)
        rows = g32[uniq].contiguous()
        for wdt in (torch.float32, torch.bfloat16):
            w0 = table.to(wdt)
            w_ref, m_ref, v_ref = _adam_step(w0, st0[0], st0[1], g32.double(),
                                             touched, _LR, eps, 5)
            tol_m, tol_v, tol_w = _tols(g32.double(), m_ref, 0.0, a_t)
            if wdt == torch.bfloat16:
                tol_w = tol_w + 2.0 ** -8 * w_ref.abs()
            tag = f"w{width} {wdt}"
            w32, m32, v32 = _adam_step(w0, st0[0], st0[1], g32, touched, _LR,
                                       eps, 5)
            _assert_within(f"cpu fp32 w {tag}", w32, w_ref, tol_w)
            w, state = w0.cuda(), st0.cuda()
            ext.sparse_row_update(w, state, uniq.cuda(), rows.cuda(), _LR,
                                  eps, False, None, adam_step=5, beta1=_B1,
                                  beta2=_B2)
            _assert_within(f"w {tag}", w.float(), w_ref, tol_w)
            _assert_within(f"m {tag}", state[0], m_ref,
                           torch.full_like(m_ref, tol_m))
            _assert_within(f"v {tag}", state[1], v_ref, tol_v)
            assert torch.equal(w.cpu()[~touched], w0[~touched])
            assert torch.equal(state.cpu()[:, ~touched], st0[:, ~touched])


@pytest.mark.gpu
@requires_gpu
def test_fused_layer_gpu_matches_sparse_optimizer():
    """The in-backward kernels and the optimizer-step kernel agree after
    three steps; ids 0 and 3 occur 2000 times each (long segments)."""
    from distributed_embeddings_amd import (Embedding, Ragged,
                                            SparseEmbeddingOptimizer)
    torch.manual_seed(31)
    w0 = torch.randn(500, 32)
    ids = torch.cat([torch.randint(0, 500, (4000,)),
                     torch.zeros(2000, dtype=torch.long),
                     torch.full((2000,), 3)]).cuda()
    ids = ids[torch.randperm(8000, device="cuda")]
    splits = torch.arange(0, 8001, 4, device="cuda")
    up = torch.randn(2000, 32, device="cuda")
    e1 = Embedding(500, 32, combiner="mean").cuda()
    e2 = Embedding(500, 32, combiner="mean").cuda()
    with torch.no_grad():
        e1.weight.copy_(w0)
        e2.weight.copy_(w0)
    e1.enable_fused_optimizer("lazy_adam", 0.1, 1e-3)
    o2 = SparseEmbeddingOptimizer(e2.parameters(), lr=0.1, method="lazy_adam",
                                  eps=1e-3)
    for _ in range(3):
        o2.zero_grad()
        e1(Ragged(ids, splits)).backward(up)
        e2(Ragged(ids, splits)).backward(up)
        o2.step()
    s1, s2 = e1._fused_state, o2.state[e2.weight]["exp_avgs"]
    assert s1.shape == s2.shape == (2, 500, 32)
    print("weight diff",
          float((e1.weight - e2.weight).detach().abs().max()),
          "state diff", float((s1 - s2).abs().max()))
    assert not torch.equal(e1.weight.detach().cpu(), w0)
    assert torch.allclose(e1.weight, e2.weight, atol=1e-3)
    assert torch.allclose(s1, s2, atol=1e-3)
    assert e1._fused_step.tolist() == [3]
    assert o2.state[e2.weight]["step"] == 3


@pytest.mark.gpu
@requires_gpu
def test_graph_capture_train_step():
    """One captured train step, replayed three times on changing ids, against
    three eager steps.  64 ids over 300 rows keep every segment on the
    in-register path, whose summation order is fixed, so the two runs are
    expected to agree bitwise (printed); asserted is tol_w of the module
    docstring per replayed step, for sums of <= 7 terms (tol_G = 1e-4).  The
    state is prefilled as in the well-conditioned tests, so v >= b2^7 * 0.01
    through the seven steps; a_t <= a_1 (it falls with t here); the loss is
    sum(w[id]^2), so |G| <= 2 * (most occurrences of one id) * max|w|; |m|
    is read off the eager run.  A captured step launches nothing: the step
    counts the warm-up steps and the replays."""
    from distributed_embeddings_amd import Embedding
    torch.manual_seed(23)
    w0 = torch.randn(300, 64)
    st0 = torch.stack([0.1 * torch.randn(300, 64),
                       0.01 + 0.99 * torch.rand(300, 64)])
    batches = [torch.randint(0, 300, (64,), device="cuda") for _ in range(7)]
    ids = batches[0].clone()
    lr, eps = 0.05, 1e-8

    def make():
        e = Embedding(300, 64).cuda()
        with torch.no_grad():
            e.weight.copy_(w0)
        e.enable_fused_optimizer("lazy_adam", lr, eps)
        e._fused_state.copy_(st0)
        return e

    def step(e, x):
        e(x).float().square().sum().backward()

    e_graph, e_eager = make(), make()
    for b in batches[:3]:
        ids.copy_(b)
        step(e_graph, ids)
        step(e_eager, b)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    ids.copy_(batches[3])
    with torch.cuda.graph(g):
        step(e_graph, ids)
    torch.cuda.synchronize()
    captured_ran = not torch.equal(e_graph.weight, e_eager.weight)
    if captured_ran:  # a runtime that runs what it captures
        step(e_eager, batches[3])
    for b in batches[4:]:
        ids.copy_(b)
        g.replay()
        step(e_eager, b)
    torch.cuda.synchronize()
    steps = 3 + int(captured_ran) + 3
    print("fused step", e_graph._fused_step.tolist(), "captured_ran",
          captured_ran)
    assert e_graph._fused_step.tolist() == [steps]
    assert e_eager._fused_step.tolist() == [steps]
    assert not torch.equal(e_eager.weight.detach().cpu(), w0)
    most = max(int(torch.bincount(b).max()) for b in batches)
    w_abs = max(float(w0.abs().max()),
                float(e_eager.weight.detach().abs().max()))
    g_abs = torch.tensor(2.0 * most * w_abs)
    m_abs = e_eager._fused_state[0].abs().max().cpu()
    tol_m, tol_v, tol_w = _tols(g_abs, m_abs, 1e-4, _a_t(lr, 1),
                                v_lo=_B2 ** 7 * 0.01)
    diff = float((e_graph.weight - e_eager.weight).detach().abs().max())
    print("graph vs eager: weight diff", diff, "bound per step",
          float(tol_w), "bitwise",
          torch.equal(e_graph.weight, e_eager.weight))
    assert diff <= 3 * float(tol_w)
    assert torch.allclose(e_graph._fused_state, e_eager._fused_state,
                          rtol=0, atol=3 * float(max(tol_m, tol_v)))


@pytest.mark.gpu
@requires_gpu
def test_empty_batch_is_a_noop_on_the_device():
    from distributed_embeddings_amd import Embedding, Ragged
    torch.manual_seed(3)
    emb = Embedding(40, 16, combiner="sum").cuda()
    emb.enable_fused_optimizer("lazy_adam", 0.1, 1e-8)
    ids = torch.randint(0, 40, (12,), device="cuda")
    splits = torch.arange(0, 13, 3, device="cuda")
    up = torch.randn(4, 16, device="cuda")
    emb(Ragged(ids, splits)).backward(up)
    assert emb._fused_step.tolist() == [1]
    w_b, st_b = emb.weight.detach().clone(), emb._fused_state.clone()
    assert bool((st_b[1] > 0).any())
    empty = Ragged(torch.zeros(0, dtype=torch.long, device="cuda"),
                   torch.zeros(5, dtype=torch.long, device="cuda"))
    emb(empty).backward(up)
    torch.cuda.synchronize()
    assert torch.equal(emb.weight.detach(), w_b)
    assert torch.equal(emb._fused_state, st_b)
    assert emb._fused_step.tolist() == [1]
