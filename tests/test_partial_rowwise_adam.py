"""Partial row-wise Adam: lazy Adam with one second moment per row,

    m[u,c] = b1*m[u,c] + (1-b1)*G[u,c];  v[u] = b2*v[u] + (1-b2)*mean_c(G[u,c]^2)
    w[u,c] = w[u,c] - a_t * m[u,c] / (sqrt(v[u]) + eps)

on the flat fp32 state m [vocab, width], v [vocab].  GPU tolerances (derived,
not tuned) by first-order propagation of tol_G = _terms_atol(counts) as in
test_lazy_adam.py, with 1e-6 for the fp32 roundings:

    tol_m = (1-b1) * tol_G + 1e-6
    tol_v = (1-b2) * mean_c(2 |G_ref| * tol_G) + 1e-6   (d mean G^2 = mean 2G dG)
    tol_w = a_t * (tol_m / sqrt(v_lo) + |m_ref| * tol_v / (2 v_lo^1.5))
            + 1e-6  (+ 2^-8 |w_ref| where the table is bf16: one rounding)

v starts in [0.01, 1], so v >= b2^t * 0.01 = v_lo after step t.  Each apply is
held to the formula in float64 on the state that apply started from.
"""

import functools
import math

import pytest
import torch

from conftest import run_distributed
from test_gpu import (_HELPER_VOCAB, _HELPER_WIDTHS, _assert_within,
                      _dense_grad_ref, _helper_case, _helper_dense,
                      _terms_atol)
from test_lazy_adam import (_B1, _B2, _CPU, _LR, _W2_EPS, _W2_IDS, _W2_LR,
                            _W2_VOCAB, _W2_WIDTH, _a_t, _ragged_batch,
                            _w2_coef, _w2_table)

_EPS = 1e-8
_METHOD = "partial_rowwise_adam"


def gpu(fn):
    return pytest.mark.gpu(pytest.mark.skipif(
        not torch.cuda.is_available(), reason="needs GPU")(fn))


def _step64(w, m, v, g, touched, t, lr=_LR, b1=_B1, b2=_B2):
    """The definition in float64 on a dense [vocab, width] summed gradient."""
    w, m, v, g = w.double(), m.double(), v.double(), g.double()
    m1 = b1 * m + (1 - b1) * g
    v1 = b2 * v + (1 - b2) * (g * g).mean(dim=1)
    w1 = w - _a_t(lr, t, b1, b2) * m1 / (v1.sqrt() + _EPS).unsqueeze(1)
    rows = touched.unsqueeze(1)
    return (torch.where(rows, w1, w), torch.where(rows, m1, m),
            torch.where(touched, v1, v))


@functools.lru_cache(maxsize=None)
def _case(width, combiner="sum", gdt=torch.float32, weighted=False,
          ids_key="ids_hot"):
    """The helper case plus two out-of-range ids; G64 one row per id."""
    case = _helper_case()
    ids = case[ids_key].clone()
    ids[int(case["splits"][11])], ids[-1] = -1, _HELPER_VOCAB
    valid = (ids >= 0) & (ids < _HELPER_VOCAB)
    gen = torch.Generator().manual_seed(900 + width)
    w = (torch.rand(ids.numel(), generator=gen) + 0.5) if weighted else None
    table, grad = _helper_dense(width)
    rows = grad.to(gdt).double()[case["row_of"]] * valid.unsqueeze(1)
    if weighted:
        rows = rows * w.double().unsqueeze(1)
    per_id = dict(row_of=torch.arange(ids.numel()),
                  lengths=case["lengths"][case["row_of"]])
    g64 = _dense_grad_ref(rows, ids.clamp(0, _HELPER_VOCAB - 1), per_id,
                          combiner, torch.float64)
    counts = torch.bincount(ids[valid], minlength=_HELPER_VOCAB)
    m0 = 0.1 * torch.randn(_HELPER_VOCAB * width, generator=gen)
    v0 = 0.01 + 0.99 * torch.rand(_HELPER_VOCAB, generator=gen)
    dev = (ids.cuda(), case["splits"].cuda(), grad.to(gdt).cuda(),
           None if w is None else w.cuda(), torch.tensor([_LR]).cuda())
    return dict(g64=g64, touched=counts > 0, table=table, dev=dev,
                tol_g=_terms_atol(counts), state=torch.cat([m0, v0]))


def _start(c, wdt=torch.float32):
    return (c["table"].to(wdt).cuda(), c["state"].cuda(),
            torch.zeros(1, dtype=torch.int64, device="cuda"))


def _apply(c, w, state, step, combiner="sum", sr=None, det=False, plan=False):
    from distributed_embeddings_amd.ops import _backend
    ext = _backend.ops()
    ids, splits, gq, pw, lr = c["dev"]
    mean = combiner == "mean"
    kw = dict(adam_step=step, beta1=_B1, beta2=_B2, deterministic=det)
    if plan:
        p = ext.csr_sort_plan(ids, splits, _HELPER_VOCAB, mean, pw)
        ext.csr_fused_optimizer_apply_planned(w, state, p, gq, lr, False, _EPS,
                                              sr, **kw)
    else:
        ext.csr_fused_optimizer_apply(w, state, ids, splits, gq, lr, mean,
                                      False, _EPS, pw, sr, **kw)


def _check_apply(tag, c, before, after, t, tol_g, sr=False):
    """`after` against one float64 step from `before`, bounds as above; with
    sr, w has to lie between the bf16 neighbours of w_ref -+ tol_w."""
    from test_stochastic_rounding import _bf16_ceil, _bf16_floor
    n, g, rest = c["g64"].numel(), c["g64"], ~c["touched"]
    w0, st0 = before[0].cpu(), before[1].cpu()
    w, m, v = _step64(w0, st0[:n].view_as(g), st0[n:], g, c["touched"], t)
    v_lo = _B2 ** t * 0.01
    tol_m = (1 - _B1) * tol_g + 1e-6
    tol_v = (1 - _B2) * (2 * g.abs() * tol_g).mean(dim=1, keepdim=True) + 1e-6
    tol_w = _a_t(_LR, t) * (tol_m / math.sqrt(v_lo)
                            + m.abs() * tol_v / (2 * v_lo ** 1.5)) + 1e-6
    if sr:
        got = after[0].cpu().double()
        assert bool(((got >= _bf16_floor(w - tol_w))
                     & (got <= _bf16_ceil(w + tol_w))).all())
    elif w0.dtype == torch.bfloat16:
        tol_w = tol_w + 2.0 ** -8 * w.abs()
    got = (after[0], after[1][:n].view_as(g), after[1][n:, None])
    refs, tols = (w, m, v[:, None]), (tol_w, tol_m.expand_as(m), tol_v)
    for name, x, ref, tol in list(zip("wmv", got, refs, tols))[int(sr):]:
        _assert_within(f"{name} {tag} t{t}", x, ref, tol)
        assert rest.any() and torch.equal(x.cpu()[rest].double(), ref[rest])


@gpu
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
@pytest.mark.parametrize("width", _HELPER_WIDTHS)
def test_fused_update_vs_fp64(width, combiner, wdt, gdt, weighted):
    c = _case(width, combiner, gdt, weighted)
    w, state, step = _start(c, wdt)
    for t in (1, 2):
        before = (w.clone(), state.clone())
        _apply(c, w, state, step, combiner)
        assert step.tolist() == [t]
        _check_apply(f"w{width}", c, before, (w, state), t, c["tol_g"])


@gpu
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("width", [3, 64, 130])
def test_row_update_vs_fp64(width, wdt):
    """The rows handed in are the kernel's exact input, so tol_G = 0."""
    from distributed_embeddings_amd.ops import _backend
    c = _case(width)
    uniq = c["touched"].nonzero().flatten().flip(0)
    rows = c["g64"].float()
    c = dict(c, g64=rows.double())
    w, state, _ = _start(c, wdt)
    before = (w.clone(), state.clone())
    _backend.ops().sparse_row_update(
        w, state, uniq.cuda(), rows[uniq].contiguous().cuda(), _LR, _EPS,
        False, None, adam_step=5, beta1=_B1, beta2=_B2)
    _check_apply(f"rows w{width}", c, before, (w, state), 5,
                 torch.zeros(_HELPER_VOCAB, 1, dtype=torch.float64))


@gpu
@pytest.mark.parametrize("width", [16, 68, 130])
def test_stochastic_rounding(width):
    """Rounding touches the weights only: m, v are the nearest-even run's."""
    from test_stochastic_rounding import _same_bits
    c = _case(width)
    w_rne, st_rne, step_rne = _start(c, torch.bfloat16)
    w, st, step = _start(c, torch.bfloat16)
    before = (w.clone(), st.clone())
    sr = torch.tensor([31 + width, 2], device="cuda")
    _apply(c, w_rne, st_rne, step_rne)
    _apply(c, w, st, step, sr=sr)
    _check_apply(f"sr w{width}", c, before, (w, st), 1, c["tol_g"], sr=True)
    assert torch.equal(st, st_rne) and not _same_bits(w, w_rne)
    assert sr.tolist() == [31 + width, 3] and step.tolist() == [1]


@gpu
@pytest.mark.parametrize("wdt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("width", [16, 68, 130])
def test_repeatable_bits(width, wdt):
    """Deterministic mode with the hot id; planned and captured applies on
    ids_rand, which has no long segment, so no atomics."""
    hot, rand = _case(width), _case(width, ids_key="ids_rand")
    graph = torch.cuda.CUDAGraph()
    for c, kw, captured in ((hot, dict(det=True), False),
                            (rand, dict(plan=True), False), (rand, {}, True)):
        w_a, st_a, step_a = _start(c, wdt)
        w_b, st_b, step_b = _start(c, wdt)
        for _ in range(3):
            _apply(c, w_a, st_a, step_a, det=kw.get("det", False))
            if not captured:
                _apply(c, w_b, st_b, step_b, **kw)
        if captured:
            torch.cuda.synchronize()
            with torch.cuda.graph(graph):
                _apply(c, w_b, st_b, step_b)
            for _ in range(3):
                graph.replay()
        assert step_a.tolist() == step_b.tolist() == [3]
        assert torch.equal(w_a.float(), w_b.float())
        assert torch.equal(st_a, st_b) and not torch.equal(st_a.cpu(),
                                                           c["state"])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_fused_layer_cpu(combiner, weighted, seed):
    """The rule in float64 on the fp32 G (a twin's sparse grad: the lookup
    is linear in the table); optimizer step, resume and validation too."""
    from distributed_embeddings_amd import Embedding, SparseEmbeddingOptimizer
    vocab, width, rows, lr, betas = 30, 6, 9, 0.01, (0.8, 0.99)
    emb = Embedding(vocab, width, combiner=combiner)
    twin = Embedding(vocab, width, combiner=combiner)
    twin.load_state_dict(emb.state_dict())
    emb.enable_fused_optimizer(_METHOD, lr, _EPS, betas=betas)
    opt = SparseEmbeddingOptimizer(twin.parameters(), lr=lr, method=_METHOD,
                                   eps=_EPS, betas=betas)
    assert emb._fused_state.shape == (vocab * (width + 1),)
    gen = torch.Generator().manual_seed(77)
    coef = torch.randn(rows, width, generator=gen)
    ref = (emb.weight.detach().clone(), torch.zeros(vocab, width),
           torch.zeros(vocab))
    for t in range(1, 6):
        rg = _ragged_batch(gen, rows, vocab, weighted)
        (emb(rg) * coef).sum().backward()
        opt.zero_grad()
        (twin(rg) * coef).sum().backward()
        g = twin.weight.grad.to_dense()
        ref = _step64(*ref, g, torch.bincount(rg.values, minlength=vocab) > 0,
                      t, lr, *betas)
        opt.step()
    assert emb.weight.grad is None and emb._fused_step.tolist() == [5]
    for got, want in zip((emb.weight.detach(), *emb.fused_moments()), ref):
        assert torch.allclose(got.double(), want, **_CPU)
    assert torch.allclose(twin.weight, emb.weight, **_CPU)
    assert torch.allclose(opt.state[twin.weight]["exp_avgs"],
                          emb._fused_state, **_CPU)
    other = Embedding(vocab, width, combiner=combiner)
    other.enable_fused_optimizer(_METHOD, lr, _EPS, betas=betas)
    other.load_state_dict(emb.state_dict())
    for e in (emb, other):
        (e(rg) * coef).sum().backward()
    assert other._fused_step.tolist() == [6]
    assert torch.equal(other.weight.detach(), emb.weight.detach())
    assert torch.equal(other._fused_state, emb._fused_state)
    for bad in ((1.0, 0.9), (0.9, -0.1)):
        with pytest.raises(ValueError):
            emb.enable_fused_optimizer(_METHOD, lr, betas=bad)
    assert emb.enable_fused_optimizer("sgd", lr)._fused_state.numel() == 0


def _world2_worker(rank, world):
    """Row shards own whole rows: their v, and so the table, equal a whole
    twin's that sees both ranks' ids."""
    import distributed_embeddings_amd as de
    model = de.DistributedEmbedding([de.TableConfig(_W2_VOCAB, _W2_WIDTH)],
                                    row_slice_threshold=1)
    model.set_weights([_w2_table().numpy()])
    twin = de.Embedding(_W2_VOCAB, _W2_WIDTH)
    with torch.no_grad():
        twin.weight.copy_(_w2_table())
    for e in (model, twin):
        e.enable_fused_optimizer(_METHOD, _W2_LR, _W2_EPS)
    lyr = model.row_layers[0]
    assert lyr._fused_state.shape == (_W2_VOCAB // 2 * (_W2_WIDTH + 1),)
    ids, coef = torch.tensor(_W2_IDS), _w2_coef()
    sl = slice(rank * 4, rank * 4 + 4)
    for _ in range(3):
        (model([ids[sl]])[0] * coef[sl]).sum().backward()
        (twin(ids) * coef).sum().backward()
    assert lyr._fused_step.tolist() == [3]
    assert not torch.equal(twin.weight.detach(), _w2_table())
    got = torch.as_tensor(model.get_weights(all_ranks=True)[0])
    assert torch.allclose(got, twin.weight.detach(), **_CPU)


def test_row_sliced_world2_matches_twin():
    run_distributed(_world2_worker, world=2)
