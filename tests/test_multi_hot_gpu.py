"""Multi-hot expansion on the GPU: the pack_ids kernel against the numpy /
torch composition (exactly: ids are integers), the modules with the kernel on
and off, hipGraph capture, and the multi-hot DLRM against the fp32 CPU model."""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

SEED = 77
VOCABS = [1, 7, 40_000_000, 2**33 + 5]


def _ids(g, vocab, shape):
    """Ids in the vocabulary with a negative one and ones at and above its
    end mixed in (those pass through unhashed)."""
    x = torch.randint(0, vocab, shape, generator=g)
    flat = x.view(-1)
    if flat.numel() >= 4:
        flat[0], flat[1], flat[2], flat[3] = -1, vocab, vocab - 1, vocab + 12345
    return x


def _segments():
    from distributed_embeddings_amd.ops.embedding_lookup import multi_hot_key
    g = torch.Generator().manual_seed(123)
    segs = []
    # 5 rows: an odd hotness makes the next segment start at an odd element
    for i, h in enumerate([1, 2, 3, 27, 100, 130]):
        vocab = VOCABS[i % 4]
        segs.append((_ids(g, vocab, (5,)), h,
                     (vocab, multi_hot_key(SEED, i)), 1000 * i + 7))
        segs.append((_ids(g, vocab, (5, h)), h, None, 31 * i + 1))
    segs.append((torch.arange(100, 140), 4, None, 0))  # an offset of zero
    for exp in (None, (7, 99)):                      # rows == 0
        segs.append((torch.empty(0, dtype=torch.int64), 3, exp, 5))
    # more segments than one launch holds
    for i in range(70):
        vocab = VOCABS[i % 4]
        if i % 3 == 0:
            segs.append((_ids(g, vocab, (3, 3)), 3, None, -i))
        else:
            segs.append((_ids(g, vocab, (3,)), 3,
                         (vocab, multi_hot_key(i, SEED)), i << 33))
    return segs


@requires_gpu
def test_pack_ids_matches_composition():
    from distributed_embeddings_amd.ops.embedding_lookup import (
        pack_ids, pack_ids_reference)
    segs = _segments()
    assert len(segs) > 64
    begins, pos = [], 0
    for src, h, exp, _ in segs:
        begins.append(pos)
        pos += src.numel() * (h if exp is not None else 1)
    assert any(b % 2 for b in begins) and any(b % 2 == 0 for b in begins[1:])
    want = pack_ids_reference(segs)
    assert want.numel() == pos

    def on_gpu(i, src):
        # every second source one element into its allocation: 8- but not
        # 16-byte aligned
        if i % 2 == 0 or src.numel() == 0:
            return src.cuda()
        padded = torch.cat([src.new_zeros(1), src.reshape(-1)]).cuda()
        assert padded[1:].data_ptr() % 16 == 8
        return padded[1:].view(src.shape)

    got = pack_ids([(on_gpu(i, src), h, exp, off)
                    for i, (src, h, exp, off) in enumerate(segs)])
    torch.cuda.synchronize()
    assert got.dtype == torch.int64 and got.shape == want.shape
    bad = (got.cpu() != want).nonzero().flatten()
    assert bad.numel() == 0, f"first mismatch at element {int(bad[0])}"


@requires_gpu
def test_pack_ids_empty_and_checks():
    from distributed_embeddings_amd.ops.embedding_lookup import pack_ids
    empty = torch.empty(0, dtype=torch.int64, device="cuda")
    out = pack_ids([(empty, 3, None, 1), (empty, 5, (7, 1), 2)])
    assert out.shape == (0,) and out.dtype == torch.int64 and out.is_cuda
    ok = torch.arange(6, device="cuda")
    with pytest.raises(RuntimeError):
        pack_ids([(ok.view(3, 2).t(), 1, None, 0)])          # not contiguous
    with pytest.raises(RuntimeError):
        pack_ids([(ok.int(), 1, None, 0)])                   # not int64
    with pytest.raises(RuntimeError):
        pack_ids([(ok, 1, None, 0), (ok.cpu(), 1, None, 0)])  # not on the GPU
    with pytest.raises(RuntimeError):
        pack_ids([(ok, 4, None, 0)])                         # no whole rows
    with pytest.raises(RuntimeError):
        pack_ids([(ok, 0, (7, 1), 0)])                       # h_out < 1


@requires_gpu
@pytest.mark.parametrize("vocab", [7, 40_000_000, 2**33 + 5])
def test_expand_gpu_equals_cpu(vocab):
    from distributed_embeddings_amd import multi_hot_expand
    g = torch.Generator().manual_seed(vocab % 1000)
    ids = _ids(g, vocab, (1000,))
    want = multi_hot_expand(ids, vocab, 100, SEED, 20)
    got = multi_hot_expand(ids.cuda(), vocab, 100, SEED, 20)
    assert got.is_cuda and got.shape == (1000, 100)
    assert torch.equal(got.cpu(), want)
    # any leading shape, and hotness 1 without a kernel
    got2 = multi_hot_expand(ids.view(10, 100).cuda(), vocab, 3, SEED, 20)
    assert torch.equal(got2.cpu(), want.view(10, 100, 100)[..., :3])
    one = multi_hot_expand(ids.cuda(), vocab, 1, SEED, 20)
    assert torch.equal(one.cpu(), ids[:, None])


# --- DistributedEmbedding with the kernel on and off -------------------------

def _train_two_steps(kind, monkeypatch, pack):
    """Two fused-SGD steps of a world-1 module: outputs, tables and the
    number of pack_ids launches."""
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.parallel import dist_embedding
    monkeypatch.setenv("DE_PACK_IDS", "1" if pack else "0")
    calls = []
    real = dist_embedding.pack_ids
    monkeypatch.setattr(dist_embedding, "pack_ids",
                        lambda segs: calls.append(len(segs)) or real(segs))
    rows = [300, 40, 100, 70]
    hot = [1, 2, 27, 5]
    gather = kind == "gather"           # tables without combiner, one-hot
    tables = [de.TableConfig(r, 32, None if gather else "sum") for r in rows]
    gw = torch.Generator().manual_seed(3)
    weights = [torch.randn(r, 32, generator=gw).numpy() for r in rows]
    with torch.device("cuda"):
        m = de.DistributedEmbedding(tables)
    m.set_weights(weights)
    m.enable_fused_sgd(0.05)
    gi = torch.Generator().manual_seed(5)
    b = 64
    one_hot = [torch.randint(0, r, (b,), generator=gi) for r in rows]
    if kind == "expand":
        m.set_multi_hot(hot, seed=SEED)
        inputs = one_hot
    elif kind == "bags":
        inputs = [de.multi_hot_expand(x, r, h, SEED, f)
                  for f, (x, r, h) in enumerate(zip(one_hot, rows, hot))]
    else:
        inputs = one_hot
    inputs = [x.cuda() for x in inputs]
    outs = []
    for step in range(2):
        if step == 0:
            out = torch.cat([o.reshape(b, -1) for o in m(inputs)], 1)
        else:
            assert m.packed_forward_available()
            packed, smaj = m.forward_packed(inputs)
            assert not smaj
            out = packed.transpose(0, 1).reshape(b, -1)
        out.square().sum().backward()
        outs.append(out.detach().clone())
    torch.cuda.synchronize()
    tabs = [torch.as_tensor(w) for w in m.get_weights()]
    assert any(not torch.equal(t, torch.as_tensor(w))
               for t, w in zip(tabs, weights)), "no update"
    return outs, tabs, calls


@requires_gpu
@pytest.mark.parametrize("kind", ["gather", "bags", "expand"])
def test_module_pack_ids_on_equals_off(kind, monkeypatch):
    outs1, tabs1, calls1 = _train_two_steps(kind, monkeypatch, True)
    outs0, tabs0, calls0 = _train_two_steps(kind, monkeypatch, False)
    # on: one launch of four segments per lookup; off: none from the module
    assert calls1 == [4, 4] and calls0 == []
    for a, b in zip(outs1 + tabs1, outs0 + tabs0):
        assert torch.equal(a, b)
    if kind == "expand":
        # and both equal the module fed the bags
        outs2, tabs2, _ = _train_two_steps("bags", monkeypatch, True)
        for a, b in zip(outs1 + tabs1, outs2 + tabs2):
            assert torch.equal(a, b)


# --- DLRM ---------------------------------------------------------------------

SIZES = [500, 37, 1200, 330, 64, 2000]
HOT = [1, 2, 3, 27, 1, 5]


def _dlrm(interaction):
    from distributed_embeddings_amd.models.dlrm import DLRM
    torch.manual_seed(0)
    return DLRM(SIZES, embedding_dim=32, bottom_mlp_dims=(64, 32),
                top_mlp_dims=(64, 1), num_numerical=13,
                interaction=interaction, cross_layers=3, cross_rank=16,
                multi_hot_sizes=HOT, multi_hot_seed=SEED)


def _batch(g, b):
    num = torch.rand(b, 13, generator=g)
    cats = [torch.randint(0, s, (b,), generator=g) for s in SIZES]
    labels = torch.randint(0, 2, (b, 1), generator=g).float()
    return num, cats, labels


@requires_gpu
@pytest.mark.parametrize("interaction", ["cross", "dot"])
def test_dlrm_gpu_bf16_vs_cpu_fp32(interaction):
    """bf16 autocast on the GPU against the fp32 CPU model, within the
    tolerance of the one-hot DLRM GPU comparisons (0.05 on the logits)."""
    ref = _dlrm(interaction)
    model = copy.deepcopy(ref).cuda()
    assert model._dot_perm is not None
    num, cats, labels = _batch(torch.Generator().manual_seed(51), 64)
    with torch.no_grad():
        want = ref(num, cats)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        logits = model(num.cuda(), [c.cuda() for c in cats])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            logits.float(), labels.cuda())
    err = float((logits.float().cpu() - want).abs().max())
    print(f"{interaction}: max |logit error| {err:.4e}, "
          f"max |logit| {float(want.abs().max()):.3f}")
    assert err < 0.05, err
    loss.backward()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        grad = p.grad.to_dense() if p.grad.is_sparse else p.grad
        assert bool(torch.isfinite(grad).all()), name


@requires_gpu
def test_dlrm_multi_hot_graph_capture():
    """A captured multi-hot train step (fused SGD on the tables, bf16
    autocast, lookup on the side stream), replayed with new one-hot ids in
    the static buffers, against the eager run of the same steps."""
    g = torch.Generator().manual_seed(61)
    batches = [_batch(g, 64) for _ in range(3)]
    models = [_dlrm("cross").cuda() for _ in range(2)]
    for m in models:
        m.embeddings.enable_fused_sgd(0.05)
    static = [t.cuda() if isinstance(t, torch.Tensor) else [c.cuda() for c in t]
              for t in batches[0]]

    def make_step(model, num, cats, labels):
        dense = [p for p in model.parameters()
                 if not any(p is q for q in model.embeddings.parameters())]

        def step():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = model(num, cats)
                loss = torch.nn.functional.binary_cross_entropy_with_logits(
                    logits.float(), labels)
            loss.backward()
            with torch.no_grad():
                for p in dense:
                    p.add_(p.grad, alpha=-0.05)
                    p.grad.zero_()
            return logits
        return step

    def load(batch):
        num, cats, labels = batch
        static[0].copy_(num)
        for dst, src in zip(static[1], cats):
            dst.copy_(src)
        static[2].copy_(labels)

    steps = [make_step(m, *static) for m in models]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            for step in steps:
                step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = steps[0]()
    for batch in batches[1:]:
        load(batch)
        graph.replay()
        eager = steps[1]()
    torch.cuda.synchronize()
    assert torch.allclose(captured.float(), eager.float(), atol=1e-3), \
        float((captured.float() - eager.float()).abs().max())
    for a, b in zip(models[0].embeddings.get_weights(),
                    models[1].embeddings.get_weights()):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        assert torch.allclose(a, b, atol=1e-3), float((a - b).abs().max())
    for (name, p), q in zip(models[0].named_parameters(),
                            models[1].parameters()):
        assert torch.allclose(p, q, atol=1e-3), name
