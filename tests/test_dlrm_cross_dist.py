"""DLRM(interaction="cross") distributed equivalence (gloo world=2): the
hybrid dp+mp path of ``tests/test_dlrm_dist.py`` with the low-rank cross
network between the concatenated features and the top MLP."""

import pytest
import torch

from conftest import run_distributed

SIZES = [50, 7, 120, 33, 64, 200]


def _dlrm_cross_worker(rank, world, fused_sgd):
    import distributed_embeddings_amd as de
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer

    torch.manual_seed(0)
    model = DLRM(SIZES, embedding_dim=16, bottom_mlp_dims=(32, 16),
                 top_mlp_dims=(32, 1), num_numerical=4,
                 strategy="memory_balanced", interaction="cross",
                 cross_layers=2, cross_rank=4)
    # deterministic weights everywhere
    gw = torch.Generator().manual_seed(42)
    weights = [torch.randn(s, 16, generator=gw).numpy() for s in SIZES]
    model.embeddings.set_weights(weights)
    for p in model.bottom_mlp.parameters():
        torch.nn.init.normal_(p, generator=gw) if p.dim() > 1 else p.data.zero_()
    for p in model.top_mlp.parameters():
        torch.nn.init.normal_(p, std=0.1, generator=gw) if p.dim() > 1 \
            else p.data.zero_()
    for p in model.cross.parameters():
        torch.nn.init.normal_(p, std=0.1, generator=gw)
    de.broadcast_parameters(model)

    if fused_sgd:
        model.embeddings.enable_fused_sgd(0.05)
    opt = de.DistributedOptimizer(
        SparseEmbeddingOptimizer(model.parameters(), lr=0.05), average=False)

    gi = torch.Generator().manual_seed(7)
    B = 8
    cats = [torch.randint(0, s, (B,), generator=gi) for s in SIZES]
    num = torch.rand(B, 4, generator=gi)
    labels = torch.randint(0, 2, (B, 1), generator=gi).float()
    lb = B // world
    sl = slice(rank * lb, (rank + 1) * lb)

    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        logits = model(num[sl], [c[sl] for c in cats])
        loss = torch.nn.functional.binary_cross_entropy_with_logits(
            logits.float(), labels[sl], reduction="sum") / B
        loss.backward()
        opt.step()
    out = model(num[sl], [c[sl] for c in cats]).detach()
    tables = model.embeddings.get_weights(all_ranks=True)
    dense = {n: p.detach().clone() for n, p in model.named_parameters()
             if not n.startswith("embeddings.")}
    return {"out": out, "tables": [torch.as_tensor(t) for t in tables],
            "dense": dense}


@pytest.mark.parametrize("fused_sgd", [False, True])
def test_dlrm_cross_world2_matches_world1(fused_sgd):
    results2 = run_distributed(_dlrm_cross_worker, world=2, args=(fused_sgd,))
    results1 = run_distributed(_dlrm_cross_worker, world=1, args=(fused_sgd,))
    full_out = results1[0]["out"]
    for rank in range(2):
        got = results2[rank]["out"]
        ref = full_out[rank * 4:(rank + 1) * 4]
        assert torch.allclose(got, ref, atol=1e-4), \
            f"rank{rank} fwd err {(got - ref).abs().max()}"
    for t in range(len(SIZES)):
        a = results2[0]["tables"][t]
        b = results1[0]["tables"][t]
        assert torch.allclose(a, b, atol=1e-4), \
            f"table {t} err {(a - b).abs().max()}"
    dense1 = results1[0]["dense"]
    assert any(n.startswith("cross.v.") for n in dense1)
    assert any(n.startswith("cross.w.") for n in dense1)
    for rank in range(2):
        for name, ref in dense1.items():
            got = results2[rank]["dense"][name]
            assert torch.allclose(got, ref, atol=1e-4), \
                f"rank{rank} {name} err {(got - ref).abs().max()}"
