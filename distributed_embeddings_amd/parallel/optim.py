"""Optimizers with fused O(nnz) sparse embedding updates.

The lookup backward emits coalesced ``(unique_ids, unique_grad)`` sparse COO
gradients (the IndexedSlices contract).  Stock torch optimizers re-coalesce
every sparse grad (a device-wide merge sort + segmented add per step); the
fused path here applies the rows directly with one HIP kernel
(``sparse_row_update`` in ``csrc/embedding_ops.hip``).

``SparseEmbeddingOptimizer`` handles both sparse-grad embedding tables and
dense-grad params (MLP weights) in one optimizer; it is the MI355X analog of
the reference examples' per-variable optimizer usage (SGD in
``examples/dlrm/utils.py:45-88``, Adagrad in
``examples/benchmarks/synthetic_models/main.py``).
"""

import torch

from ..ops import _backend
from ..ops.embedding_lookup import _write_rows_sr, mix64_int, to_int64


class SparseEmbeddingOptimizer(torch.optim.Optimizer):
    """SGD / Adagrad / row-wise Adagrad with fused sparse row updates.

    Args:
      params: iterable of parameters (dense and sparse-grad mixed).
      lr: learning rate.
      method: ``"sgd"``, ``"adagrad"`` or ``"rowwise_adagrad"``.  Row-wise
        Adagrad keeps one fp32 accumulator per row of a sparse-grad param
        (state ``[vocab]``), fed with the mean square of the row's gradient.
        Dense-grad params in the same optimizer keep element-wise Adagrad.
      eps: adagrad epsilon.
      assume_coalesced: trust that every sparse grad holds unique, sorted ids
        (true when each embedding parameter receives exactly one lookup
        backward per step — the fused-group design guarantees it).  Set False
        if a table is looked up multiple times per step outside the fused
        path.
      stochastic_rounding: store the updated rows of **bf16 sparse-grad**
        params with stochastic instead of nearest-even rounding
        (``ops.stochastic_round_bf16``), so updates below half a bf16 ulp of
        the weight survive on average.  fp32 and dense-grad params are not
        affected (one optimizer holds both kinds, so this is no error).
      seed: base seed of the rounding bits; ``None`` draws one from torch's
        default CPU generator.  Param ``i`` (in param-group order) rounds
        with ``mix64(mix64(seed) ^ i)`` and its own step counter, kept as the
        int64 ``[2]`` device tensor ``state[p]["sr"] = (seed, step)``, which
        ``state_dict()`` / ``load_state_dict()`` carry over.
    """

    def __init__(self, params, lr: float = 0.01, method: str = "sgd",
                 eps: float = 1e-10, assume_coalesced: bool = True,
                 stochastic_rounding: bool = False, seed=None):
        if method not in ("sgd", "adagrad", "rowwise_adagrad"):
            raise ValueError(f"unknown method {method!r}")
        if stochastic_rounding and seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)))
        defaults = dict(lr=lr, method=method, eps=eps,
                        assume_coalesced=assume_coalesced,
                        stochastic_rounding=bool(stochastic_rounding),
                        seed=None if seed is None else int(seed))
        super().__init__(params, defaults)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        # torch casts every state tensor to its param's dtype, which would
        # turn the int64 (seed, step) pairs into bf16: take them from the
        # source again
        ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        params = [p for g in self.param_groups for p in g["params"]]
        for i, p in zip(ids, params):
            sr = state_dict["state"].get(i, {}).get("sr")
            if sr is not None:
                self.state[p]["sr"] = sr.detach().to(
                    device=p.device, dtype=torch.int64).clone()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr = group["lr"]
            eps = group["eps"]
            adagrad = group["method"] != "sgd"
            rowwise = group["method"] == "rowwise_adagrad"
            dense = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.layout == torch.sparse_coo:
                    sr = None
                    if (group.get("stochastic_rounding", False)
                            and p.dtype == torch.bfloat16):
                        sr = self._sr_for(p, group["seed"])
                    self._sparse_update(p, g, lr, eps, adagrad, rowwise,
                                        group["assume_coalesced"], sr)
                else:
                    dense.append(p)
            if dense:
                self._dense_update_batch(dense, lr, eps, adagrad)
        return loss

    def _state_for(self, p, rowwise=False):
        st = self.state[p]
        if "sum" not in st:
            # fp32 accumulator state regardless of param storage dtype
            st["sum"] = torch.zeros(p.shape[:1] if rowwise else p.shape,
                                    dtype=torch.float32, device=p.device)
        return st["sum"]

    def _sr_for(self, p, seed):
        st = self.state[p]
        if "sr" not in st:
            index = [id(q) for grp in self.param_groups
                     for q in grp["params"]].index(id(p))
            own = to_int64(mix64_int(mix64_int(int(seed)) ^ index))
            st["sr"] = torch.tensor([own, 0], dtype=torch.int64,
                                    device=p.device)
        return st["sr"]

    def _sparse_update(self, p, g, lr, eps, adagrad, rowwise,
                       assume_coalesced, sr=None):
        if not (assume_coalesced or g.is_coalesced()):
            g = g.coalesce()
        ids = g._indices()[0]
        vals = g._values().float()
        if p.is_cuda:
            # the kernel reads the mode off the state: [vocab] is row-wise
            state = (self._state_for(p, rowwise) if adagrad
                     else torch.empty(0))
            _backend.ops().sparse_row_update(p.data, state, ids.contiguous(),
                                             vals.contiguous(), lr, eps,
                                             adagrad, sr)
        else:
            if adagrad:
                state = self._state_for(p, rowwise)
                sq = vals * vals
                state.index_add_(0, ids, sq.mean(dim=1) if rowwise else sq)
                denom = state.index_select(0, ids).sqrt_().add_(eps)
                if rowwise:
                    denom = denom.unsqueeze(1)
                delta = -lr * vals / denom
            else:
                delta = -lr * vals
            if sr is None:
                p.data.index_add_(0, ids, delta.to(p.dtype))
            elif ids.numel() > 0:
                # unique ids (the sparse-grad contract): read, add, round
                rows = p.data.index_select(0, ids).float() + delta
                _write_rows_sr(p.data, ids, rows, sr)

    def _dense_update_batch(self, params, lr, eps, adagrad):
        """foreach-batched dense updates (one fused launch set per step)."""
        grads = [p.grad for p in params]
        if adagrad:
            states = [self._state_for(p) for p in params]
            torch._foreach_addcmul_(states, grads, grads, value=1.0)
            denoms = torch._foreach_sqrt(states)
            torch._foreach_add_(denoms, eps)
            torch._foreach_addcdiv_([p.data for p in params], grads, denoms,
                                    value=-lr)
        else:
            torch._foreach_add_([p.data for p in params], grads, alpha=-lr)
