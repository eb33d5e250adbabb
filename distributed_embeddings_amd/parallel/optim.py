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
from ..ops.embedding_lookup import (_lazy_adam_rows, _write_rows_sr,
                                    check_betas, mix64_int, to_int64)


class SparseEmbeddingOptimizer(torch.optim.Optimizer):
    """SGD / Adagrad / row-wise Adagrad / lazy Adam with fused sparse row
    updates.

    Args:
      params: iterable of parameters (dense and sparse-grad mixed).
      lr: learning rate.
      method: ``"sgd"``, ``"adagrad"``, ``"rowwise_adagrad"`` or
        ``"lazy_adam"``.  Row-wise
        Adagrad keeps one fp32 accumulator per row of a sparse-grad param
        (state ``[vocab]``), fed with the mean square of the row's gradient.
        Dense-grad params in the same optimizer keep element-wise Adagrad.
        Lazy Adam is ``torch.optim.SparseAdam``'s update: the rows of a
        sparse grad get ``m = b1 m + (1 - b1) g``, ``v = b2 v + (1 - b2)
        g^2`` and ``w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) +
        eps)``, all other rows keep ``w``, ``m`` and ``v`` (no decay).  The
        moments are one fp32 tensor ``state[p]["exp_avgs"]`` of shape
        ``[2, *p.shape]``, ``exp_avg`` first, and ``state[p]["step"]`` a
        host int.  Dense-grad params take the same formula over all their
        elements; their ``state[p]["step"]`` is a 0-dim float64 tensor on
        the param's device, so a hipGraph-captured ``step()`` takes a new
        ``t`` on every replay.
      eps: adagrad / adam epsilon (Adam users normally pass ``1e-8``).
      betas: lazy Adam's ``(b1, b2)``, each in ``[0, 1)``.
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
                 stochastic_rounding: bool = False, seed=None,
                 betas=(0.9, 0.999)):
        if method not in ("sgd", "adagrad", "rowwise_adagrad", "lazy_adam"):
            raise ValueError(f"unknown method {method!r}")
        check_betas(betas)
        if stochastic_rounding and seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)))
        defaults = dict(lr=lr, method=method, eps=eps,
                        assume_coalesced=assume_coalesced,
                        stochastic_rounding=bool(stochastic_rounding),
                        seed=None if seed is None else int(seed),
                        betas=(float(betas[0]), float(betas[1])))
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
            # ... and the fp32 moments of a bf16 param into bf16
            mom = state_dict["state"].get(i, {}).get("exp_avgs")
            if mom is not None:
                self.state[p]["exp_avgs"] = mom.detach().to(
                    device=p.device, dtype=torch.float32).clone()
            # a dense-grad param counts its Adam steps on its device
            step = state_dict["state"].get(i, {}).get("step")
            if isinstance(step, torch.Tensor):
                self.state[p]["step"] = step.detach().to(
                    device=p.device, dtype=torch.float64).clone()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            lr = group["lr"]
            eps = group["eps"]
            adagrad = group["method"] in ("adagrad", "rowwise_adagrad")
            rowwise = group["method"] == "rowwise_adagrad"
            adam = group["method"] == "lazy_adam"
            betas = group.get("betas", (0.9, 0.999))
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
                    if adam:
                        self._sparse_adam(p, g, lr, eps, betas,
                                          group["assume_coalesced"], sr)
                        continue
                    self._sparse_update(p, g, lr, eps, adagrad, rowwise,
                                        group["assume_coalesced"], sr)
                else:
                    dense.append(p)
            if dense and adam:
                self._dense_adam_batch(dense, lr, eps, betas)
            elif dense:
                self._dense_update_batch(dense, lr, eps, adagrad)
        return loss

    def _state_for(self, p, rowwise=False):
        st = self.state[p]
        if "sum" not in st:
            # fp32 accumulator state regardless of param storage dtype
            st["sum"] = torch.zeros(p.shape[:1] if rowwise else p.shape,
                                    dtype=torch.float32, device=p.device)
        return st["sum"]

    def _adam_state_for(self, p, device_step=False):
        """(moments [2, *p.shape] fp32, the step counter before this
        update): a host int, or with device_step a 0-dim float64 tensor."""
        st = self.state[p]
        if "exp_avgs" not in st:
            st["exp_avgs"] = torch.zeros((2,) + tuple(p.shape),
                                         dtype=torch.float32, device=p.device)
            st["step"] = (torch.zeros((), dtype=torch.float64, device=p.device)
                          if device_step else 0)
        return st["exp_avgs"], st["step"]

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

    def _sparse_adam(self, p, g, lr, eps, betas, assume_coalesced, sr=None):
        if not (assume_coalesced or g.is_coalesced()):
            g = g.coalesce()
        ids = g._indices()[0]
        vals = g._values().float()
        if ids.numel() == 0:
            return  # nothing applied: t stays, like the fused path's
        state, t = self._adam_state_for(p)
        t = self.state[p]["step"] = int(t) + 1
        if p.is_cuda:
            _backend.ops().sparse_row_update(
                p.data, state, ids.contiguous(), vals.contiguous(), lr, eps,
                False, sr, adam_step=t, beta1=betas[0], beta2=betas[1])
            return
        delta = _lazy_adam_rows(state, ids, vals, lr, betas[0], betas[1], eps,
                                t)
        if sr is None:
            p.data.index_add_(0, ids, delta.to(p.dtype))
        else:
            rows = p.data.index_select(0, ids).float() + delta
            _write_rows_sr(p.data, ids, rows, sr)

    def _dense_adam_batch(self, params, lr, eps, betas):
        """The lazy-Adam formula over every element, foreach-batched.  The
        steps are device tensors and a_t is formed from them on the device
        (in float64), so the whole update can be graph-captured."""
        b1, b2 = betas
        grads = [p.grad.float() for p in params]
        ms, vs, steps = [], [], []
        for p in params:
            state, step = self._adam_state_for(p, device_step=True)
            ms.append(state[0])
            vs.append(state[1])
            steps.append(step)
        torch._foreach_add_(steps, 1)
        neg_a = [((1.0 - b2 ** t).sqrt_() / (1.0 - b1 ** t)).mul_(-lr).float()
                 for t in steps]
        torch._foreach_mul_(ms, b1)
        torch._foreach_add_(ms, grads, alpha=1.0 - b1)
        torch._foreach_mul_(vs, b2)
        torch._foreach_addcmul_(vs, grads, grads, value=1.0 - b2)
        denoms = torch._foreach_sqrt(vs)
        torch._foreach_add_(denoms, eps)
        updates = torch._foreach_div(ms, denoms)
        updates = [u.mul_(a) for u, a in zip(updates, neg_a)]
        torch._foreach_add_([p.data for p in params],
                            [u.to(p.dtype) for p, u in zip(params, updates)])

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
