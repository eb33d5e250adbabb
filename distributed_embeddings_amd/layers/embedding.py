"""Embedding layers (single-GPU building blocks).

MI355X-native equivalents of the reference Keras layers in
``/root/reference/distributed_embeddings/python/layers/embedding.py``:

* :class:`Embedding`  — unified dense/ragged/sparse lookup + combiner
  (parity: ``embedding.py:50-170``).
* :class:`ConcatOneHotEmbedding` — all-one-hot tables fused into one variable
  with cumulative row offsets (parity: ``embedding.py:173-198``).
"""

import math
from typing import Callable, Optional, Union

import torch
from torch import nn

from ..ops.embedding_lookup import (Ragged, _csr_lookup_q8,
                                    check_per_id_weights,
                                    check_betas, csr_lookup_fused_optimizer,
                                    _check_bits, _check_packed,
                                    dequantize_rowwise_int4,
                                    dequantize_rowwise_int8, embedding_lookup,
                                    quantize_rowwise_int4,
                                    quantize_rowwise_int8,
                                    quantized_embedding_lookup, to_int64)


def _default_init(weight: torch.Tensor) -> None:
    # Matches the reference default keras 'uniform' initializer range.
    nn.init.uniform_(weight, -0.05, 0.05)


def scaled_uniform_init(weight: torch.Tensor) -> None:
    """DLRM-style uniform(-1/sqrt(rows), 1/sqrt(rows)) initializer.

    Parity: reference ``examples/dlrm/utils.py:27-41`` (DLRMInitializer).
    """
    bound = 1.0 / math.sqrt(weight.shape[0])
    nn.init.uniform_(weight, -bound, bound)


class Embedding(nn.Module):
    """An embedding lookup layer with optional row combiner.

    Args:
      input_dim: vocabulary size (number of rows).
      output_dim: embedding width (number of columns).
      combiner: ``None``, ``'sum'`` or ``'mean'``.  With a combiner, the
        hotness (last) dimension of the input is reduced away.
      initializer: callable applied to the weight at construction.
      dtype: parameter dtype (default fp32).

    Input/output shapes (parity: reference ``embedding.py:65-69``):
      * dense ``[d0, ..., dn]`` ids, no combiner -> ``[d0, ..., dn, output_dim]``
      * dense ``[d0, ..., dn, hotness]`` + combiner -> ``[d0, ..., dn, output_dim]``
      * ``Ragged`` (2-D CSR) + combiner -> ``[nrows, output_dim]``
      * ``torch.sparse_coo`` 2-D ids + combiner -> ``[nrows, output_dim]``

    Per-sample weights (with a combiner only): ``Ragged.weights``, or
    ``forward(ids, per_sample_weights)`` with the shape of dense ids.  Each row
    is scaled by its weight before the reduce; ``mean`` still divides by the
    number of ids in the bag, not by the weight sum.  Weights that require
    grad get one, in their own dtype, in every mode of the layer.

    Serving from int8: :meth:`quantize_` replaces the ``weight`` parameter by
    the buffer ``qweight`` (int8 row-wise packed, ``[input_dim,
    output_dim + 8]`` uint8, see ``quantize_rowwise_int8``);
    :meth:`from_quantized` builds such a layer from packed bytes.  A quantized
    layer serves every input kind, forward only: its outputs never require
    grad and it takes no optimizer.  ``bits=4`` on either selects int4
    row-wise storage instead (``[input_dim, output_dim / 2 + 4]`` uint8, see
    ``quantize_rowwise_int4``; ``output_dim`` a multiple of 8).
    """

    def __init__(
        self,
        input_dim: int,
        output_dim: int,
        combiner: Optional[str] = None,
        initializer: Optional[Callable[[torch.Tensor], None]] = None,
        dtype: torch.dtype = torch.float32,
        device=None,
        sparse_grad: bool = True,
    ):
        super().__init__()
        if input_dim <= 0 or output_dim <= 0:
            raise ValueError("input_dim and output_dim must be positive")
        if combiner not in (None, "sum", "mean"):
            raise ValueError(f"invalid combiner {combiner!r}")
        self.input_dim = int(input_dim)
        self.output_dim = int(output_dim)
        self.combiner = combiner
        # sparse_grad: plain-gather lookups route through the CSR kernel so the
        # weight grad is a coalesced sparse tensor (IndexedSlices contract) —
        # a dense grad for a 288 GB-class table is not an option.
        self.sparse_grad = sparse_grad
        self.weight = nn.Parameter(torch.empty(input_dim, output_dim, dtype=dtype, device=device))
        (initializer or _default_init)(self.weight)
        # Internal: row-slice shards tolerate out-of-range ids (contribute a
        # zero row) so only the owning shard is in-bounds — parity with the
        # reference's reliance on TF GPU OOB-gather-zeros
        # (dist_model_parallel.py:889-904).
        self._oob_zero = False
        self.quantized = False
        self.quantized_bits = None      # 8 or 4 once quantized

    def extra_repr(self) -> str:
        s = f"input_dim={self.input_dim}, output_dim={self.output_dim}, combiner={self.combiner}"
        return (s + f", quantized=int{self.quantized_bits}" if self.quantized
                else s)

    # -------------------------------------------- int8 / int4 row-wise serving

    def quantize_(self, chunk_rows: int = 1 << 20, bits: int = 8):
        """Converts the table in place to int8 (``bits=8``) or int4
        (``bits=4``) row-wise storage: registers the buffer ``qweight``,
        removes the ``weight`` parameter (its memory is released) and returns
        ``self``.  The table stays on its device — a CPU-offloaded table
        stays on the CPU.  One-way: load the weights first, then quantize,
        then serve; a second call with the same ``bits`` does nothing, one
        with different ``bits`` raises."""
        _check_bits(bits)
        if self.quantized:
            if bits != self.quantized_bits:
                raise RuntimeError(
                    f"the table is already quantized to "
                    f"int{self.quantized_bits}: it cannot be converted to "
                    f"int{bits}")
            return self
        if getattr(self, "_fused_lr", None) is not None:
            raise RuntimeError("a layer with a fused optimizer enabled "
                               "cannot be quantized: it is being trained")
        quantize = quantize_rowwise_int4 if bits == 4 else quantize_rowwise_int8
        packed = quantize(self.weight.detach(), chunk_rows)
        # a model-parallel shard stays shard-local
        packed.de_local = getattr(self.weight, "de_local", False)
        del self._parameters["weight"]
        self.register_buffer("qweight", packed)
        self.quantized = True
        self.quantized_bits = bits
        return self

    @classmethod
    def from_quantized(cls, packed: torch.Tensor,
                       combiner: Optional[str] = None,
                       bits: int = 8) -> "Embedding":
        """A quantized layer around int8 row-wise ``packed`` bytes
        (``[input_dim, output_dim + 8]`` uint8) or, with ``bits=4``, int4
        row-wise ones (``[input_dim, output_dim / 2 + 4]`` uint8); no fp32
        table is ever allocated."""
        if combiner not in (None, "sum", "mean"):
            raise ValueError(f"invalid combiner {combiner!r}")
        width = _check_packed(packed, bits)
        if packed.shape[0] <= 0:
            raise ValueError("packed must have at least one row")
        self = cls.__new__(cls)
        nn.Module.__init__(self)
        self.input_dim = int(packed.shape[0])
        self.output_dim = width
        self.combiner = combiner
        self.sparse_grad = True
        self._oob_zero = False
        self.register_buffer("qweight", packed.detach().contiguous())
        self.quantized = True
        self.quantized_bits = bits
        return self

    def dequantized_weight(self) -> torch.Tensor:
        """fp32 ``[input_dim, output_dim]`` values the quantized table
        stands for."""
        if not self.quantized:
            raise RuntimeError("dequantized_weight() needs a quantized layer")
        if self.quantized_bits == 4:
            return dequantize_rowwise_int4(self.qweight)
        return dequantize_rowwise_int8(self.qweight)

    def _quantized_forward(self, ids, per_sample_weights):
        if isinstance(ids, Ragged) or ids.layout == torch.sparse_coo:
            return quantized_embedding_lookup(self.qweight, ids, self.combiner,
                                              per_sample_weights,
                                              bits=self.quantized_bits)
        if self.combiner is None:
            return quantized_embedding_lookup(self.qweight, ids,
                                              bits=self.quantized_bits)
        if ids.dim() < 2:
            raise ValueError("ids with a combiner must have a hotness dimension "
                             "(parity: reference embedding.py:133-135)")
        if (per_sample_weights is not None
                and per_sample_weights.shape != ids.shape):
            raise ValueError(
                f"per_sample_weights shape {tuple(per_sample_weights.shape)} "
                f"does not match ids shape {tuple(ids.shape)}")
        h = ids.shape[-1]
        out = quantized_embedding_lookup(
            self.qweight, ids.reshape(-1, h), self.combiner,
            None if per_sample_weights is None
            else per_sample_weights.reshape(-1, h), bits=self.quantized_bits)
        return out.view(*ids.shape[:-1], self.output_dim)

    def _apply(self, fn, recurse=True):
        # CPU-offloaded tables are pinned: .to('cuda') / .cuda() on the parent
        # module must not move the weight (parity: reference builds offloaded
        # variables under tf.device('CPU:0'), dist_model_parallel.py:1186-1189).
        if getattr(self, "_cpu_offload", False):
            return self
        return super()._apply(fn, recurse)

    def enable_fused_sgd(self, lr: float):
        """In-backward SGD (see enable_fused_optimizer)."""
        return self.enable_fused_optimizer("sgd", lr)

    def enable_fused_optimizer(self, method: str, lr: float, eps: float = 1e-10,
                               stochastic_rounding: bool = False,
                               seed: Optional[int] = None,
                               betas=(0.9, 0.999)):
        """In-backward fused optimizer: the lookup's backward applies the
        update directly (no grad tensor, no host sync; the step becomes
        hipGraph-capturable).  The training optimizer must not also update
        this weight (its ``.grad`` stays ``None``).

        ``method`` is ``"sgd"``, ``"adagrad"`` (fp32 state
        ``[input_dim, output_dim]``), ``"rowwise_adagrad"`` (fp32 state
        ``[input_dim]``: one accumulator per row, fed with the mean square of
        the row's summed gradient) or ``"lazy_adam"``.  Calling it again
        replaces the state.

        ``"lazy_adam"`` is ``torch.optim.SparseAdam``'s update with ``betas``
        (each in ``[0, 1)``, else ``ValueError``): rows whose id occurs in
        the step get ``m = b1 m + (1 - b1) G``, ``v = b2 v + (1 - b2) G^2``
        and ``w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)`` on
        their summed gradient ``G``; all other rows keep ``w``, ``m`` and
        ``v`` bit for bit (no decay).  The moments are the fp32 buffer
        ``_fused_state`` ``[2, input_dim, output_dim]`` (``m`` first)
        whatever the table dtype: 8 bytes per table element.  ``t`` is the
        int64 buffer ``_fused_step`` ``[1]``; it counts the applied updates
        on the device and is part of ``state_dict``, so a resumed run
        continues at the right ``t``.  ``eps`` keeps its Adagrad default of
        ``1e-10``; Adam users normally pass ``1e-8``.

        ``stochastic_rounding`` (bf16 tables only; ``ValueError`` on fp32)
        stores the updated weights with stochastic instead of nearest-even
        rounding, so updates below half a bf16 ulp of the weight survive on
        average instead of being dropped (``ops.stochastic_round_bf16``).  It
        registers the int64 buffer ``_fused_sr = (seed, step)``; the step
        counts the applied updates on the device and the buffer is part of
        ``state_dict``, so a resumed run continues the bit stream.
        ``seed=None`` draws the seed from torch's default CPU generator
        (``torch.manual_seed`` makes runs repeatable)."""
        if method not in ("sgd", "adagrad", "rowwise_adagrad", "lazy_adam"):
            raise ValueError(f"unknown fused optimizer {method!r}")
        check_betas(betas)
        if self.quantized:
            raise RuntimeError(f"a quantized (int{self.quantized_bits}) table "
                               "is inference-only: it takes no optimizer")
        if stochastic_rounding and self.weight.dtype != torch.bfloat16:
            raise ValueError("stochastic_rounding needs a bf16 table: an "
                             f"{self.weight.dtype} table has nothing to round")
        # allow re-configuring
        for name in ("_fused_lr", "_fused_state", "_fused_sr", "_fused_step"):
            if name in self._buffers:
                del self._buffers[name]
        self.register_buffer("_fused_lr",
                             torch.tensor([float(lr)], dtype=torch.float32,
                                          device=self.weight.device))
        self._fused_method = method
        self._fused_eps = float(eps)
        self._fused_betas = (float(betas[0]), float(betas[1]))
        if method == "lazy_adam":
            self.register_buffer("_fused_state",
                                 torch.zeros((2,) + tuple(self.weight.shape),
                                             dtype=torch.float32,
                                             device=self.weight.device))
            self.register_buffer("_fused_step",
                                 torch.zeros(1, dtype=torch.int64,
                                             device=self.weight.device))
        elif method in ("adagrad", "rowwise_adagrad"):
            # fp32 state regardless of table storage dtype
            shape = (self.weight.shape if method == "adagrad"
                     else self.weight.shape[:1])
            self.register_buffer("_fused_state",
                                 torch.zeros(shape, dtype=torch.float32,
                                             device=self.weight.device))
        else:
            self.register_buffer("_fused_state",
                                 torch.empty(0, dtype=torch.float32,
                                             device=self.weight.device))
        # optimizer state is shard-local: never broadcast/allreduce it (the
        # weight itself carries de_local when model-parallel)
        self._fused_state.de_local = getattr(self.weight, "de_local", False)
        self._fused_lr.de_local = False  # lr is global; broadcasting is fine
        if method == "lazy_adam":
            self._fused_step.de_local = self._fused_state.de_local
        if stochastic_rounding:
            if seed is None:
                seed = int(torch.randint(0, 1 << 62, (1,)))
            self.register_buffer("_fused_sr",
                                 torch.tensor([to_int64(int(seed)), 0],
                                              dtype=torch.int64,
                                              device=self.weight.device))
            # the bit stream belongs to the shard, like the optimizer state
            self._fused_sr.de_local = self._fused_state.de_local
        return self

    def set_fused_lr(self, lr: float):
        if self.quantized:
            raise RuntimeError(f"a quantized (int{self.quantized_bits}) table "
                               "is inference-only: it takes no optimizer")
        if getattr(self, "_fused_lr", None) is None:
            raise RuntimeError("enable_fused_sgd() first")
        with torch.no_grad():
            self._fused_lr.fill_(float(lr))

    def csr_lookup(self, values: torch.Tensor, row_splits: torch.Tensor,
                   combiner: str, out_dtype=None,
                   per_id_w: Optional[torch.Tensor] = None) -> torch.Tensor:
        """CSR lookup through this layer (fused-SGD aware).

        ``out_dtype=torch.bfloat16`` makes the HIP kernel store bf16 directly
        (fp32 accumulation; backward consumes bf16 grads natively) — no
        separate cast kernel on the hot path.  ``per_id_w``: one floating
        weight per id (see ``Ragged.weights``)."""
        if per_id_w is not None:
            check_per_id_weights(per_id_w, values.numel())
            per_id_w = per_id_w.reshape(-1)
        if self.quantized:
            with torch.no_grad():
                return _csr_lookup_q8(self.qweight, values, row_splits,
                                      combiner, out_dtype, per_id_w,
                                      self.quantized_bits)
        if getattr(self, "_fused_lr", None) is not None and self.training:
            adam = None
            if self._fused_method == "lazy_adam":
                adam = (self._fused_step,) + self._fused_betas
            return csr_lookup_fused_optimizer(
                self.weight, values, row_splits, combiner, self._fused_lr,
                self._fused_state,
                self._fused_method in ("adagrad", "rowwise_adagrad"),
                self._fused_eps, out_dtype, per_id_w,
                getattr(self, "_fused_sr", None), adam)
        from ..ops.embedding_lookup import _CsrLookup
        return _CsrLookup.apply(self.weight, values, row_splits, combiner,
                                out_dtype, per_id_w)

    def get_config(self) -> dict:
        """Planner-facing config (reference uses keras ``get_config()``)."""
        return {
            "input_dim": self.input_dim,
            "output_dim": self.output_dim,
            "combiner": self.combiner,
        }

    def _gather(self, ids: torch.Tensor) -> torch.Tensor:
        flat = ids.reshape(-1)
        if self.sparse_grad and (self.weight.requires_grad or self._oob_zero):
            # hotness-1 CSR: same gather, sparse (IndexedSlices-style) grad,
            # OOB ids contribute zero rows.
            splits = torch.arange(flat.numel() + 1, device=flat.device, dtype=torch.long)
            out = self.csr_lookup(flat, splits, "sum")
        elif self._oob_zero:
            valid = (flat >= 0) & (flat < self.input_dim)
            safe = torch.where(valid, flat, torch.zeros_like(flat))
            out = self.weight.index_select(0, safe)
            out = out * valid.unsqueeze(1).to(out.dtype)
        else:
            out = self.weight.index_select(0, flat)
        return out.view(*ids.shape, self.output_dim)

    def forward(self, ids: Union[torch.Tensor, Ragged],
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.quantized:
            return self._quantized_forward(ids, per_sample_weights)
        if isinstance(ids, Ragged):
            if self.combiner is None:
                raise ValueError("Ragged input requires a combiner")
            if ids.weights is not None and per_sample_weights is not None:
                raise ValueError("give the weights either as Ragged.weights "
                                 "or as per_sample_weights, not both")
            w = ids.weights if ids.weights is not None else per_sample_weights
            return self.csr_lookup(ids.values.long(), ids.row_splits.long(),
                                    self.combiner, per_id_w=w)

        if per_sample_weights is not None and self.combiner is None:
            raise ValueError("per_sample_weights require a combiner")

        if ids.layout == torch.sparse_coo:
            if self.combiner is None:
                raise ValueError("Sparse input requires a combiner")
            return embedding_lookup(self.weight, ids, self.combiner,
                                    per_sample_weights)

        if ids.dtype != torch.long:
            # parity: reference casts non-int inputs (embedding.py:121-123)
            ids = ids.long()

        if self.combiner is None:
            return self._gather(ids)

        if ids.dim() < 2:
            raise ValueError("ids with a combiner must have a hotness dimension "
                             "(parity: reference embedding.py:133-135)")
        lead_shape = ids.shape[:-1]
        flat2d = ids.reshape(-1, ids.shape[-1])
        if per_sample_weights is not None:
            # weighted: always the CSR path (fused-optimizer aware), with the
            # weights reshaped alongside N-D ids
            if per_sample_weights.shape != ids.shape:
                raise ValueError(
                    f"per_sample_weights shape {tuple(per_sample_weights.shape)} "
                    f"does not match ids shape {tuple(ids.shape)}")
            b, h = flat2d.shape
            splits = torch.arange(b + 1, device=flat2d.device,
                                  dtype=torch.long) * h
            out = self.csr_lookup(flat2d.reshape(-1), splits, self.combiner,
                                  per_id_w=per_sample_weights.reshape(-1))
        elif getattr(self, "_fused_lr", None) is not None and self.training:
            # fused in-backward optimizer: dense [b, h] as CSR so the update
            # applies here too (not only for Ragged inputs)
            b, h = flat2d.shape
            splits = torch.arange(b + 1, device=flat2d.device,
                                  dtype=torch.long) * h
            out = self.csr_lookup(flat2d.reshape(-1), splits, self.combiner)
        elif self._oob_zero or flat2d.shape[1] > 1:
            out = embedding_lookup(self.weight, flat2d, self.combiner)
        else:
            out = self._gather(flat2d.reshape(-1))
        return out.view(*lead_shape, self.output_dim)


class ConcatOneHotEmbedding(nn.Module):
    """Multiple one-hot (hotness-1) tables fused into a single variable.

    Inputs of shape ``[batch, num_tables]`` are offset by per-table cumulative
    row starts and looked up with a single gather.
    Parity: reference ``embedding.py:173-198``.
    """

    def __init__(self, table_sizes, output_dim, initializer=None, dtype=torch.float32,
                 device=None):
        super().__init__()
        self.table_sizes = [int(s) for s in table_sizes]
        self.output_dim = int(output_dim)
        total = sum(self.table_sizes)
        self.weight = nn.Parameter(torch.empty(total, output_dim, dtype=dtype, device=device))
        (initializer or _default_init)(self.weight)
        offsets = torch.cumsum(torch.tensor([0] + self.table_sizes[:-1], dtype=torch.long), 0)
        self.register_buffer("offsets", offsets)

    def forward(self, ids: torch.Tensor) -> torch.Tensor:
        if ids.dim() != 2 or ids.shape[1] != len(self.table_sizes):
            raise ValueError(
                f"expected ids [batch, {len(self.table_sizes)}], got {tuple(ids.shape)}")
        shifted = ids.long() + self.offsets.unsqueeze(0)
        return self.weight.index_select(0, shifted.reshape(-1)).view(
            ids.shape[0], len(self.table_sizes), self.output_dim)
