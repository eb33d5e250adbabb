"""DistributedEmbedding — hybrid data+model parallel embedding execution.

MI355X-native re-design of the reference wrapper
(``/root/reference/distributed_embeddings/python/layers/dist_model_parallel.py:712-1214``).
One process per GPU, ``torch.distributed`` collectives (RCCL over xGMI on GPU,
gloo on CPU), all four parallelism modes of the reference coexisting in one
module:

* data-parallel small tables (local call, grads allreduced by
  :class:`~distributed_embeddings_amd.parallel.grad.DistributedOptimizer`),
* table-parallel / column-sliced tables (dp->mp id all-to-all, fused local
  lookups, mp->dp output all-to-all; parity ``:842-887`` + ``:169-288``),
* row-sliced tables (allgather ids -> offset local lookup with OOB->zero ->
  unscaled reduce-scatter; parity ``:889-904``),
* CPU offload of the largest tables (parity ``:449-476``).

Key MI355X departures from the reference:

* The concat-fusion groups are not an XLA hint — each fused group executes as
  **one** kernel call over a single CSR batch (ids offset into the fused
  variable), so a DLRM-style model with N same-width tables does one lookup
  kernel + two all-to-alls per step regardless of N.
* All-to-alls are single fused ``all_to_all_single`` calls with per-peer
  splits — on the 8-GPU xGMI full mesh every peer pair has a dedicated link,
  so one grouped call saturates all 7 links at once.
"""

from typing import List, Optional, Sequence, Union

import numpy as np
import torch
from torch import nn

from ..layers.embedding import Embedding
from ..ops import _backend
from ..ops.embedding_lookup import (Ragged, embedding_lookup, mix64_int,
                                    multi_hot_expand_keyed, multi_hot_key,
                                    pack_ids, pack_ids_enabled,
                                    quantized_embedding_lookup, to_int64)
from . import comm
from .strategy import DistEmbeddingStrategy, TableConfig



def _cat_or_view(parts):
    """torch.cat that returns a zero-copy flat view when the parts are
    already adjacent slices of ONE storage (the world==1 / post-a2a layout)."""
    if len(parts) == 1:
        return parts[0].reshape(-1)
    base = parts[0]
    try:
        storage = base.untyped_storage()
        sptr = storage.data_ptr()
        off = base.storage_offset()
        total = 0
        for p in parts:
            if (p.untyped_storage().data_ptr() != sptr
                    or not p.is_contiguous()
                    or p.storage_offset() != off + total):
                raise StopIteration
            total += p.numel()
        return torch.empty(0, dtype=base.dtype, device=base.device).set_(
            storage, off, (total,), (1,))
    except StopIteration:
        return torch.cat([q.reshape(-1) for q in parts])


def _layer_to_config(layer) -> TableConfig:
    if isinstance(layer, Embedding):
        return TableConfig(layer.input_dim, layer.output_dim, layer.combiner)
    if isinstance(layer, nn.Embedding):
        return TableConfig(layer.num_embeddings, layer.embedding_dim, None)
    if isinstance(layer, TableConfig):
        return layer
    if isinstance(layer, dict):
        # tolerate stock-Keras config keys (parity: reference from_config
        # drops mask_zero/input_length, embedding.py:163-170)
        import dataclasses
        fields = {f.name for f in dataclasses.fields(TableConfig)}
        return TableConfig(**{k: v for k, v in layer.items() if k in fields})
    # custom user layers, duck-typed via get_config() or attributes (parity:
    # reference accepts any layer whose get_config() yields
    # input_dim/output_dim — dist_model_parallel_test.py:50-68, 501-511)
    if hasattr(layer, "get_config"):
        cfg = layer.get_config()
        if isinstance(cfg, dict) and "input_dim" in cfg and "output_dim" in cfg:
            return TableConfig(int(cfg["input_dim"]), int(cfg["output_dim"]),
                               cfg.get("combiner"))
    if hasattr(layer, "input_dim") and hasattr(layer, "output_dim"):
        return TableConfig(int(layer.input_dim), int(layer.output_dim),
                           getattr(layer, "combiner", None))
    raise TypeError(f"unsupported layer/config type {type(layer)}")


def _layer_weight(obj, rows, cols):
    """The handed-in layer's weight, if it looks like an embedding table."""
    w = getattr(obj, "weight", None)
    if isinstance(w, torch.Tensor) and tuple(w.shape) == (rows, cols):
        return w
    return None


def _offloaded_lookup(layer, ragged, combiner):
    """Lookup from a CPU-offloaded table, quantized or not."""
    if layer.quantized:
        return quantized_embedding_lookup(layer.qweight, ragged, combiner,
                                          bits=layer.quantized_bits)
    return embedding_lookup(layer.weight, ragged, combiner)


class DistributedEmbedding(nn.Module):
    """Shards a list of embedding tables across all ranks of the default group.

    Args:
      embeddings: list of :class:`Embedding` / ``nn.Embedding`` layers, or
        :class:`TableConfig`/dicts.
      strategy: placement strategy (``basic|memory_balanced|memory_optimized``).
      column_slice_threshold / row_slice_threshold / data_parallel_threshold /
        gpu_embedding_size: see :class:`DistEmbeddingStrategy`.
      dp_input: if True (default) inputs are data-parallel (each rank passes
        its local batch for every feature).  If False, inputs are
        model-parallel: each rank passes global-batch ids for the features in
        ``self.local_input_ids()`` only (parity: reference ``dp_input`` arg).
      input_table_map: optional input->table map for shared embeddings.

    Weighted lookups: an input may be a ``Ragged`` with ``weights`` (one
    floating weight per id); every parallelism mode carries them to the
    lookup.  Weights are data here: a weights tensor that requires grad is
    rejected (a single-table :class:`Embedding` does give weight gradients).

    Multi-hot expansion: after :meth:`set_multi_hot` a dense one-hot input is
    expanded on the device into a bag of ids that its table's combiner sums.
    """

    def __init__(
        self,
        embeddings: Sequence,
        strategy: str = "basic",
        column_slice_threshold: Optional[int] = None,
        row_slice_threshold: Optional[int] = None,
        data_parallel_threshold: Optional[int] = None,
        gpu_embedding_size: Optional[int] = None,
        dp_input: bool = True,
        input_table_map: Optional[Sequence[int]] = None,
        table_dtype: torch.dtype = torch.float32,
    ):
        super().__init__()
        if table_dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("table_dtype must be float32 or bfloat16")
        self.table_dtype = table_dtype
        self.world_size = comm.world_size()
        self.rank = comm.rank()
        self.dp_input = dp_input
        configs = [_layer_to_config(e) for e in embeddings]

        self.strategy = DistEmbeddingStrategy(
            configs,
            self.world_size,
            strategy=strategy,
            input_table_map=input_table_map,
            column_slice_threshold=column_slice_threshold,
            row_slice_threshold=row_slice_threshold,
            data_parallel_threshold=data_parallel_threshold,
            gpu_embedding_size=gpu_embedding_size,
        )
        self._built = False
        self._local_batch = None
        self.quantized = False
        self._mh_hotness = None  # set_multi_hot: hotness per input
        self._mh_seed = 0
        self._mh_pair = None     # per local pair: (h, vocab, key_f) or None

        plan = self.strategy
        # ---- data-parallel layers (replicated; grads allreduced) ----
        self.dp_layers = nn.ModuleList([
            Embedding(configs[t].input_dim, configs[t].output_dim, configs[t].combiner,
                      initializer=configs[t].initializer, dtype=table_dtype)
            for t in plan.dp_table_ids
        ])
        # Preserve weights of layer instances handed to us (PyTorch modules
        # have materialized weights at construction, unlike unbuilt Keras
        # layers — same contract as the col-group copy below).
        with torch.no_grad():
            for local_t, t in enumerate(plan.dp_table_ids):
                w = _layer_weight(embeddings[t], configs[t].input_dim,
                                  configs[t].output_dim)
                if w is not None:
                    self.dp_layers[local_t].weight.copy_(w)

        # ---- column/table-parallel fused variables ----
        # The fused group runs at EVERY world size (world==1 included): one
        # lookup kernel + one backward pipeline per group per step, instead of
        # one per table — the single biggest launch/sync saving for
        # many-table models (MI355X departure from the reference's
        # XLA-fusion hint, dist_model_parallel.py:650).
        col_layers = []
        for grp in plan.local_concat_groups(self.rank):
            # offloaded tables are built ON CPU and pinned there (the explicit
            # device= overrides any enclosing torch.device('cuda') context;
            # Embedding._apply then refuses later moves).
            lyr = Embedding(grp.input_dim, grp.output_dim, grp.combiner,
                            dtype=table_dtype,
                            device="cpu" if grp.cpu_offload else None)
            for p in lyr.parameters():
                if self.world_size > 1:
                    p.de_local = True  # model-parallel: excluded from grad allreduce
            if grp.cpu_offload:
                lyr._cpu_offload = True
            # apply per-member initializers (or copy weights handed to us)
            with torch.no_grad():
                for m in grp.members:
                    cfg = configs[m.table_id]
                    dst = lyr.weight[m.concat_row_offset:
                                     m.concat_row_offset + cfg.input_dim]
                    src_w = _layer_weight(embeddings[m.table_id],
                                          cfg.input_dim, cfg.output_dim)
                    if src_w is not None:
                        dst.copy_(src_w[:, m.col_offset:
                                        m.col_offset + m.width])
                    elif cfg.initializer is not None:
                        if m.width == cfg.output_dim:
                            if dst.dtype == torch.float32:
                                cfg.initializer(dst)
                            else:
                                tmp = torch.empty(dst.shape, dtype=torch.float32,
                                                  device=dst.device)
                                cfg.initializer(tmp)
                                dst.copy_(tmp)
                        else:
                            full = torch.empty(cfg.input_dim, cfg.output_dim,
                                               dtype=dst.dtype, device=dst.device)
                            cfg.initializer(full)
                            dst.copy_(full[:, m.col_offset:m.col_offset + m.width])
            col_layers.append(lyr)
        self.col_layers = nn.ModuleList(col_layers)

        # ---- row-sliced shards ----
        row_layers = []
        for shard in plan.local_row_shards(self.rank):
            cfg = configs[shard.table_id]
            lyr = Embedding(max(shard.rows, 1), cfg.output_dim, cfg.combiner,
                            dtype=table_dtype)
            lyr._oob_zero = True
            for p in lyr.parameters():
                p.de_local = True
            src_w = _layer_weight(embeddings[shard.table_id], cfg.input_dim,
                                  cfg.output_dim)
            if src_w is not None and shard.rows > 0:
                with torch.no_grad():
                    lyr.weight[:shard.rows].copy_(
                        src_w[shard.row_offset:shard.row_offset + shard.rows])
            row_layers.append(lyr)
        self.row_layers = nn.ModuleList(row_layers)

        # Per local (input, slice) pair: hotness discovered at first call;
        # row offsets into the fused variable are static.
        my_slices = plan.rank_input_slices[self.rank]
        self._pair_group = [s.concat_group for s in my_slices]
        self._pair_row_offset = [s.concat_row_offset for s in my_slices]
        self._pair_width = [s.width for s in my_slices]

    # ------------------------------------------------------------------ utils

    def enable_fused_sgd(self, lr: float):
        return self.enable_fused_optimizer("sgd", lr)

    def enable_fused_optimizer(self, method: str, lr: float, eps: float = 1e-10,
                               stochastic_rounding: bool = False,
                               seed: Optional[int] = None,
                               betas=(0.9, 0.999)):
        """Enables the in-backward fused optimizer (``"sgd"``, ``"adagrad"``,
        ``"rowwise_adagrad"`` or ``"lazy_adam"``, which takes ``betas``) on
        all model-parallel tables (col + row groups).  Data-parallel tables keep sparse grads (they need the
        allreduce); CPU-offloaded tables keep sparse grads too (their lookup
        runs through the CPU fallback, not the HIP fused kernel).
        See Embedding.enable_fused_optimizer.

        Row-wise Adagrad state is shard-local.  A row-sliced shard owns whole
        rows, so its state equals the undistributed table's.  A column-sliced
        shard sees only its own columns and takes the row mean over that
        slice, so a column-sliced table does *not* train like the unsliced
        one: each slice has its own per-row step size (TorchRec's column-wise
        sharding behaves the same way).  The row sums are not all-reduced.

        Lazy Adam is element-wise: every element's ``m``, ``v`` and update
        depend on that element's summed gradient alone, and every shard
        counts the same steps.  Row-sliced and column-sliced shards
        therefore train exactly like the undistributed table.

        ``stochastic_rounding`` (bf16 tables, ``table_dtype=torch.bfloat16``)
        and ``seed`` are the layer's.  Every local layer gets a seed of its
        own, ``mix64(mix64(mix64(seed) ^ rank) ^ local layer index)``, so no
        two shards share a bit stream; ``seed=None`` draws the base seed
        from torch's default CPU generator."""
        if stochastic_rounding and seed is None:
            seed = int(torch.randint(0, 1 << 62, (1,)))
        for i, lyr in enumerate(list(self.col_layers) + list(self.row_layers)):
            if getattr(lyr, "_cpu_offload", False):
                continue
            lyr_seed = None
            if stochastic_rounding:
                lyr_seed = to_int64(mix64_int(
                    mix64_int(mix64_int(int(seed)) ^ self.rank) ^ i))
            lyr.enable_fused_optimizer(method, lr, eps, stochastic_rounding,
                                       lyr_seed, betas)
        return self

    def quantize_(self, chunk_rows: int = 1 << 20, bits: int = 8):
        """Converts every local table to int8 (``bits=8``) or int4
        (``bits=4``) row-wise storage for serving
        (``Embedding.quantize_``): data-parallel tables, fused column-slice
        groups, row shards and CPU-offloaded tables, each on its device.
        Order of use: load the weights, quantize, serve.  Afterwards
        ``forward`` / ``forward_packed`` run the quantized lookups, outputs
        carry no grad, and ``get_weights`` / ``set_weights`` and the
        checkpoint helpers raise.

        Each local table is quantized by itself, so a column-sliced table
        gets one scale and bias per row *per slice*: slightly more accurate
        than quantizing the whole row, but not the same bytes.  int4 needs
        every local table width, slices included, to be a multiple of 8."""
        if bits not in (4, 8):
            raise ValueError(f"bits must be 4 or 8, got {bits!r}")
        layers = (list(self.dp_layers) + list(self.col_layers)
                  + list(self.row_layers))
        # all or nothing: refuse before the first table is converted
        if any(getattr(lyr, "_fused_lr", None) is not None
               and not lyr.quantized for lyr in layers):
            raise RuntimeError("tables with a fused optimizer enabled cannot "
                               "be quantized: they are being trained")
        if any(lyr.quantized and lyr.quantized_bits != bits
               for lyr in layers):
            raise RuntimeError("some tables are already quantized to another "
                               f"format than int{bits}")
        step = 8 if bits == 4 else 4
        bad = sorted({lyr.output_dim for lyr in layers
                      if lyr.output_dim % step != 0})
        if bad:
            raise ValueError(
                f"int{bits} row-wise quantization needs every local table "
                f"width, column slices included, to be a multiple of {step}, "
                f"got widths {bad}")
        for lyr in layers:
            lyr.quantize_(chunk_rows, bits)
        self.quantized = True
        return self

    def set_multi_hot(self, hotness: Optional[Sequence[int]], seed: int = 0):
        """Turns on-device multi-hot expansion on (``hotness``: one int >= 1
        per input) or off (``None``).

        With the mode on, the dense input of feature ``f`` is either one-hot,
        ``[b]`` or ``[b, 1]``, and then expanded to ``hotness[f]`` ids per
        sample by ``multi_hot_expand(ids, vocab, hotness[f], seed, feature=f)``
        with ``vocab`` the table's full ``input_dim``; or it is
        ``[b, hotness[f]]`` already and taken as it is.  ``Ragged`` inputs
        pass through untouched.  ``hotness[f] > 1`` needs a table with a
        combiner.  Table-parallel and column-sliced inputs cross the dp->mp
        exchange one-hot and are expanded behind it, by the kernel that also
        packs the fused group's ids; every other path expands and then runs
        as it does for ``[b, h]`` inputs.  Either way the result equals
        ``forward`` of the expanded ids, bit for bit.

        ``hotness`` and ``seed`` are configuration, not checkpoint state: a
        model has to be served with the seed (and hotness) it was trained
        with, or its ids select other rows."""
        plan = self.strategy
        if hotness is None:
            self._mh_hotness, self._mh_pair = None, None
            return self
        hotness = [int(h) for h in hotness]
        if len(hotness) != len(plan.input_table_map):
            raise ValueError(
                f"hotness needs one entry per input: got {len(hotness)} for "
                f"{len(plan.input_table_map)} inputs")
        for f, h in enumerate(hotness):
            if h < 1:
                raise ValueError(f"hotness must be >= 1, got {h} (input {f})")
            if h > 1 and plan.configs[plan.input_table_map[f]].combiner is None:
                raise ValueError(
                    f"input {f} has hotness {h} but its table has no "
                    "combiner to reduce the bag")
        self._mh_hotness = hotness
        self._mh_seed = int(seed)
        col_in = plan.input_groups[1]
        self._mh_pair = [self._mh_spec(col_in[i])
                         for i in plan.rank_input_ids[self.rank]]
        return self

    def extra_repr(self) -> str:
        if self._mh_hotness is None:
            return ""
        return f"multi_hot={self._mh_hotness}, multi_hot_seed={self._mh_seed}"

    def _mh_spec(self, f):
        """(hotness, vocab, key_f) of input ``f``; None where nothing is
        expanded (mode off, or hotness 1)."""
        if self._mh_hotness is None or self._mh_hotness[f] == 1:
            return None
        plan = self.strategy
        vocab = plan.configs[plan.input_table_map[f]].input_dim
        return (self._mh_hotness[f], int(vocab),
                multi_hot_key(self._mh_seed, f))

    @staticmethod
    def _mh_one_hot(x) -> bool:
        return x.dim() == 1 or (x.dim() == 2 and x.shape[1] == 1)

    def _mh_check_inputs(self, gids, inputs):
        """With the mode on, a dense input is one-hot or [b, hotness]."""
        if self._mh_hotness is None or len(gids) != len(inputs):
            return
        for f, x in zip(gids, inputs):
            if isinstance(x, Ragged):
                continue
            h = self._mh_hotness[f]
            if not (self._mh_one_hot(x)
                    or (x.dim() == 2 and x.shape[1] == h)):
                raise ValueError(
                    f"input {f}: multi-hot mode takes dense ids of shape "
                    f"[b], [b, 1] or [b, {h}], got {tuple(x.shape)}")

    def _mh_expand(self, spec, x):
        """``x`` expanded by ``spec`` when it is one-hot, else ``x``."""
        if spec is None or isinstance(x, Ragged) or not self._mh_one_hot(x):
            return x
        h, vocab, key_f = spec
        return multi_hot_expand_keyed(x.reshape(x.shape[0]), vocab, h, key_f)

    def _check_not_quantized(self, what):
        if self.quantized:
            raise RuntimeError(
                f"{what} is not available on quantized tables: load "
                "the weights first, then quantize_(), then serve")

    def set_fused_lr(self, lr: float):
        for lyr in list(self.col_layers) + list(self.row_layers):
            if getattr(lyr, "_fused_lr", None) is not None:
                lyr.set_fused_lr(lr)

    def local_input_ids(self) -> List[int]:
        """Global input indices this rank serves in the table-parallel group,
        in local order (for ``dp_input=False`` callers).

        Parity: reference ``strategy.input_ids_list[rank]`` use in
        ``examples/dlrm/main.py:162-176``.
        """
        col_inputs = self.strategy.input_groups[1]
        return [col_inputs[i] for i in self.strategy.rank_input_ids[self.rank]]

    def _validate_batch(self, b: int):
        if self._built or self.world_size == 1:
            return
        sizes = [row[0] for row in comm.all_gather_ints([int(b)])]
        if any(s != sizes[0] for s in sizes):
            raise ValueError(f"per-rank batch sizes differ: {sizes} "
                             "(parity: reference build() check :1171-1173)")
        self._built = True

    # ---------------------------------------------------------------- forward

    def forward(self, inputs: Sequence[Union[torch.Tensor, Ragged]],
                output_dtype: Optional[torch.dtype] = None,
                async_handle: Optional[dict] = None) -> List[torch.Tensor]:
        plan = self.strategy
        self._output_dtype = output_dtype
        dp_in, col_in, row_in = plan.input_groups
        for x in inputs:
            if isinstance(x, torch.Tensor) and x.layout == torch.sparse_coo:
                # parity: the reference rejects SparseTensor inputs to the
                # distributed wrapper (dist_model_parallel.py:263-265)
                raise ValueError(
                    "sparse COO inputs are not supported by "
                    "DistributedEmbedding — convert to Ragged "
                    "(single-table Embedding layers do accept sparse)")
            if isinstance(x, Ragged) and x.weights is not None:
                if x.weights.requires_grad:
                    raise ValueError(
                        "DistributedEmbedding treats Ragged.weights as data "
                        "and computes no gradient for them; weight gradients "
                        "are supported by a single-table Embedding layer "
                        "(pass weights.detach() here)")
                if (not x.weights.is_floating_point()
                        or x.weights.numel() != x.values.numel()):
                    raise ValueError(
                        f"Ragged.weights must hold one floating weight per "
                        f"id: got {x.weights.numel()} for "
                        f"{x.values.numel()} ids")
        self._mh_check_inputs(
            range(len(inputs)) if self.dp_input else self.local_input_ids(),
            inputs)
        if self.dp_input:
            if len(inputs) != len(plan.input_table_map):
                raise ValueError("wrong number of inputs")
            dp_inputs = [self._mh_expand(self._mh_spec(i), inputs[i])
                         for i in dp_in]
            col_inputs = [inputs[i] for i in col_in]
            row_inputs = [inputs[i] for i in row_in]
        else:
            if dp_in or row_in:
                raise ValueError("dp_input=False requires all tables in the "
                                 "table-parallel group")
            dp_inputs, row_inputs = [], []
            col_inputs = list(inputs)

        dp_out = [self.dp_layers[plan.input_maps[0][j]](x)
                  for j, x in enumerate(dp_inputs)]
        if output_dtype is not None:
            dp_out = [o.to(output_dtype) for o in dp_out]
        col_out = self._call_table_parallel(col_inputs, async_handle) \
            if (col_inputs or plan.col_table_ids) else []
        row_out = self._call_row_slice(row_inputs, row_in) \
            if row_inputs else []

        outs = dp_out + col_out + row_out
        return [outs[i] for i in plan.reverse_input_order]

    # ------------------------------------------------------------- checkpoint

    @staticmethod
    def _as_tensor(w):
        if isinstance(w, str):
            w = np.load(w, mmap_mode="r")  # parity: reference mmap path :911,919,950
        if isinstance(w, np.ndarray):
            import warnings
            with warnings.catch_warnings():
                # mmap'd checkpoints are read-only; the tensor is only ever a
                # copy_ SOURCE here, so the non-writable warning is moot
                warnings.simplefilter("ignore", UserWarning)
                w = torch.from_numpy(np.ascontiguousarray(w))
        return w

    def set_weights(self, weights: Sequence, chunk_elements: int = 128 * 1024 * 1024):
        """Distributes full global per-table weights to the local shards.

        ``weights``: one array / tensor / ``.npy`` path per original table, in
        table order — the checkpoint layout contract of the reference
        (``set_weights`` :971-1022; chunked writes parity :1003-1017).
        """
        self._check_not_quantized("set_weights")
        cfgs = self.strategy.configs
        if len(weights) != len(cfgs):
            raise ValueError(f"expected {len(cfgs)} tables, got {len(weights)}")

        def copy_into(dst, src):
            n = src.shape[0]
            step = max(1, chunk_elements // max(1, src.shape[1]))
            with torch.no_grad():
                for s in range(0, n, step):
                    e = min(n, s + step)
                    dst[s:e].copy_(self._as_tensor(src[s:e]).to(dst.dtype))

        plan = self.strategy
        for local_t, t in enumerate(plan.dp_table_ids):
            copy_into(self.dp_layers[local_t].weight, self._as_tensor(weights[t]))
        for s in plan.rank_slices[self.rank]:
            w = self._as_tensor(weights[s.table_id])
            dst = self.col_layers[s.concat_group].weight
            rows = self.strategy.configs[s.table_id].input_dim
            sub = w[:, s.col_offset:s.col_offset + s.width]
            copy_into(dst[s.concat_row_offset:s.concat_row_offset + rows], sub)
        for local_t, shard in enumerate(plan.local_row_shards(self.rank)):
            w = self._as_tensor(weights[shard.table_id])
            copy_into(self.row_layers[local_t].weight,
                      w[shard.row_offset:shard.row_offset + shard.rows])

    def get_weights(self, all_ranks: bool = False,
                    chunk_elements: int = 128 * 1024 * 1024) -> List[np.ndarray]:
        """Reassembles full global per-table weights (on CPU, numpy).

        Parity: reference ``get_weights`` (:1139-1162) — returns the tables in
        original order; with ``all_ranks=False`` only rank 0's return value is
        meaningful on GPU backends (collectives still run on every rank).

        Every collective moves at most ``chunk_elements`` elements and the
        transient device buffers are O(chunk), not O(table) — 2e9-row tables
        reassemble with bounded peak memory (parity: reference ≤2e9-element
        chunked allgather + ``_split_1d``, dist_model_parallel.py:1024-1046,
        1069-1098; per-chunk counts stay far below int32 limits by
        construction).
        """
        import torch.distributed as dist
        self._check_not_quantized("get_weights")
        cfgs = self.strategy.configs
        plan = self.strategy
        out: List[Optional[np.ndarray]] = [None] * len(cfgs)
        for local_t, t in enumerate(plan.dp_table_ids):
            # .float(): checkpoints are fp32 numpy regardless of table_dtype
            # (bf16 storage has no numpy dtype)
            out[t] = self.dp_layers[local_t].weight.detach().float().cpu().numpy()

        # column slices: broadcast each slice from its owner in row chunks.
        device = self._comm_device()
        for t in plan.col_table_ids:
            cfg = cfgs[t]
            cols = []
            for s in plan.table_slices[t]:
                step = max(1, chunk_elements // s.width)
                pieces = []
                for r0 in range(0, cfg.input_dim, step):
                    r1 = min(cfg.input_dim, r0 + step)
                    buf = torch.empty(r1 - r0, s.width, device=device)
                    if s.rank == self.rank:
                        src = self.col_layers[s.concat_group].weight.detach()
                        buf.copy_(src[s.concat_row_offset + r0:
                                      s.concat_row_offset + r1])
                    if self.world_size > 1:
                        dist.broadcast(buf, src=s.rank)
                    pieces.append(buf.cpu())
                cols.append(torch.cat(pieces, dim=0))
            out[t] = torch.cat(cols, dim=1).numpy()

        # row shards: chunked allgather of uneven rows (every rank iterates
        # the same global chunk count so the collectives stay matched).
        for t in plan.row_table_ids:
            local_t = plan.row_table_ids.index(t)
            my_rows = plan.row_shards[t][self.rank].rows
            width = cfgs[t].output_dim
            max_rows = max(sh.rows for sh in plan.row_shards[t])
            step = max(1, chunk_elements // width)
            nchunks = max(-(-max_rows // step), 1)
            per_rank = [[] for _ in range(self.world_size)]
            w_local = self.row_layers[local_t].weight.detach()
            for ci in range(nchunks):
                r0 = ci * step
                r1 = min(my_rows, r0 + step)
                piece = w_local[r0:max(r0, r1)].float().to(device)
                parts = comm.all_gather_uneven(piece)
                for k, p in enumerate(parts):
                    if p.shape[0]:
                        per_rank[k].append(p.cpu())
            out[t] = torch.cat(
                [torch.cat(p, dim=0) if p else
                 torch.empty(0, width) for p in per_rank], dim=0).numpy()
        return out

    def _comm_device(self):
        import os
        import torch.distributed as dist
        ov = os.environ.get("DE_COMM_DEVICE")
        if ov == "cuda":
            # test-lane override: build comm buffers as an nccl job would
            # (see comm._strict_check)
            return torch.device("cuda", torch.cuda.current_device())
        if self.world_size > 1 and dist.get_backend() == "nccl":
            return torch.device("cuda", torch.cuda.current_device())
        if self.world_size == 1:
            if not len(self.col_layers):
                return torch.device("cpu")
            lyr = self.col_layers[0]
            return (lyr.qweight if lyr.quantized else lyr.weight).device
        return torch.device("cpu")

    # ----------------------------------------------------- table parallel path

    def _dense_splits(self, col_inputs):
        """Cached (in_splits, my_sizes, out_splits) per input-shape signature."""
        plan = self.strategy
        W = self.world_size
        sig = ("dp2mp", tuple(tuple(x.shape) for x in col_inputs))
        cache = getattr(self, "_split_cache", None)
        if cache is None:
            cache = self._split_cache = {}
        cached = cache.get(sig)
        if cached is None:
            in_splits = []
            for k in range(W):
                in_splits.append(sum(col_inputs[i].numel()
                                     for i in plan.rank_input_ids[k]))
            my_sizes = [col_inputs[i].numel()
                        for i in plan.rank_input_ids[self.rank]]
            cached = (in_splits, my_sizes, [sum(my_sizes)] * W)
            cache[sig] = cached
        return cached

    def _dense_send_buffer(self, col_inputs):
        plan = self.strategy
        W = self.world_size
        send_parts = [col_inputs[i].reshape(-1)
                      for k in range(W) for i in plan.rank_input_ids[k]]
        return torch.cat(send_parts) if send_parts else \
            torch.empty(0, dtype=torch.long, device=self._comm_device())

    def _carve_dense_recv(self, recv, my_sizes, col_inputs):
        """recv: [W * sum(my_sizes)] flat ids -> per local pair [W*b, ...]."""
        plan = self.strategy
        W = self.world_size
        recv = recv.view(W, -1) if recv.numel() else recv.view(W, 0)
        parts = torch.split(recv, my_sizes, dim=1) if my_sizes else []
        out = []
        for j, i in enumerate(plan.rank_input_ids[self.rank]):
            shape = col_inputs[i].shape
            out.append(parts[j].reshape(W * shape[0], *shape[1:]))
        return out

    def _dp_to_mp_dense(self, col_inputs):
        """Dense id redistribution dp->mp (parity: reference ``:169-221``).

        Returns per local pair: ids tensor of shape [W*b, ...feature dims].
        """
        in_splits, my_sizes, out_splits = self._dense_splits(col_inputs)
        send = self._dense_send_buffer(col_inputs)
        recv = comm.all_to_all_single(send, out_splits, in_splits)
        return self._carve_dense_recv(recv, my_sizes, col_inputs)

    def redistribute_async(self, inputs) -> Optional[dict]:
        """Posts the dp->mp ID all-to-all WITHOUT waiting, so the caller can
        overlap independent compute (e.g. DLRM's bottom MLP) with the id
        exchange on the xGMI links.  Ids carry no gradient, so no autograd
        plumbing is needed.  Pass the returned handle to
        ``forward(..., async_handle=h)``.

        Returns None when there is nothing to overlap (world==1, mp-input
        mode, no table-parallel inputs, or ragged inputs present — those take
        the two-phase sync path).
        """
        import torch.distributed as dist
        plan = self.strategy
        if self.world_size == 1 or not self.dp_input or not plan.col_table_ids:
            return None
        col_in = plan.input_groups[1]
        col_inputs = [inputs[i] for i in col_in]
        if not col_inputs or any(isinstance(x, Ragged) for x in col_inputs):
            return None
        self._validate_batch(col_inputs[0].shape[0])
        in_splits, my_sizes, out_splits = self._dense_splits(col_inputs)
        send = self._dense_send_buffer(col_inputs)
        dev = comm.backend_device()
        src = send.contiguous().to(dev)
        recv = src.new_empty(sum(out_splits))
        work = dist.all_to_all_single(recv, src,
                                      output_split_sizes=[int(v) for v in out_splits],
                                      input_split_sizes=[int(v) for v in in_splits],
                                      async_op=True)
        return {"work": work, "recv": recv, "my_sizes": my_sizes,
                "device": send.device,
                "sig": tuple(tuple(x.shape) for x in col_inputs)}

    def _dp_to_mp_ragged(self, col_inputs, ragged_mask):
        """Ragged id redistribution dp->mp (two-phase; parity ``:115-166``).

        Dense inputs in the same batch are redistributed by `_dp_to_mp_dense`
        semantics within one fused pair of all-to-alls.  When any input
        carries weights, one more fp32 all-to-all with the value splits moves
        them (unweighted inputs send ones); without weights nothing extra is
        sent.
        """
        plan = self.strategy
        W = self.world_size
        if W == 1:
            # nothing to exchange: the inputs are the pairs (and sizing the
            # receive buffers would cost a host sync per ragged pair)
            return [col_inputs[i] for i in plan.rank_input_ids[self.rank]]
        # Phase 1: all-to-all of row_lengths for ragged pairs + flat sizes.
        len_parts, len_in_splits = [], []
        for k in range(W):
            n = 0
            for i in plan.rank_input_ids[k]:
                x = col_inputs[i]
                if isinstance(x, Ragged):
                    len_parts.append(x.row_lengths())
                    n += x.nrows
            len_in_splits.append(n)
        my_ragged = [i for i in plan.rank_input_ids[self.rank]
                     if isinstance(col_inputs[i], Ragged)]
        my_rows = [col_inputs[i].nrows for i in my_ragged]
        len_out_splits = [sum(my_rows)] * W
        if len_parts:
            lens = comm.all_to_all_single(torch.cat(len_parts), len_out_splits, len_in_splits)
            lens = lens.view(W, -1)
        else:
            lens = None

        # Phase 2: all-to-all of values (ragged) interleaved with dense ids.
        send_parts, in_splits = [], []
        for k in range(W):
            n = 0
            for i in plan.rank_input_ids[k]:
                x = col_inputs[i]
                v = x.values if isinstance(x, Ragged) else x.reshape(-1)
                send_parts.append(v)
                n += v.numel()
            in_splits.append(n)
        send = torch.cat(send_parts)
        any_weighted = any(isinstance(x, Ragged) and x.weights is not None
                           for x in col_inputs)
        send_w = None
        if any_weighted:
            w_parts = []
            for k in range(W):
                for i in plan.rank_input_ids[k]:
                    x = col_inputs[i]
                    if isinstance(x, Ragged) and x.weights is not None:
                        w_parts.append(x.weights.reshape(-1).float())
                    else:
                        n = x.values.numel() if isinstance(x, Ragged) else x.numel()
                        w_parts.append(torch.ones(n, dtype=torch.float32,
                                                  device=send.device))
            send_w = torch.cat(w_parts)
        # out sizes per src rank: dense sizes are static; ragged from lens.
        lens_by_pair = torch.split(lens, my_rows, dim=1) if lens is not None else []
        per_src_sizes = []  # [W][num_my_pairs]
        for r in range(W):
            sizes = []
            ri = 0
            for i in plan.rank_input_ids[self.rank]:
                x = col_inputs[i]
                if isinstance(x, Ragged):
                    sizes.append(int(lens_by_pair[ri][r].sum().item()))
                    ri += 1
                else:
                    sizes.append(x.numel())
            per_src_sizes.append(sizes)
        out_splits = [sum(s) for s in per_src_sizes]
        recv = comm.all_to_all_single(send, out_splits, in_splits)
        recv_w = None
        if send_w is not None:
            recv_w = comm.all_to_all_single(send_w, out_splits, in_splits)

        # Reassemble per pair across sources.
        def pair_slice(buf, j):
            chunks = torch.split(buf, out_splits)
            return torch.cat([chunks[r].split(per_src_sizes[r])[j]
                              for r in range(W)])

        out = []
        ri = 0
        for j, i in enumerate(plan.rank_input_ids[self.rank]):
            x = col_inputs[i]
            vals = pair_slice(recv, j)
            if isinstance(x, Ragged):
                pair_lens = lens_by_pair[ri].reshape(-1)  # [W*b]
                ri += 1
                pair_w = (pair_slice(recv_w, j) if x.weights is not None
                          else None)
                out.append(Ragged.from_row_lengths(vals, pair_lens, pair_w))
            else:
                shape = x.shape
                out.append(vals.reshape(W * shape[0], *shape[1:]))
        return out

    def _fused_group_lookup(self, pair_ids, unsplit=False):
        """Runs every local pair's lookup, one fused call per concat group.

        Returns per-pair 2-D outputs [rows, out_cols] in local pair order.
        With ``unsplit=True`` (single concat group, packed fast path) the raw
        group output [total_rows, width] is returned without the per-pair
        split — zero extra copies.
        """
        plan = self.strategy
        groups = plan.local_concat_groups(self.rank)
        per_group_pairs = [[] for _ in groups]
        for j, ids in enumerate(pair_ids):
            per_group_pairs[self._pair_group[j]].append(j)

        outs: List[Optional[torch.Tensor]] = [None] * len(pair_ids)
        for gi, pair_js in enumerate(per_group_pairs):
            if not pair_js:
                continue
            layer = self.col_layers[gi]
            grp = groups[gi]
            offload = getattr(layer, "_cpu_offload", False)
            if grp.combiner is None:
                if any(isinstance(pair_ids[j], Ragged) for j in pair_js):
                    raise ValueError("Ragged input requires a table with a "
                                     "combiner")
                # hotness-1 CSR gather: one cat + one cached-offset add for the
                # whole group (instead of one add per pair per step).
                metas = [(j, pair_ids[j].shape, pair_ids[j].numel()) for j in pair_js]
                allids = self._group_ids(
                    gi, [(pair_ids[j], 1, None, self._pair_row_offset[j])
                         for j in pair_js])
                if offload:
                    allids_cpu = allids.cpu()
                    splits = torch.arange(allids_cpu.numel() + 1, dtype=torch.long)
                    emb = _offloaded_lookup(layer, Ragged(allids_cpu, splits),
                                            "sum").to(allids.device)
                else:
                    splits = torch.arange(allids.numel() + 1, device=allids.device,
                                          dtype=torch.long)
                    emb = layer.csr_lookup(allids, splits, "sum",
                                           out_dtype=self._kernel_out_dtype(allids))
                if getattr(self, "_output_dtype", None) is not None:
                    emb = emb.to(self._output_dtype)
                if unsplit:
                    return emb
                # torch.split (not manual narrow): its backward is ONE cat
                # instead of per-slice zero-fill + accumulate.
                parts = torch.split(emb, [n for _, _, n in metas])
                for (j, shape, n), part in zip(metas, parts):
                    outs[j] = part.reshape(shape[0], -1)
            else:
                # One CSR batch over all pairs of this group; splits merged on
                # device (no host syncs even for ragged inputs).
                val_parts, metas, row_offs = [], [], []
                # per dense pair (hotness after expansion, expansion or None)
                hots = {}
                device = None
                all_dense = all(not isinstance(pair_ids[j], Ragged) for j in pair_js)
                for j in pair_js:
                    ids = pair_ids[j]
                    off = self._pair_row_offset[j]
                    if isinstance(ids, Ragged):
                        val_parts.append(ids.values)
                        nrows = ids.nrows
                        device = ids.values.device
                    else:
                        nrows = ids.shape[0]
                        device = ids.device
                        spec = self._mh_pair[j] if self._mh_pair else None
                        if spec is not None and self._mh_one_hot(ids):
                            hots[j] = (spec[0], spec)
                        else:
                            hots[j] = (ids.shape[1] if ids.dim() > 1 else 1,
                                       None)
                        if not all_dense:
                            ids = self._mh_expand(hots[j][1], ids)
                        val_parts.append(ids)
                    row_offs.append((off, nrows))
                    metas.append((j, nrows))

                def make_len_parts():
                    lp = []
                    for j in pair_js:
                        ids = pair_ids[j]
                        if isinstance(ids, Ragged):
                            lp.append(ids.row_lengths())
                        else:
                            lp.append(torch.full((ids.shape[0],), hots[j][0],
                                                 dtype=torch.long, device=device))
                    return lp

                if not all_dense:
                    allvals = _cat_or_view(val_parts)
                # per-id weights, only when a pair of the group has some:
                # its unweighted pairs count with ones
                allw = None
                if any(isinstance(pair_ids[j], Ragged)
                       and pair_ids[j].weights is not None for j in pair_js):
                    allw = torch.cat([
                        pair_ids[j].weights.reshape(-1).float()
                        if isinstance(pair_ids[j], Ragged)
                        and pair_ids[j].weights is not None
                        else torch.ones(v.numel(), dtype=torch.float32,
                                        device=device)
                        for j, v in zip(pair_js, val_parts)])
                if all_dense:
                    # static shapes: per-element offsets + splits fully cached
                    espec, segs = [], []
                    # an offloaded table expands on the host, in numpy
                    on_host = offload and any(
                        hots[j][1] is not None for j in pair_js)
                    for j, ids in zip(pair_js, val_parts):
                        h, spec = hots[j]
                        espec.append((self._pair_row_offset[j], ids.shape[0] * h))
                        if on_host:
                            ids = ids.cpu()
                        if spec is None:
                            segs.append((ids, 1, None, self._pair_row_offset[j]))
                        else:
                            segs.append((ids, h, spec[1:],
                                         self._pair_row_offset[j]))
                    allvals = self._group_ids(gi, segs)
                    skey = ("splits", gi, tuple(espec), str(device))
                    cache = getattr(self, "_off_cache", None) or {}
                    self._off_cache = cache
                    if skey not in cache:
                        all_lengths = torch.cat(make_len_parts())
                        sp = torch.zeros(all_lengths.numel() + 1, dtype=torch.long,
                                         device=device)
                        torch.cumsum(all_lengths, 0, out=sp[1:])
                        cache[skey] = sp
                    allsplits = cache[skey]
                else:
                    all_lengths = torch.cat(make_len_parts())
                    row_off_vec = self._row_offset_vector(gi, row_offs, device)
                    if row_off_vec is not None:
                        # output_size: no host sync to size the result
                        allvals = allvals + torch.repeat_interleave(
                            row_off_vec, all_lengths,
                            output_size=allvals.numel())
                    allsplits = torch.zeros(all_lengths.numel() + 1, dtype=torch.long,
                                            device=device)
                    torch.cumsum(all_lengths, 0, out=allsplits[1:])
                if offload:
                    out = _offloaded_lookup(
                        layer,
                        Ragged(allvals.cpu(), allsplits.cpu(),
                               None if allw is None else allw.cpu()),
                        grp.combiner).to(device)
                else:
                    out = layer.csr_lookup(allvals, allsplits, grp.combiner,
                                           out_dtype=self._kernel_out_dtype(allvals),
                                           per_id_w=allw)
                if getattr(self, "_output_dtype", None) is not None:
                    out = out.to(self._output_dtype)
                if unsplit:
                    return out
                parts = torch.split(out, [nrows for _, nrows in metas])
                for (j, nrows), part in zip(metas, parts):
                    outs[j] = part
        return outs

    def _group_ids(self, gi, segs):
        """The flat id vector of one fused group from ``segs``, a list of
        ``pack_ids`` segments ``(ids, h_out, expand, row offset)``.

        One ``pack_ids`` launch when there is anything to do (an offset to
        add or a bag to expand) and the kernel applies: contiguous int64 GPU
        ids, the extension loaded, ``DE_PACK_IDS`` not 0.  Otherwise the torch
        composition: expansion, cat (a view when the parts are adjacent),
        cached offset vector add."""
        if any(off or exp is not None for _, _, exp, off in segs) \
                and pack_ids_enabled() and _backend.available() \
                and all(ids.is_cuda and ids.dtype == torch.int64
                        and ids.is_contiguous() for ids, _, _, _ in segs):
            return pack_ids([(ids.reshape(-1), h, exp, off)
                             for ids, h, exp, off in segs])
        parts = [ids if exp is None
                 else multi_hot_expand_keyed(ids.reshape(ids.shape[0]),
                                             exp[0], h, exp[1])
                 for ids, h, exp, _ in segs]
        allids = _cat_or_view(parts)
        off_vec = self._offset_vector(
            gi, [(off, p.numel()) for p, (_, _, _, off) in zip(parts, segs)],
            allids.device)
        if off_vec is not None:
            allids = allids + off_vec
        return allids

    def _kernel_out_dtype(self, ids):
        """bf16 when the caller asked for bf16 outputs and the lookup runs
        the HIP kernel (the kernel stores bf16 directly; the later .to() then
        no-ops).  None otherwise — CPU/gloo paths keep fp32 numerics."""
        if getattr(self, "_output_dtype", None) == torch.bfloat16 and ids.is_cuda:
            return torch.bfloat16
        return None

    def _offset_vector(self, gi, spec, device, kind="elem"):
        """Cached fused-table offset vector for ``spec`` = [(offset, count)].

        ``kind='elem'``: one entry per id element; ``kind='row'``: one entry
        per CSR row (expanded by repeat_interleave at the call site).
        Returns None when every offset is zero.
        """
        key = (kind, gi, tuple(spec), str(device))
        cache = getattr(self, "_off_cache", None)
        if cache is None:
            cache = self._off_cache = {}
        if key not in cache:
            if all(off == 0 for off, _ in spec):
                cache[key] = None
            else:
                cache[key] = torch.cat([
                    torch.full((n,), off, dtype=torch.long, device=device)
                    for off, n in spec])
        return cache[key]

    def _row_offset_vector(self, gi, spec, device):
        return self._offset_vector(gi, spec, device, kind="row")

    def _call_table_parallel(self, col_inputs, async_handle=None):
        plan = self.strategy
        W = self.world_size
        if not plan.col_table_ids:
            return []

        local_b = None
        if self.dp_input:
            any_ragged = any(isinstance(x, Ragged) for x in col_inputs)
            if col_inputs:
                b = (col_inputs[0].nrows if isinstance(col_inputs[0], Ragged)
                     else col_inputs[0].shape[0])
                self._validate_batch(b)
                local_b = b  # dp-side batch known on every rank
            if async_handle is not None:
                if async_handle["sig"] != tuple(tuple(x.shape) for x in col_inputs):
                    raise ValueError("async_handle does not match these inputs")
                async_handle["work"].wait()
                recv = async_handle["recv"].to(async_handle["device"])
                pair_ids = self._carve_dense_recv(
                    recv, async_handle["my_sizes"], col_inputs)
            elif any_ragged:
                pair_ids = self._dp_to_mp_ragged(col_inputs, None)
            else:
                pair_ids = self._dp_to_mp_dense(col_inputs)
        else:
            pair_ids = list(col_inputs)
            if pair_ids:
                n0 = pair_ids[0].nrows if isinstance(pair_ids[0], Ragged) else \
                    pair_ids[0].shape[0]
                if n0 % W:
                    raise ValueError(
                        f"model-parallel input batch {n0} not divisible by world {W} "
                        "(parity: reference :1175-1177)")
                local_b = n0 // W
        # A rank left without column slices by the planner still participates
        # in the output all-to-all: exchange the batch size when the plan
        # leaves ANY rank empty (global plan => every rank enters the
        # collective consistently).
        if any(len(plan.rank_input_ids[k]) == 0 for k in range(W)):
            vals = comm.all_gather_ints([local_b if local_b is not None else -1])
            known = [v[0] for v in vals if v[0] >= 0]
            local_b = known[0] if known else 0
        if local_b is None:
            local_b = 0

        outs = self._fused_group_lookup(pair_ids)  # per pair [W*b, c]

        if W == 1:
            # the all-to-all is a passthrough: the pair outputs ARE the
            # worker outputs — skip the send-side cat + recv split entirely
            # (a 116-slice batched cat costs real time on many-table models)
            worker_outs = outs
        else:
            # mp->dp output all-to-all (parity: reference :868-878).
            if outs:
                send = torch.cat([o.reshape(W, -1) for o in outs],
                                 dim=1).reshape(-1)
            else:
                # empty-contribution rank: buffer must match peers'
                # device/dtype for the RCCL collective, and must REQUIRE GRAD
                # so this rank enters the reverse all-to-all in backward
                send = torch.empty(
                    0,
                    dtype=getattr(self, "_output_dtype", None) or self.table_dtype,
                    device=self._comm_device(),
                    requires_grad=torch.is_grad_enabled())
            my_cols = sum(o.shape[1] for o in outs) if outs else 0
            in_splits = [local_b * my_cols] * W
            # Per-pair output column counts of every rank (static after first
            # call; out_cols may exceed the slice width for no-combiner
            # multi-hot inputs).
            my_pair_cols = [o.shape[1] for o in outs]
            all_cols = self._exchange_pair_cols(my_pair_cols)
            out_splits = [local_b * sum(all_cols[k]) for k in range(W)]
            recv = comm.all_to_all_single(send, out_splits, in_splits)

            # split per source rank, then per pair (pair-major layout within
            # each source block, matching the send layout); reorder to input
            # order.
            chunks = torch.split(recv, out_splits)
            worker_outs = []
            for k in range(W):
                sizes = [local_b * c for c in all_cols[k]]
                parts = torch.split(chunks[k], sizes)
                worker_outs.extend(p.view(local_b, c)
                                   for p, c in zip(parts, all_cols[k]))
        ordered = [worker_outs[i] for i in plan.rev_tp_order]
        # per ordered entry, the slice width (ordered slices of one input are
        # in col_offset order — worker order == rank walk order in the plan)
        ordered_widths = [plan.widths_list_flat[i] for i in plan.rev_tp_order]

        # concat column slices back together (parity: reference :884-886) and
        # restore the hotness dimension for no-combiner multi-hot inputs
        # (matching the Embedding layer / row-slice output contract: the
        # column count of such a pair is hotness*width, so slice concat must
        # interleave on the LAST dim, not blockwise on dim 1).
        merged = []
        ranges = {start: stop for start, stop in plan.sliced_out_ranges}
        idx = 0
        inp_local = 0
        while idx < len(ordered):
            stop = ranges.get(idx, idx + 1)
            parts = ordered[idx:stop]
            widths = ordered_widths[idx:stop]
            t = plan.col_table_ids[plan.input_maps[1][inp_local]]
            feat_shape = None
            if plan.configs[t].combiner is None:
                if self.dp_input and inp_local < len(col_inputs):
                    x = col_inputs[inp_local]
                    if not isinstance(x, Ragged) and x.dim() > 1:
                        feat_shape = tuple(x.shape[1:])
                else:
                    # mp-input mode: derive hotness from the column count
                    hot = parts[0].shape[1] // widths[0]
                    if hot > 1:
                        feat_shape = (hot,)
            if feat_shape is not None:
                parts = [p.view(local_b, *feat_shape, w)
                         for p, w in zip(parts, widths)]
                merged.append(parts[0] if len(parts) == 1
                              else torch.cat(parts, dim=-1))
            else:
                merged.append(parts[0] if len(parts) == 1
                              else torch.cat(parts, dim=1))
            idx = stop
            inp_local += 1
        return merged

    def _exchange_pair_cols(self, my_pair_cols):
        """Share per-pair output column counts across ranks.

        Cached PER column-count signature: for no-combiner inputs the count is
        ``hotness*width``, so a hotness change between calls must re-exchange
        (shape changes are globally consistent — the same contract as the
        dp-side ``_split_cache``).  Tensor collectives only (RCCL-safe).
        """
        key = tuple(my_pair_cols)
        cache = getattr(self, "_pair_cols_cache", None)
        if cache is None:
            cache = self._pair_cols_cache = {}
        if key not in cache:
            cache[key] = comm.all_gather_int_vectors(list(my_pair_cols))
        return cache[key]

    # ------------------------------------------------------ packed fast path

    def packed_forward_available(self) -> bool:
        """True when ``forward_packed`` applies: dp-input mode, every table in
        ONE same-width table-parallel concat group per rank, no column
        slicing, no dp/row groups.  (The DLRM flagship shape.)"""
        plan = self.strategy
        if not self.dp_input:
            return False
        if plan.dp_table_ids or plan.row_table_ids:
            return False
        if plan.sliced_out_ranges:
            return False
        widths = {s.width for r in range(self.world_size)
                  for s in plan.rank_slices[r]}
        if len(widths) != 1:
            return False
        if any(g.cpu_offload for r in range(self.world_size)
               for g in plan.rank_concat_groups[r]):
            return False
        return all(len(plan.rank_concat_groups[r]) == 1
                   for r in range(self.world_size))

    def packed_order(self) -> List[int]:
        """``packed_order()[f]`` = packed row of input f (worker order).

        Build this once into a device int32 buffer and hand it to
        ``dot_interact_packed`` so interaction columns stay in model input
        order at every world size / plan.
        """
        return list(self.strategy.rev_tp_order)

    def forward_packed(self, inputs: Sequence[torch.Tensor],
                       output_dtype: Optional[torch.dtype] = None,
                       async_handle: Optional[dict] = None):
        """Returns ALL lookups as one packed tensor: ``(packed, sample_major)``.

        Zero-copy relative to :meth:`forward`: ``packed`` is
        [P, b, width] feature-major — at world==1 a view of the fused-group
        lookup output, at world>1 a view of the mp->dp all-to-all recv
        buffer.  Packed rows are in worker order (see :meth:`packed_order`);
        the per-pair split + stack/merge copies of the general path
        disappear.  Requires :meth:`packed_forward_available` and hotness-1
        dense inputs (or 2-D with a combiner); in multi-hot mode
        (:meth:`set_multi_hot`) the one-hot inputs are expanded like in
        :meth:`forward`.  (``DE_PACKED_SMAJ=1``
        switches world==1 to a sample-major [b, P, width] layout — measured
        slower end-to-end, kept for experiments; hence the boolean in the
        return value.)
        """
        plan = self.strategy
        W = self.world_size
        self._output_dtype = output_dtype
        col_in = plan.input_groups[1]
        col_inputs = [inputs[i] for i in col_in]
        self._mh_check_inputs(col_in, col_inputs)
        for j, x in enumerate(col_inputs):
            comb = plan.configs[plan.col_table_ids[plan.input_maps[1][j]]].combiner
            if isinstance(x, Ragged) or x.dim() > 2 or (
                    x.dim() == 2 and comb is None and x.shape[1] != 1):
                raise ValueError("forward_packed requires hotness-1 dense "
                                 "inputs (or 2-D with a combiner)")
        b = col_inputs[0].shape[0]
        self._validate_batch(b)
        if async_handle is not None:
            if async_handle["sig"] != tuple(tuple(x.shape) for x in col_inputs):
                raise ValueError("async_handle does not match these inputs")
            async_handle["work"].wait()
            recv_ids = async_handle["recv"].to(async_handle["device"])
            pair_ids = self._carve_dense_recv(
                recv_ids, async_handle["my_sizes"], col_inputs)
        else:
            pair_ids = self._dp_to_mp_dense(col_inputs)
        if W == 1:
            import os
            if os.environ.get("DE_PACKED_SMAJ") == "1":
                # sample-interleaved ids give a [b, P, D] output directly,
                # but MEASURED SLOWER end-to-end: they destroy the lookup's
                # per-table cache locality (pair-major streams each table's
                # whole batch through one hot region).  Kept for measurement.
                if self._mh_pair:
                    pair_ids = [self._mh_expand(spec, ids) for spec, ids
                                in zip(self._mh_pair, pair_ids)]
                return self._packed_lookup_sample_major(pair_ids, b), True
            group_out = self._fused_group_lookup(pair_ids, unsplit=True)
            return group_out.view(len(pair_ids), b, -1), False
        group_out = self._fused_group_lookup(pair_ids, unsplit=True)
        D = group_out.shape[-1]
        P_local = len(pair_ids)
        send = group_out.view(P_local, W, b * D).transpose(0, 1).reshape(-1)
        all_cols = self._exchange_pair_cols([D] * P_local)
        out_splits = [b * sum(all_cols[k]) for k in range(W)]
        in_splits = [b * D * P_local] * W
        recv = comm.all_to_all_single(send, out_splits, in_splits)
        P_total = sum(len(c) for c in all_cols)
        return recv.view(P_total, b, D), False

    def _packed_lookup_sample_major(self, pair_ids, b):
        """One fused CSR lookup over sample-interleaved ids -> [b, P, D]."""
        plan = self.strategy
        layer = self.col_layers[0]
        grp = plan.local_concat_groups(self.rank)[0]
        parts = [ids.view(b, -1) for ids in pair_ids]
        mat = torch.cat(parts, dim=1)            # [b, sum_h] — ids only
        allids = mat.reshape(-1)
        device = allids.device
        espec = tuple((self._pair_row_offset[j], int(p.shape[1]))
                      for j, p in enumerate(parts))
        key = ("smaj", espec, b, str(device))
        cache = getattr(self, "_off_cache", None)
        if cache is None:
            cache = self._off_cache = {}
        if key not in cache:
            offp = None
            if any(off for off, _ in espec):
                offp = torch.cat([
                    torch.full((h,), off, dtype=torch.long, device=device)
                    for off, h in espec]).repeat(b)
            if grp.combiner is None:
                splits = torch.arange(allids.numel() + 1, device=device,
                                      dtype=torch.long)
            else:
                lens = torch.tensor([h for _, h in espec], dtype=torch.long,
                                    device=device).repeat(b)
                splits = torch.zeros(lens.numel() + 1, dtype=torch.long,
                                     device=device)
                torch.cumsum(lens, 0, out=splits[1:])
            cache[key] = (offp, splits)
        offp, splits = cache[key]
        if offp is not None:
            allids = allids + offp
        out = layer.csr_lookup(allids, splits, grp.combiner or "sum",
                               out_dtype=self._kernel_out_dtype(allids))
        if getattr(self, "_output_dtype", None) is not None:
            out = out.to(self._output_dtype)
        return out.view(b, len(pair_ids), -1)

    # --------------------------------------------------------- row slice path

    def _call_row_slice(self, row_inputs, row_gids):
        """Allgather ids -> offset local lookup (OOB->0) -> reduce-scatter.

        Parity: reference ``_call_row_slice`` (:889-904) with the xGMI-native
        twist that all tables share one fused reduce-scatter.
        """
        plan = self.strategy
        W = self.world_size
        shards = plan.local_row_shards(self.rank)
        outs = []
        for j, x in enumerate(row_inputs):
            tbl_local = plan.input_maps[2][j]
            shard = shards[tbl_local]
            layer = self.row_layers[tbl_local]
            if isinstance(x, Ragged):
                # ragged row-slice (beyond the reference, which is dense-only
                # here): allgather lengths + values, lookup with offset
                # (OOB contributes zero), reduce-scatter the combined rows.
                lens_parts = comm.all_gather_uneven(x.row_lengths())
                vals_parts = comm.all_gather_uneven(x.values)
                g_w = None
                if x.weights is not None:
                    g_w = torch.cat(comm.all_gather_uneven(
                        x.weights.reshape(-1).float()))
                g_ragged = Ragged.from_row_lengths(
                    torch.cat(vals_parts) - shard.row_offset,
                    torch.cat(lens_parts), g_w)
                out = layer(g_ragged)                # [W*b, D]
            else:
                gathered = comm.all_gather(x)        # [W*b, ...]
                # multi-hot: expand behind the gather, with the full table's
                # vocabulary, before the ids become shard-relative
                gathered = self._mh_expand(self._mh_spec(row_gids[j]), gathered)
                ids = gathered - shard.row_offset    # negative => OOB => zero row
                out = layer(ids)                     # [W*b, (h,) D]
            outs.append(out.reshape(W, -1))
        fused = torch.cat(outs, dim=1).reshape(-1)   # [W * sum(b*c)]
        red = comm.reduce_scatter(fused)             # [sum(b*c)]
        # split back per input
        result, pos = [], 0
        for j, x in enumerate(row_inputs):
            b = x.nrows if isinstance(x, Ragged) else x.shape[0]
            n = outs[j].shape[1]
            flat = red[pos:pos + n]
            pos += n
            tbl_local = plan.input_maps[2][j]
            width = self.row_layers[tbl_local].output_dim
            if (self.row_layers[tbl_local].combiner is None
                    and not isinstance(x, Ragged) and x.dim() > 1):
                out_t = flat.view(b, *x.shape[1:], width)
            else:
                out_t = flat.view(b, width)
            if getattr(self, "_output_dtype", None) is not None:
                out_t = out_t.to(self._output_dtype)
            result.append(out_t)
        return result
