"""The fused update split in two: csr_sort_plan (ids only) and
csr_fused_optimizer_apply_planned (gradient), against the one-shot
csr_fused_optimizer_apply, and the DLRM path that builds the plan during the
forward (DE_HOIST_SORT).

Where the one-shot call is itself exact -- deterministic mode, or no id more
than 128 times, so no long segment -- the planned form has to give the same
bits.  On the default long path partials meet in fp32 atomics, so the one-shot
call does not repeat itself bit for bit; there the two are compared with the
bound of the fused-update tests of test_gpu.py:

  * a sum of n N(0,1)-sized terms: atol 1e-3 (n * eps * max|x|, tenfold
    margin).  Here n <= 5003 and the upstream gradient is scaled by 2**-5, so
    n * eps * max|x| ~ 5003 * 6e-8 * 0.15 ~ 5e-5 stays inside that margin, and
    the Adagrad and Adam states start at 1, which keeps g / (sqrt(state) +
    eps) no more sensitive than g;
  * a bf16 table: plus one bf16 ulp, 2**-7 * |w| -- each side rounds its own
    fp32 value once (to nearest, or stochastically with the same bits), and
    two fp32 values a hair apart can land on neighbouring bf16 values.
"""

import functools

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")

_LR = 0.125
_EPS = float(torch.tensor(1e-10, dtype=torch.float32))
_BETAS = (0.9, 0.999)
_SEED = 77

_SIZES = [(1, 3), (1, 1000), (5003, 3), (5003, 1000)]     # (n, vocab)
_WIDTHS = [8, 128]
_METHODS = ["sgd", "adagrad", "rowwise_adagrad", "lazy_adam"]
_TABLES = ["fp32", "bf16", "bf16_sr"]


def _ext():
    from distributed_embeddings_amd.ops import _backend
    return _backend.ops()


@functools.lru_cache(maxsize=None)
def _ids_case(n, vocab):
    """n ids over rows of 0..4 ids, about 2 % of them out of range on either
    side, and one fp32 weight per id.  Left unchanged by the tests."""
    g = torch.Generator().manual_seed(n * 7 + vocab)
    ids = torch.randint(0, vocab, (n,), generator=g)
    if n > 1:
        oob = torch.rand(n, generator=g) < 0.02
        low = torch.rand(n, generator=g) < 0.5
        ids = torch.where(oob, torch.where(low, -1 - ids, ids + vocab), ids)
        ids[n // 7], ids[n // 5], ids[n // 3] = -1, vocab + 2, vocab - 1
    lengths = []
    while sum(lengths) < n:
        lengths.append(min(int(torch.randint(0, 5, (1,), generator=g)),
                           n - sum(lengths)))
    lengths = torch.tensor(lengths + [0])                  # a trailing empty row
    splits = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)])
    per_id_w = 0.5 + torch.rand(n, generator=g)
    return {"ids": ids, "splits": splits, "per_id_w": per_id_w,
            "num_rows": lengths.numel(),
            "max_count": int(torch.bincount(ids[(ids >= 0) & (ids < vocab)],
                                            minlength=1).max())}


@functools.lru_cache(maxsize=None)
def _dense_case(num_rows, vocab, width):
    g = torch.Generator().manual_seed(num_rows + 3 * vocab + width)
    return (torch.randn(vocab, width, generator=g),
            torch.randn(num_rows, width, generator=g) * 2.0 ** -5)


class _Table:
    """Weight, optimizer state and counters of one method on one table type."""

    def __init__(self, method, table, vocab, width):
        w0 = _dense_case(0, vocab, width)[0]
        self.method = method
        self.weight = w0.to(torch.float32 if table == "fp32" else torch.bfloat16).cuda()
        self.sr = torch.tensor([_SEED, 5], device="cuda") if table == "bf16_sr" else None
        self.step = None
        if method == "sgd":
            self.state = torch.empty(0, device="cuda")
        elif method == "adagrad":
            self.state = torch.ones(vocab, width, device="cuda")
        elif method == "rowwise_adagrad":
            self.state = torch.ones(vocab, device="cuda")
        else:
            self.state = torch.stack([torch.zeros(vocab, width),
                                      torch.ones(vocab, width)]).cuda()
            self.step = torch.tensor([3], device="cuda")

    def _kw(self, deterministic):
        kw = {"sr": self.sr, "deterministic": deterministic}
        if self.step is not None:
            kw.update(adam_step=self.step, beta1=_BETAS[0], beta2=_BETAS[1])
        return kw

    def one_shot(self, ids, splits, grad, lr, mean, per_id_w, deterministic):
        _ext().csr_fused_optimizer_apply(
            self.weight, self.state, ids, splits, grad, lr, mean,
            "adagrad" in self.method, _EPS, per_id_w, **self._kw(deterministic))

    def planned(self, plan, grad, lr, deterministic):
        _ext().csr_fused_optimizer_apply_planned(
            self.weight, self.state, plan, grad, lr, "adagrad" in self.method,
            _EPS, **self._kw(deterministic))

    def counters(self):
        return (None if self.sr is None else self.sr.tolist(),
                None if self.step is None else self.step.tolist())


def _assert_same(a, b, exact, tag):
    """Tables a and b after the same updates: equal bits, or within the
    bound of the module docstring."""
    assert a.counters() == b.counters(), tag
    for what, x, y in (("weight", a.weight, b.weight), ("state", a.state, b.state)):
        if exact or x.numel() == 0:
            assert torch.equal(x, y), f"{what} differs: {tag}"
            continue
        x, y = x.double().cpu(), y.double().cpu()
        tol = 1e-3 + (2.0 ** -7 * y.abs() if a.weight.dtype == torch.bfloat16
                      and what == "weight" else 0.0)
        err = (x - y).abs()
        print(f"{what} {tag}: max err {float(err.max()):.3e}")
        assert bool((err <= tol).all()), f"{what} out of tolerance: {tag}"


def _variants():
    for n, vocab in _SIZES:
        for width in _WIDTHS:
            for mean in (False, True):
                for weighted in (False, True):
                    yield n, vocab, width, mean, weighted


def _inputs(n, vocab, width, weighted):
    c = _ids_case(n, vocab)
    grad = _dense_case(c["num_rows"], vocab, width)[1].cuda()
    per_id_w = c["per_id_w"].cuda() if weighted else None
    return c, c["ids"].cuda(), c["splits"].cuda(), grad, per_id_w


# ---------------------------------------------------------------------------
# 1. plan + planned apply == one-shot apply
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("table", _TABLES)
@pytest.mark.parametrize("method", _METHODS)
def test_planned_apply_equals_one_shot(method, table):
    ext = _ext()
    lr = torch.tensor([_LR], device="cuda")
    saw_long = False
    for deterministic in (True, False):
        for n, vocab, width, mean, weighted in _variants():
            c, ids, splits, grad, per_id_w = _inputs(n, vocab, width, weighted)
            exact = deterministic or c["max_count"] <= 128
            saw_long |= not exact
            a = _Table(method, table, vocab, width)
            b = _Table(method, table, vocab, width)
            before = a.counters()
            plan = ext.csr_sort_plan(ids, splits, vocab, mean, per_id_w)
            assert (plan.nnz, plan.num_rows, plan.vocab) == (n, c["num_rows"], vocab)
            assert (plan.sw is not None) == (mean or weighted)
            torch.cuda.synchronize()
            assert a.counters() == before, "the plan advanced a step"
            a.planned(plan, grad, lr, deterministic)
            b.one_shot(ids, splits, grad, lr, mean, per_id_w, deterministic)
            sr_step, adam_step = a.counters()
            if before[0] is not None:
                assert sr_step == [_SEED, before[0][1] + 1]
            if before[1] is not None:
                assert adam_step == [before[1][0] + 1]
            if n > 1:       # one small step need not move a bf16 weight
                w0 = _dense_case(0, vocab, width)[0].to(a.weight.dtype)
                assert not torch.equal(a.weight.cpu(), w0), "nothing was applied"
            _assert_same(a, b, exact,
                         f"{method} {table} det={deterministic} n={n} vocab={vocab} "
                         f"w={width} mean={mean} weighted={weighted}")
    assert saw_long, "no case took the atomic long path"


def test_id_cases_hold_what_the_tests_need():
    """Out-of-range ids of both kinds, a long segment at vocab 3 and none at
    vocab 1000.  Needs no GPU."""
    for n, vocab in _SIZES:
        c = _ids_case(n, vocab)
        assert c["ids"].numel() == n and int(c["splits"][-1]) == n
        assert c["splits"].numel() == c["num_rows"] + 1
        if n > 1:
            assert (c["ids"] < 0).any() and (c["ids"] >= vocab).any()
            assert (c["max_count"] > 128) == (vocab == 3)


# ---------------------------------------------------------------------------
# 2. the apply reads the plan only    3. the plan is not consumed
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("method", _METHODS)
def test_apply_reads_only_the_plan(method):
    ext = _ext()
    lr = torch.tensor([_LR], device="cuda")
    for table in ("fp32", "bf16_sr"):
        for n, vocab, width, mean, weighted in _variants():
            _, ids, splits, grad, per_id_w = _inputs(n, vocab, width, weighted)
            ids, splits = ids.clone(), splits.clone()
            a = _Table(method, table, vocab, width)
            b = _Table(method, table, vocab, width)
            b.one_shot(ids, splits, grad, lr, mean, per_id_w, True)
            plan = ext.csr_sort_plan(ids, splits, vocab, mean, per_id_w)
            if per_id_w is not None:
                assert plan.sw.data_ptr() != per_id_w.data_ptr()
            kept = [t.clone() for t in (plan.sorted_ids, plan.srow, plan.seg,
                                        plan.unique_ids, plan.num_unique, plan.bounds)]
            ids.fill_(2 ** 40 + 1)
            splits.fill_(-7)
            if per_id_w is not None:      # the very tensor the plan was given
                per_id_w.fill_(float("nan"))
            a.planned(plan, grad, lr, True)
            tag = f"{method} {table} n={n} vocab={vocab} w={width} mean={mean} weighted={weighted}"
            _assert_same(a, b, True, tag)
            for was, now in zip(kept, (plan.sorted_ids, plan.srow, plan.seg,
                                       plan.unique_ids, plan.num_unique, plan.bounds)):
                assert torch.equal(was, now), f"the apply wrote into the plan: {tag}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("method", _METHODS)
def test_plan_applies_twice(method):
    ext = _ext()
    lr = torch.tensor([_LR], device="cuda")
    for table in ("fp32", "bf16_sr"):
        for n, vocab, width, mean, weighted in _variants():
            _, ids, splits, grad, per_id_w = _inputs(n, vocab, width, weighted)
            a = _Table(method, table, vocab, width)
            b = _Table(method, table, vocab, width)
            plan = ext.csr_sort_plan(ids, splits, vocab, mean, per_id_w)
            for _ in range(2):
                a.planned(plan, grad, lr, True)
                b.one_shot(ids, splits, grad, lr, mean, per_id_w, True)
            _assert_same(a, b, True, f"{method} {table} n={n} vocab={vocab} w={width} "
                                     f"mean={mean} weighted={weighted}")


# ---------------------------------------------------------------------------
# 4. empty and degenerate inputs
# ---------------------------------------------------------------------------

_DEGENERATE = {
    "no_ids": ([], [0, 0, 0]),
    "no_rows": ([], [0]),
    "single_row": ([2, 0, 2, 9, -1], [0, 5]),
    "all_out_of_range": ([-1, 7, 9, -3, 2 ** 40], [0, 2, 2, 5]),
}


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("case", sorted(_DEGENERATE))
@pytest.mark.parametrize("method", _METHODS)
def test_degenerate_inputs(method, case):
    ext = _ext()
    vocab, width = 7, 8
    ids, splits = (torch.tensor(v, dtype=torch.int64).cuda() for v in _DEGENERATE[case])
    num_rows = splits.numel() - 1
    lr = torch.tensor([_LR], device="cuda")
    grad = torch.ones(max(num_rows, 0), width, device="cuda")
    for table in _TABLES:
        for deterministic in (False, True):
            a = _Table(method, table, vocab, width)
            b = _Table(method, table, vocab, width)
            w0 = a.weight.clone()
            before = a.counters()
            plan = ext.csr_sort_plan(ids, splits, vocab, False, None)
            a.planned(plan, grad, lr, deterministic)
            b.one_shot(ids, splits, grad, lr, False, None, deterministic)
            torch.cuda.synchronize()
            _assert_same(a, b, True, f"{method} {table} {case}")
            if case == "single_row":
                assert not torch.equal(a.weight, w0)
                touched = torch.tensor([0, 2], device="cuda")
                w0[touched] = a.weight[touched]
            elif ids.numel() == 0:
                assert plan.sorted_ids is None and plan.nnz == 0
                assert a.counters() == before, "an empty apply advanced a step"
            assert torch.equal(a.weight, w0), f"{method} {table} {case}"


@pytest.mark.gpu
@requires_gpu
def test_planned_apply_rejects_a_plan_of_another_shape():
    ext = _ext()
    ids = torch.tensor([1, 2, 3], device="cuda")
    splits = torch.tensor([0, 1, 3], device="cuda")
    lr = torch.tensor([_LR], device="cuda")
    state = torch.empty(0, device="cuda")
    plan = ext.csr_sort_plan(ids, splits, 10, False, None)
    with pytest.raises(RuntimeError):           # the weight has fewer rows
        ext.csr_fused_optimizer_apply_planned(
            torch.zeros(4, 8, device="cuda"), state, plan,
            torch.zeros(2, 8, device="cuda"), lr, False, 0.0)
    with pytest.raises(RuntimeError):           # srow would run past grad_out
        ext.csr_fused_optimizer_apply_planned(
            torch.zeros(10, 8, device="cuda"), state, plan,
            torch.zeros(1, 8, device="cuda"), lr, False, 0.0)


@pytest.mark.gpu
@requires_gpu
def test_one_shot_checks_before_it_launches():
    """A bad argument of the apply half raises, and the shape of grad_out is
    checked, in the one-shot call too."""
    ext = _ext()
    ids = torch.tensor([1, 2, 3], device="cuda")
    splits = torch.tensor([0, 1, 3], device="cuda")
    lr = torch.tensor([_LR], device="cuda")
    weight = torch.ones(10, 8, device="cuda")
    with pytest.raises(RuntimeError):           # one row of grad_out for two rows
        ext.csr_fused_optimizer_apply(weight, torch.empty(0, device="cuda"), ids, splits,
                                      torch.ones(1, 8, device="cuda"), lr, False, False, 0.0)
    with pytest.raises(RuntimeError):           # Adagrad state of another shape
        ext.csr_fused_optimizer_apply(weight, torch.ones(3, 8, device="cuda"), ids, splits,
                                      torch.ones(2, 8, device="cuda"), lr, False, True, 0.0)
    torch.cuda.synchronize()
    assert bool((weight == 1.0).all())


# ---------------------------------------------------------------------------
# 5. the hoisted path end to end
# ---------------------------------------------------------------------------

_DLRM_SIZES = [300, 200, 411, 257]
_DLRM_BATCH = 256
_DLRM_STEPS = 3
_DLRM_WARMUP = 2


@functools.lru_cache(maxsize=None)
def _dlrm_batches():
    g = torch.Generator().manual_seed(5)
    return [(torch.rand(_DLRM_BATCH, 4, generator=g),
             [torch.randint(0, s, (_DLRM_BATCH,), generator=g) for s in _DLRM_SIZES],
             torch.randint(0, 2, (_DLRM_BATCH, 1), generator=g).float())
            for _ in range(_DLRM_STEPS + 1)]


def _count_builds(monkeypatch):
    import importlib
    # the package exports a function of the module's name
    el = importlib.import_module("distributed_embeddings_amd.ops.embedding_lookup")
    built = []
    real = el.SortPlanCollector.build

    def build(self):
        built.append(real(self))
        return built[-1]
    monkeypatch.setattr(el.SortPlanCollector, "build", build)
    return built


def _run_dlrm(monkeypatch, hoist, graph, method, width, train=True):
    """Two eager steps on batch 0, then one step on each of batches 1..3,
    eager or as replays of one captured step with refilled static inputs.
    Returns (parameters and buffers, the logits of the three steps, how many
    plans each build() launched)."""
    from distributed_embeddings_amd.models.dlrm import DLRM
    from distributed_embeddings_amd.ops import deterministic
    from distributed_embeddings_amd.parallel.optim import SparseEmbeddingOptimizer
    monkeypatch.setenv("DE_HOIST_SORT", "1" if hoist else "0")
    built = _count_builds(monkeypatch)
    with deterministic(True):
        torch.manual_seed(11)
        with torch.device("cuda"):
            model = DLRM(_DLRM_SIZES, embedding_dim=width, bottom_mlp_dims=(32, width),
                         top_mlp_dims=(32, 1), num_numerical=4)
        opt = SparseEmbeddingOptimizer(model.parameters(), lr=0.05, method="sgd")
        model.embeddings.enable_fused_optimizer(method, 0.05)
        model.train(train)
        batches = [(n.cuda(), [c.cuda() for c in cats], y.cuda())
                   for n, cats, y in _dlrm_batches()]
        loss_fn = torch.nn.BCEWithLogitsLoss()

        def step(num, cats, labels):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                logits = model(num, cats)
            if train:
                opt.zero_grad(set_to_none=False)
                loss_fn(logits.float(), labels).backward()
                opt.step()
            return logits

        for _ in range(_DLRM_WARMUP):
            step(*batches[0])
        assert model._emb_stream is not None, "the side-stream branch did not run"
        logits = []
        if graph:
            s_num, s_cats, s_labels = (batches[0][0].clone(),
                                       [c.clone() for c in batches[0][1]],
                                       batches[0][2].clone())
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                s_out = step(s_num, s_cats, s_labels)
            for num, cats, labels in batches[1:]:
                s_num.copy_(num)
                for dst, src in zip(s_cats, cats):
                    dst.copy_(src)
                s_labels.copy_(labels)
                g.replay()
                logits.append(s_out.detach().clone())
        else:
            for b in batches[1:]:
                logits.append(step(*b).detach().clone())
        torch.cuda.synchronize()
        tensors = {k: v.detach().clone() for k, v in model.state_dict().items()}
        return tensors, logits, list(built)


def _assert_runs_equal(a, b, tag):
    assert a[0].keys() == b[0].keys()
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), f"{k} differs: {tag}"
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert torch.equal(x, y), f"logits of step {i} differ: {tag}"


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("width", [16, 128])
@pytest.mark.parametrize("method", ["sgd", "adagrad"])
def test_dlrm_hoisted_equals_unhoisted(monkeypatch, method, width):
    off = _run_dlrm(monkeypatch, False, False, method, width)
    on = _run_dlrm(monkeypatch, True, False, method, width)
    assert off[2] == [] and len(on[2]) == _DLRM_WARMUP + _DLRM_STEPS
    assert all(n >= 1 for n in on[2]), "the forward built no plan"
    initial = _run_dlrm(monkeypatch, True, False, method, width, train=False)[0]
    moved = [k for k in on[0] if not torch.equal(on[0][k], initial[k])]
    assert any("embeddings" in k for k in moved) and any("mlp" in k for k in moved), moved
    _assert_runs_equal(on, off, f"eager {method} w{width}")
    # captured once, replayed on three other batches: every replay sorts anew
    on_graph = _run_dlrm(monkeypatch, True, True, method, width)
    assert len(on_graph[2]) == _DLRM_WARMUP + 1
    _assert_runs_equal(on_graph, on, f"graph on {method} w{width}")
    off_graph = _run_dlrm(monkeypatch, False, True, method, width)
    _assert_runs_equal(off_graph, on, f"graph off {method} w{width}")


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("graph", [False, True])
def test_dlrm_eval_builds_no_plan(monkeypatch, graph):
    off = _run_dlrm(monkeypatch, False, graph, "sgd", 128, train=False)
    on = _run_dlrm(monkeypatch, True, graph, "sgd", 128, train=False)
    assert sum(on[2]) == 0, "an evaluation forward built a sort plan"
    _assert_runs_equal(on, off, f"eval graph={graph}")
    assert not torch.equal(on[1][0], on[1][1])


# ---------------------------------------------------------------------------
# 6. CPU: the collector changes nothing
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("method", ["sgd", "adagrad"])
def test_collector_is_inert_on_cpu(method):
    from distributed_embeddings_amd import Embedding
    from distributed_embeddings_amd.ops import Ragged, hoisted_sort_plans
    c = _ids_case(5003, 1000)
    ids = c["ids"].clamp(0, 999)             # the CPU gather takes no stray ids
    up = _dense_case(c["num_rows"], 1000, 8)[1]
    outs = []
    for hoisted in (False, True):
        torch.manual_seed(3)
        e = Embedding(1000, 8, combiner="sum")
        e.enable_fused_optimizer(method, 0.1)
        w0 = e.weight.detach().clone()
        if hoisted:
            with hoisted_sort_plans() as plans:
                out = e(Ragged(ids, c["splits"]))
                assert plans.slots == [] and plans.build() == 0
        else:
            out = e(Ragged(ids, c["splits"]))
        out.backward(up)
        outs.append((out.detach().clone(), e.weight.detach().clone()))
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[1][1], w0)
