"""Deterministic mode of the long-segment lookup paths.

With the mode on (``set_deterministic`` / ``deterministic()`` /
``DE_DETERMINISTIC=1``) a segment of more than LONG_T = 128 ids -- a long bag
of the forward, a hot id of the sparse backward and of the fused optimizers --
is reduced chunk by chunk into slab rows that are then added in a fixed order
(docs/KERNELS.md, "Deterministic mode"): with p_c the partial of 128-id chunk
c and G = 64,

    S_g = ((p_{gG} + p_{gG+1}) + ...)   left to right over group g's chunks
    t   = ((S_0 + S_1) + ...)           left to right over the groups

in fp32; up to 64 chunks that is the plain left-to-right sum of the partials.

Shapes: vocab 50, fewer than 4096 row-waves everywhere, so the threshold is
128.  Forward bags of lengths [3, 129, 0, 257, 128, 1000, 1] with an
out-of-range and a negative id inside long bags; backward and fused inputs of
175 bags of 4 ids in which one id occurs 300 times, one 129 times, one exactly
128 times and the rest a few times each.  Widths 8, 32, 64 (narrow tiles), 65
(VEC 1), 130 (VEC 2), 128 and 260 (VEC 4; 260 takes the column loop).

Tolerances.  The exact-arithmetic tests use small integers (times a power of
two), so every fp32 sum and every SGD update with lr = 2**-3 is exact in any
order and has to equal the CPU path's bit for bit.  `mean` forwards multiply
each chunk partial by fl(1/len): two roundings per partial and one per add,
so they are held to (chunks + 3) * 2**-24 * sum_k |w_k x_k| / len.  Adagrad
and row-wise Adagrad are held to _terms_atol(counts) of test_gpu.py and lazy
Adam to _tols of test_lazy_adam.py, the bounds of those rules' own tests; a
bf16 table adds 2**-8 * |w_ref|, one rounding.  Random-float sums are held to
n * 2**-24 * sum_i |t_i| against float64, the first-order bound of any fixed
order of n terms (n + 1 where the terms are rounded products w_k * x_k).
"""

import os
import subprocess
import sys

import pytest
import torch

from test_gpu import _HELPER_VOCAB, _assert_within, _helper_case, _terms_atol
from test_lazy_adam import (_B1, _B2, _V_LO, _a_t, _adam_step, _prefill,
                            _tols)

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VOCAB = 50
assert VOCAB == _HELPER_VOCAB  # _prefill's state shape
WIDTHS = [8, 32, 64, 65, 128, 130, 260]
WIDE = [128, 130, 65, 260]
LONG_T, SLAB_G = 128, 64
FWD_LENGTHS = [3, 129, 0, 257, 128, 1000, 1]
HOT, HOT129, HOT128 = 7, 11, 13
U = 2.0 ** -24
LR = 2.0 ** -3
RULES = ["sgd", "adagrad", "rowwise_adagrad", "lazy_adam"]


def _ops():
    # the package re-exports the function of the same name over the module
    import importlib
    return importlib.import_module(
        "distributed_embeddings_amd.ops.embedding_lookup")


def _ext():
    from distributed_embeddings_amd.ops import _backend
    return _backend.ops()


# --------------------------------------------------------------------------
# Inputs
# --------------------------------------------------------------------------

def _splits(lengths):
    lengths = torch.as_tensor(lengths, dtype=torch.long)
    return torch.cat([torch.zeros(1, dtype=torch.long), lengths.cumsum(0)])


def _fwd_ids(seed=11):
    """ids and splits of FWD_LENGTHS; -1 and VOCAB sit inside the bags of 257
    and of 1000 ids, in different chunks."""
    g = torch.Generator().manual_seed(seed)
    splits = _splits(FWD_LENGTHS)
    ids = torch.randint(0, VOCAB, (int(splits[-1]),), generator=g)
    s257, s1000 = int(splits[3]), int(splits[5])
    ids[s257 + 5] = -1
    ids[s257 + 200] = VOCAB
    ids[s1000 + 127] = VOCAB + 3
    ids[s1000 + 128] = -7
    ids[s1000 + 999] = VOCAB
    return ids, splits


def _int_table(width, seed=0):
    g = torch.Generator().manual_seed(1000 + width + seed)
    return torch.randint(-4, 5, (VOCAB, width), generator=g).float()


def _int_weights(n, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-2, 3, (n,), generator=g).float()


def _bwd_ids(seed=3):
    """700 ids as 175 bags of 4: HOT 300 times, HOT129 129 times, HOT128 128
    times, 141 draws of the other ids and one -1 and one VOCAB, shuffled."""
    g = torch.Generator().manual_seed(seed)
    others = torch.tensor([i for i in range(VOCAB)
                           if i not in (HOT, HOT129, HOT128)])
    rest = others[torch.randint(0, others.numel(), (141,), generator=g)]
    ids = torch.cat([torch.full((300,), HOT), torch.full((129,), HOT129),
                     torch.full((128,), HOT128), rest,
                     torch.tensor([-1, VOCAB])])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    assert ids.numel() == 700
    return ids, torch.arange(0, 701, 4)


def _int_grad(rows, width, seed=0):
    """integers in [-2, 2] times 2**-6: exact in bf16, and a 300-fold sum of
    them, weighted by integers in [-2, 2] and by 1/4, is exact in fp32."""
    g = torch.Generator().manual_seed(2000 + width + seed)
    return torch.randint(-2, 3, (rows, width), generator=g).float() * 2.0 ** -6


def _state_for(rule, width):
    if rule == "sgd":
        return torch.empty(0)
    if rule == "lazy_adam":
        return _prefill(width)
    g = torch.Generator().manual_seed(77 + width)
    shape = (VOCAB, width) if rule == "adagrad" else (VOCAB,)
    return torch.rand(shape, generator=g) + 0.5


def _fused_step(rule, table, state, ids, splits, grad, combiner, w=None,
                sr=None, t0=4, eps=1e-8):
    """One fused step through the public autograd function, on the tensors'
    device, in the current mode.  Returns (weight, state, step)."""
    ops = _ops()
    dev = table.device
    weight = table.clone().requires_grad_(True)
    state = state.clone()
    lr = torch.tensor([LR], device=dev)
    step = torch.tensor([t0], device=dev)
    adam = (step, _B1, _B2) if rule == "lazy_adam" else None
    # a bf16 output hands the kernels a bf16 upstream gradient
    out_dtype = torch.bfloat16 if grad.dtype == torch.bfloat16 else None
    out = ops.csr_lookup_fused_optimizer(
        weight, ids, splits, combiner, lr, state,
        rule in ("adagrad", "rowwise_adagrad"), eps, out_dtype, w, sr, adam)
    assert out.dtype == grad.dtype
    out.backward(grad)
    return weight.detach(), state, step


def _ordered_sum(partials):
    """The documented order over the [chunks, width] fp32 partials."""
    groups = []
    for g0 in range(0, partials.shape[0], SLAB_G):
        t = partials[g0].clone()
        for p in partials[g0 + 1:g0 + SLAB_G]:
            t = t + p
        groups.append(t)
    t = groups[0]
    for s in groups[1:]:
        t = t + s
    return t


# --------------------------------------------------------------------------
# 1. Flag plumbing (CPU)
# --------------------------------------------------------------------------

def test_flag_api_and_context_manager():
    import distributed_embeddings_amd as de
    ops = _ops()
    assert de.set_deterministic is ops.set_deterministic
    assert de.is_deterministic is ops.is_deterministic
    assert de.deterministic is ops.deterministic
    before = de.is_deterministic()
    try:
        de.set_deterministic(False)
        assert de.is_deterministic() is False
        with de.deterministic():
            assert de.is_deterministic() is True
            with de.deterministic(False):
                assert de.is_deterministic() is False
            assert de.is_deterministic() is True
        assert de.is_deterministic() is False
        with pytest.raises(RuntimeError):
            with de.deterministic():
                raise RuntimeError("leaves the block")
        assert de.is_deterministic() is False
        de.set_deterministic(True)
        with de.deterministic(False):
            assert de.is_deterministic() is False
        assert de.is_deterministic() is True
    finally:
        de.set_deterministic(before)


@pytest.mark.parametrize("value,expected", [("1", True), ("0", False),
                                            (None, False)])
def test_env_switch_in_fresh_process(value, expected):
    env = {k: v for k, v in os.environ.items() if k != "DE_DETERMINISTIC"}
    if value is not None:
        env["DE_DETERMINISTIC"] = value
    code = ("import sys; sys.path.insert(0, %r); "
            "import distributed_embeddings_amd as de; "
            "print(de.is_deterministic())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, check=True,
                         capture_output=True, text=True).stdout
    assert out.strip() == str(expected)


@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_cpu_paths_ignore_the_flag(combiner):
    import distributed_embeddings_amd as de
    ops = _ops()
    g = torch.Generator().manual_seed(1)
    table = torch.randn(VOCAB, 16, generator=g)
    ids, splits = _fwd_ids()
    w = torch.randn(ids.numel(), generator=g)
    bids, bsplits = _bwd_ids()
    grad = torch.randn(175, 16, generator=g)

    def run():
        res = []
        for pw in (None, w):
            wt = table.clone().requires_grad_(True)
            out = de.embedding_lookup(wt, de.Ragged(ids, splits, pw), combiner)
            out.backward(torch.ones_like(out))
            gw = wt.grad.coalesce()
            res += [out.detach(), gw.indices(), gw.values()]
        for rule in RULES:
            res += list(_fused_step(rule, table, _state_for(rule, 16), bids,
                                    bsplits, grad, combiner))
        return res

    with de.deterministic(False):
        off = run()
    with de.deterministic(True):
        on = run()
    assert len(on) == len(off)
    for a, b in zip(on, off):
        assert torch.equal(a, b)


# --------------------------------------------------------------------------
# 2. Exact arithmetic (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_exact_forward(width):
    ops, ext = _ops(), _ext()
    ids, splits = _fwd_ids()
    lengths = splits[1:] - splits[:-1]
    chunks = (lengths + LONG_T - 1) // LONG_T
    pw = _int_weights(ids.numel())
    for tdt in (torch.float32, torch.bfloat16):
        table = _int_table(width).to(tdt)
        for w in (None, pw):
            for combiner in ("sum", "mean"):
                tag = f"w{width} {tdt} weighted={w is not None} {combiner}"
                ref = ops._csr_lookup_ref(table, ids, splits, combiner, w)
                out = ext.csr_lookup_forward(
                    table.cuda(), ids.cuda(), splits.cuda(),
                    combiner == "mean", False,
                    None if w is None else w.cuda(), deterministic=True)
                if combiner == "sum":
                    assert torch.equal(out.cpu(), ref), tag
                    continue
                mag = ops._csr_lookup_ref(table.float().abs(), ids, splits,
                                          "mean", None if w is None else w.abs())
                tol = (chunks.double().unsqueeze(1) + 3) * U * mag.double()
                _assert_within(tag, out, ref, tol)
                assert torch.equal(out.cpu()[2], torch.zeros(width)), tag


@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_exact_sparse_backward(width):
    ops, ext = _ops(), _ext()
    ids, splits = _bwd_ids()
    pw = _int_weights(ids.numel())
    for gdt in (torch.float32, torch.bfloat16):
        grad = _int_grad(175, width).to(gdt)
        for w in (None, pw):
            for combiner in ("sum", "mean"):
                tag = f"w{width} {gdt} weighted={w is not None} {combiner}"
                uid_ref, ug_ref = ops._csr_lookup_backward_ref(
                    grad.float(), ids, splits, VOCAB, combiner, w)
                uid, ug = ext.csr_lookup_backward(
                    grad.cuda(), ids.cuda(), splits.cuda(), VOCAB,
                    combiner == "mean", None if w is None else w.cuda(),
                    deterministic=True)
                assert torch.equal(uid.cpu(), uid_ref), tag
                assert torch.equal(ug.cpu(), ug_ref), tag


@gpu
@requires_gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("width", WIDTHS)
def test_exact_fused_update(width, rule):
    import distributed_embeddings_amd as de
    ids, splits = _bwd_ids()
    counts = torch.bincount(ids[(ids >= 0) & (ids < VOCAB)], minlength=VOCAB)
    touched = counts > 0
    tol_g = _terms_atol(counts)
    pw = _int_weights(ids.numel())
    table, st0 = _int_table(width), _state_for(rule, width)
    for gdt in (torch.float32, torch.bfloat16):
        grad = _int_grad(175, width).to(gdt)
        for w in (None, pw):
            for combiner in ("sum", "mean"):
                w_ref, st_ref, _ = _fused_step(rule, table, st0, ids, splits,
                                               grad.float(), combiner, w)
                for tdt in (torch.float32, torch.bfloat16):
                    tag = (f"{rule} w{width} {tdt} {gdt} "
                           f"weighted={w is not None} {combiner}")
                    with de.deterministic():
                        w_gpu, st_gpu, step = _fused_step(
                            rule, table.to(tdt).cuda(), st0.cuda(), ids.cuda(),
                            splits.cuda(), grad.cuda(), combiner,
                            None if w is None else w.cuda())
                    one_rounding = (2.0 ** -8 * w_ref.abs().double()
                                    if tdt == torch.bfloat16 else 0.0)
                    if rule == "sgd" and tdt == torch.float32:
                        assert torch.equal(w_gpu.cpu(), w_ref), tag
                    elif rule == "sgd":
                        _assert_within(tag, w_gpu.float(), w_ref,
                                       one_rounding + torch.zeros(1, 1).double())
                    elif rule == "lazy_adam":
                        assert step.tolist() == [5]
                        uid, ug = _ops()._csr_lookup_backward_ref(
                            grad.float(), ids, splits, VOCAB, combiner, w)
                        g_ref = torch.zeros(VOCAB, width, dtype=torch.float64)
                        g_ref[uid] = ug.double()
                        # as in test_lazy_adam.py: the formula in float64 on
                        # the (here exact) summed gradient
                        w64, m64, v64 = _adam_step(table, st0[0], st0[1],
                                                   g_ref, touched, LR, 1e-8, 5)
                        assert float(v64[touched].min()) >= _V_LO
                        tol_m, tol_v, tol_w = _tols(g_ref, m64, tol_g,
                                                    _a_t(LR, 5))
                        _assert_within(f"cpu w {tag}", w_ref, w64, tol_w)
                        _assert_within(f"w {tag}", w_gpu.float(), w64,
                                       tol_w + 2.0 ** -8 * w64.abs()
                                       * (tdt == torch.bfloat16))
                        _assert_within(f"m {tag}", st_gpu[0], m64, tol_m)
                        _assert_within(f"v {tag}", st_gpu[1], v64, tol_v)
                    else:
                        st_tol = tol_g if st_ref.dim() == 2 else tol_g[:, 0]
                        _assert_within(f"w {tag}", w_gpu.float(), w_ref,
                                       tol_g + one_rounding)
                        _assert_within(f"state {tag}", st_gpu, st_ref, st_tol)
                    keep = ~touched
                    assert torch.equal(w_gpu.cpu()[keep],
                                       table.to(tdt)[keep]), tag


# --------------------------------------------------------------------------
# 3. The defined order, wide widths (GPU)
# --------------------------------------------------------------------------

def _chunk_partials(ext, src, values, n):
    """[chunks, width]: the first n of `values` looked up 128 at a time as
    separate short bags -- kernel A's in-register wide_accumulate."""
    splits = torch.cat([torch.arange(0, n, LONG_T), torch.tensor([n])])
    return ext.csr_lookup_forward(src, values[:n].contiguous(), splits.cuda(),
                                  False, False, None)


@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDE)
@pytest.mark.parametrize("length", [300, 1000, 130 * LONG_T + 17])
def test_forward_follows_the_documented_order(width, length):
    """300 and 1000 ids: one group, the plain chunk-order sum.  16657 ids: 131
    chunks, three groups of 64, 64 and 3."""
    ext = _ext()
    g = torch.Generator().manual_seed(width + length)
    table = torch.randn(VOCAB, width, generator=g).cuda()
    ids = torch.randint(0, VOCAB, (5 + length,), generator=g)
    ids[5 + 77], ids[5 + 128], ids[5 + length - 1] = -1, VOCAB, VOCAB + 1
    ids = ids.cuda()
    splits = torch.tensor([0, 5, 5 + length]).cuda()
    out = ext.csr_lookup_forward(table, ids, splits, False, False, None,
                                 deterministic=True)
    partials = _chunk_partials(ext, table, ids[5:], length)
    assert partials.shape[0] == (length + LONG_T - 1) // LONG_T
    assert torch.equal(out[1], _ordered_sum(partials))
    assert torch.equal(out[0], _chunk_partials(ext, table, ids, 5)[0])


@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDE)
def test_sparse_backward_follows_the_documented_order(width):
    """The hot id's 300 gradient rows in position order -- the stable sort's
    order -- 128 at a time."""
    ext = _ext()
    ids, splits = _bwd_ids()
    g = torch.Generator().manual_seed(width)
    grad = torch.randn(175, width, generator=g).cuda()
    uid, ug = ext.csr_lookup_backward(grad, ids.cuda(), splits.cuda(), VOCAB,
                                      False, None, deterministic=True)
    for hot, n in ((HOT, 300), (HOT129, 129)):
        rows = (torch.nonzero(ids == hot).flatten() // 4).cuda()
        assert rows.numel() == n
        partials = _chunk_partials(ext, grad, rows, n)
        got = ug[torch.nonzero(uid == hot).flatten()[0]]
        assert torch.equal(got, _ordered_sum(partials)), hot


# --------------------------------------------------------------------------
# 4. Random floats against float64; 6. the bf16-out long split (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_forward_random_floats_vs_fp64(width):
    ext = _ext()
    ids, splits = _fwd_ids()
    lengths = (splits[1:] - splits[:-1]).double().unsqueeze(1)
    seg = torch.repeat_interleave(torch.arange(len(FWD_LENGTHS)),
                                  splits[1:] - splits[:-1])
    g = torch.Generator().manual_seed(width)
    pw = torch.rand(ids.numel(), generator=g) * 3 - 1.5
    valid = ((ids >= 0) & (ids < VOCAB)).double().unsqueeze(1)
    for tdt in (torch.float32, torch.bfloat16):
        table = torch.randn(VOCAB, width, generator=g).to(tdt)
        rows = table.double()[ids.clamp(0, VOCAB - 1)] * valid
        for w in (None, pw):
            terms = rows if w is None else rows * w.double().unsqueeze(1)
            ref = torch.zeros(len(FWD_LENGTHS), width, dtype=torch.float64)
            ref.index_add_(0, seg, terms)
            mag = torch.zeros_like(ref).index_add_(0, seg, terms.abs())
            n = lengths + (0 if w is None else 1)
            for combiner in ("sum", "mean"):
                # mean: one more rounding for fl(1/len), one for the product
                c = 1.0 / lengths.clamp(min=1) if combiner == "mean" else 1.0
                extra = 2 if combiner == "mean" else 0
                tag = f"w{width} {tdt} weighted={w is not None} {combiner}"
                args = (table.cuda(), ids.cuda(), splits.cuda(),
                        combiner == "mean")
                wc = None if w is None else w.cuda()
                out = ext.csr_lookup_forward(*args, False, wc,
                                             deterministic=True)
                _assert_within(tag, out, c * ref, (n + extra) * U * c * mag)
                assert torch.equal(out.cpu()[2], torch.zeros(width)), tag
                # bf16 out: the RNE rounding of the deterministic fp32 result,
                # long bags included (they are split, not reduced in-register)
                out_bf = ext.csr_lookup_forward(*args, True, wc,
                                                deterministic=True)
                assert out_bf.dtype == torch.bfloat16
                assert torch.equal(out_bf, out.bfloat16()), tag
                # and within one bf16 rounding of the default in-register path
                dflt = ext.csr_lookup_forward(*args, True, wc)
                _assert_within(f"bf16 out {tag}", out_bf.float(), c * ref,
                               (n + extra) * U * c * mag
                               + 2.0 ** -8 * (c * ref).abs())
                _assert_within(f"det vs default bf16 {tag}", out_bf.float(),
                               dflt.float().cpu(),
                               2 * (n + extra) * U * c * mag
                               + 2.0 ** -7 * (c * ref).abs())


@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_sparse_backward_random_floats_vs_fp64(width):
    ext = _ext()
    ids, splits = _bwd_ids()
    g = torch.Generator().manual_seed(width)
    pw = torch.rand(ids.numel(), generator=g) * 3 - 1.5
    ok = (ids >= 0) & (ids < VOCAB)
    counts = torch.bincount(ids[ok], minlength=VOCAB).double().unsqueeze(1)
    for gdt in (torch.float32, torch.bfloat16):
        grad = torch.randn(175, width, generator=g).to(gdt)
        for w in (None, pw):
            for combiner in ("sum", "mean"):
                tag = f"w{width} {gdt} weighted={w is not None} {combiner}"
                coef = torch.full((700,), 0.25 if combiner == "mean" else 1.0,
                                  dtype=torch.float64)
                if w is not None:
                    coef = coef * w.double()
                terms = (grad.double()[torch.arange(700) // 4]
                         * coef.unsqueeze(1))[ok]
                ref = torch.zeros(VOCAB, width, dtype=torch.float64)
                ref.index_add_(0, ids[ok], terms)
                mag = torch.zeros_like(ref).index_add_(0, ids[ok], terms.abs())
                uid, ug = ext.csr_lookup_backward(
                    grad.cuda(), ids.cuda(), splits.cuda(), VOCAB,
                    combiner == "mean", None if w is None else w.cuda(),
                    deterministic=True)
                uid = uid.cpu()
                assert torch.equal(uid, torch.nonzero(counts[:, 0]).flatten())
                # products w_k * g_k are rounded: n + 1 (mean alone scales by
                # the exact 1/4)
                n = counts[uid] + (0 if w is None else 1)
                _assert_within(tag, ug, ref[uid], n * U * mag[uid])


# --------------------------------------------------------------------------
# 5. Bits depend on the segment only (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_forward_bits_depend_on_the_bag_only(width):
    ext = _ext()
    g = torch.Generator().manual_seed(width)
    table = torch.randn(VOCAB, width, generator=g).cuda()
    bag = torch.randint(0, VOCAB, (1000,), generator=g)
    bag_w = torch.rand(1000, generator=g) * 3 - 1.5
    filler = [int(x) for x in torch.randint(0, 200, (59,), generator=g)]
    layouts = [([3, 1000], 1), (filler[:30] + [1000] + filler[30:], 30)]
    for weighted in (False, True):
        for mean in (False, True):
            rows = []
            for lengths, at in layouts:
                splits = _splits(lengths)
                ids = torch.randint(0, VOCAB, (int(splits[-1]),), generator=g)
                w = torch.rand(ids.numel(), generator=g)
                ids[splits[at]:splits[at + 1]] = bag
                w[splits[at]:splits[at + 1]] = bag_w
                out = ext.csr_lookup_forward(
                    table, ids.cuda(), splits.cuda(), mean, False,
                    w.cuda() if weighted else None, deterministic=True)
                rows.append(out[at])
            assert torch.equal(rows[0], rows[1]), (width, weighted, mean)


@gpu
@requires_gpu
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("width", [32, 65, 128, 260])
def test_fused_bits_depend_on_the_hot_id_only(width, rule):
    """The hot id's 300 occurrences keep their relative order and gradient
    rows; the foreign ids between them differ in number and value."""
    import distributed_embeddings_amd as de
    g = torch.Generator().manual_seed(width)
    table = torch.randn(VOCAB, width, generator=g)
    st0 = _state_for(rule, width)
    hot_grad = torch.randn(300, width, generator=g)
    results = []
    for n_foreign in (150, 420):
        n = 300 + n_foreign
        where = torch.randperm(n, generator=g)[:300].sort().values
        ids = torch.randint(HOT + 1, VOCAB, (n,), generator=g)
        ids[where] = HOT
        grad = torch.randn(n, width, generator=g)
        grad[where] = hot_grad
        with de.deterministic():
            w, st, _ = _fused_step(rule, table.cuda(), st0.cuda(), ids.cuda(),
                                   torch.arange(n + 1).cuda(), grad.cuda(),
                                   "sum")
        hot_state = st[:, HOT] if rule == "lazy_adam" else st[HOT:HOT + 1]
        results.append((w[HOT], hot_state))
    assert torch.equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])
    assert not torch.equal(results[0][0].cpu(), table[HOT])


@gpu
@requires_gpu
@pytest.mark.parametrize("width", [8, 65, 128, 260])
def test_five_runs_agree_bitwise(width):
    import distributed_embeddings_amd as de
    ext = _ext()
    g = torch.Generator().manual_seed(width)
    table = torch.randn(VOCAB, width, generator=g).cuda()
    fids, fsplits = (x.cuda() for x in _fwd_ids())
    fw = torch.rand(fids.numel(), generator=g).cuda()
    bids, bsplits = (x.cuda() for x in _bwd_ids())
    bw = torch.rand(700, generator=g).cuda()
    grad = torch.randn(175, width, generator=g).cuda()

    def once():
        res = [ext.csr_lookup_forward(table, fids, fsplits, True, bf16, fw,
                                      deterministic=True)
               for bf16 in (False, True)]
        res += ext.csr_lookup_backward(grad, bids, bsplits, VOCAB, True, bw,
                                       deterministic=True)
        with de.deterministic():
            for rule in RULES:
                for tdt in (torch.float32, torch.bfloat16):
                    res += _fused_step(rule, table.to(tdt),
                                       _state_for(rule, width).cuda(), bids,
                                       bsplits, grad, "mean", bw)
                sr = torch.tensor([1234, 7], device="cuda")
                res += _fused_step(rule, table.bfloat16(),
                                   _state_for(rule, width).cuda(), bids,
                                   bsplits, grad, "mean", bw, sr)
                assert sr.tolist() == [1234, 8]
        return res

    first = once()
    for _ in range(4):
        for a, b in zip(first, once()):
            assert torch.equal(a, b)


# --------------------------------------------------------------------------
# 7. Quantized tables (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("bits", [8, 4])
@pytest.mark.parametrize("combiner", ["sum", "mean"])
def test_quantized_long_bag(bits, combiner):
    """Width 128, the 300-id bag of test_gpu.py's helper case with its
    out-of-range ids, at the bound of the quantized tables' own tests."""
    import test_quantized_int4 as q4
    import test_quantized_lookup as q8
    mod = q4 if bits == 4 else q8
    ext = _ext()
    forward = (ext.csr_lookup_forward_q4 if bits == 4
               else ext.csr_lookup_forward_q8)
    packed = mod._packed(128)
    case = _helper_case()
    ids, splits = case["ids_oob"], case["splits"]
    for w in (None, mod._case_weights()):
        ref, tol = mod._ref_tol(packed, ids, splits, combiner, w)
        for out_bf16 in (False, True):
            outs = [forward(packed.cuda(), ids.cuda(), splits.cuda(),
                            combiner == "mean", out_bf16,
                            None if w is None else w.cuda(),
                            deterministic=True) for _ in range(2)]
            assert torch.equal(outs[0], outs[1])
            mod._assert_bound(
                f"q{bits} {combiner} weighted={w is not None} bf16={out_bf16}",
                outs[0].float(), ref,
                tol + 2.0 ** -8 * ref.abs() if out_bf16 else tol)
        assert torch.equal(outs[1], forward(
            packed.cuda(), ids.cuda(), splits.cuda(), combiner == "mean",
            False, None if w is None else w.cuda(),
            deterministic=True).bfloat16())


# --------------------------------------------------------------------------
# 8. hipGraph capture (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
def test_graph_capture_deterministic_adagrad_step():
    """A captured fused-Adagrad step in deterministic mode (a capture admits
    no host sync): two replays from the same weights and state give the same
    bits, and the eager step's."""
    import distributed_embeddings_amd as de
    ops = _ops()
    width = 128
    g = torch.Generator().manual_seed(8)
    w0 = torch.randn(VOCAB, width, generator=g).cuda()
    s0 = (torch.rand(VOCAB, width, generator=g) + 0.5).cuda()
    ids, splits = (x.cuda() for x in _bwd_ids())
    grad = torch.randn(175, width, generator=g).cuda()
    lr = torch.tensor([LR], device="cuda")
    weight = w0.clone().requires_grad_(True)
    state = s0.clone()

    def step():
        out = ops.csr_lookup_fused_optimizer(weight, ids, splits, "sum", lr,
                                             state, True, 1e-8)
        out.backward(grad)

    def reset():
        with torch.no_grad():
            weight.copy_(w0)
            state.copy_(s0)

    with de.deterministic():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        reset()
        step()
        eager = (weight.detach().clone(), state.clone())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            step()
    replays = []
    for _ in range(2):
        reset()
        graph.replay()
        torch.cuda.synchronize()
        replays.append((weight.detach().clone(), state.clone()))
    assert not torch.equal(replays[0][0], w0)
    for a, b, c in zip(replays[0], replays[1], eager):
        assert torch.equal(a, b)
        assert torch.equal(a, c)


# --------------------------------------------------------------------------
# 9. The default path (GPU)
# --------------------------------------------------------------------------

@gpu
@requires_gpu
@pytest.mark.parametrize("width", [32, 128])
def test_flag_off_is_the_call_without_the_keyword(width):
    """Integer inputs: the default path's atomic sums are exact in any order,
    so the two spellings have to agree bit for bit."""
    import test_quantized_int4 as q4
    import test_quantized_lookup as q8
    ext = _ext()
    table = _int_table(width).cuda()
    fids, fsplits = (x.cuda() for x in _fwd_ids())
    bids, bsplits = (x.cuda() for x in _bwd_ids())
    grad = _int_grad(175, width).cuda()
    lr = torch.tensor([LR], device="cuda")
    for bf16 in (False, True):
        assert torch.equal(
            ext.csr_lookup_forward(table, fids, fsplits, False, bf16, None),
            ext.csr_lookup_forward(table, fids, fsplits, False, bf16, None,
                                   deterministic=False))
    case = _helper_case()
    for fwd, packed in ((ext.csr_lookup_forward_q8, q8._packed(width)),
                        (ext.csr_lookup_forward_q4, q4._packed(width))):
        # a 300-id bag of non-integers: compared at twice the tables' bound
        args = (packed.cuda(), case["ids_oob"].cuda(), case["splits"].cuda(),
                False, False, None)
        _, tol = (q8 if fwd is ext.csr_lookup_forward_q8 else q4)._ref_tol(
            packed, case["ids_oob"], case["splits"], "sum")
        a, b = fwd(*args), fwd(*args, deterministic=False)
        assert bool(((a - b).abs().double().cpu() <= 2 * tol).all())
    a = ext.csr_lookup_backward(grad, bids, bsplits, VOCAB, False, None)
    b = ext.csr_lookup_backward(grad, bids, bsplits, VOCAB, False, None,
                                deterministic=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    ws = []
    for kw in ({}, {"deterministic": False}):
        w = table.clone()
        ext.csr_fused_optimizer_apply(w, torch.empty(0, device="cuda"), bids,
                                      bsplits, grad, lr, False, False, 0.0,
                                      **kw)
        ws.append(w)
    assert torch.equal(ws[0], ws[1])
    assert not torch.equal(ws[0], table)
