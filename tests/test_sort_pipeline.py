"""Exact tests of the sparse-backward sort pipeline (bindings.cpp
build_sorted_segments: mask_oob_pack -> radix sort -> unpack -> gather ->
head flags -> scan -> unique -> bounds -> seg finish).

Everything here is integer work, so the HIP pipeline is compared for exact
equality with a plain int64 torch reference on the CPU.  The reference itself
is checked against brute-force Python loops by the tests that need no GPU.
"""

import functools

import pytest
import torch

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs GPU")


# ---------------------------------------------------------------------------
# CPU reference (int64 throughout)
# ---------------------------------------------------------------------------

def ref_sort(ids, vocab):
    """Stable sort of the ids with out-of-range ones masked to `vocab`."""
    ids = ids.to(torch.int64)
    masked = torch.where((ids < 0) | (ids >= vocab), torch.full_like(ids, vocab), ids)
    sorted_ids, sorted_pos = torch.sort(masked, stable=True)
    return sorted_ids, sorted_pos


def ref_pos_weights(lengths, mean, user_w):
    """fp32 weight of each position, iw * user_w in the kernel's order, or
    None when the pipeline carries no weights."""
    if not mean and user_w is None:
        return None
    n = int(lengths.sum())
    if mean:
        iw_row = torch.ones((), dtype=torch.float32) / lengths.clamp(min=1).to(torch.float32)
        iw = torch.repeat_interleave(iw_row, lengths)
    else:
        iw = torch.ones(n, dtype=torch.float32)
    return iw * user_w.to(torch.float32) if user_w is not None else iw


def ref_segments(ids, lengths, vocab, mean, user_w=None):
    sorted_ids, sorted_pos = ref_sort(ids, vocab)
    row_of_position = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    w = ref_pos_weights(lengths, mean, user_w)
    valid = sorted_ids[sorted_ids < vocab]
    unique_ids, counts = torch.unique_consecutive(valid, return_counts=True)
    return {
        "sorted_ids": sorted_ids,
        "sorted_pos": sorted_pos,
        "srow": row_of_position[sorted_pos],
        "sw": None if w is None else w[sorted_pos],
        "unique_ids": unique_ids,
        # segment starts, then the end of the last one
        "seg": torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(counts, 0)]),
        "num_unique": int(unique_ids.numel()),
        "bounds": int(valid.numel()),
    }


# ---------------------------------------------------------------------------
# The reference against brute force (no GPU)
# ---------------------------------------------------------------------------

_TINY = [
    # (ids, row lengths, vocab)
    ([3], [1], 5),
    ([5], [1], 5),                                # the only id is out of range
    ([4, 4, 4, 4], [0, 3, 0, 1], 5),              # all equal, id == vocab - 1
    ([2, 0, 1, 3], [2, 2], 4),                    # all distinct, none out of range
    ([-1, 7, 9, -3], [4], 7),                     # all out of range, both kinds
    ([6, -1, 0, 7, 6, 0, 6, 12, 3, 0], [3, 0, 0, 5, 2], 7),   # mixed, empty rows
    ([1, 0, 1, 0, 1, 0, 1], [7], 2),
    ([0, 1, 0, 0], [1, 1, 2], 1),                 # vocab 1: only id 0 is valid
]


def _brute_segments(ids, lengths, vocab, mean, user_w):
    n = len(ids)
    masked = [vocab if (v < 0 or v >= vocab) else v for v in ids]
    order = []
    for key in range(vocab + 1):                  # ascending keys, positions in order
        for p in range(n):
            if masked[p] == key:
                order.append(p)
    row_of = []
    for r, ln in enumerate(lengths):
        row_of += [r] * ln
    unique_ids, seg = [], []
    for i, p in enumerate(order):
        if masked[p] < vocab and (i == 0 or masked[order[i - 1]] != masked[p]):
            unique_ids.append(masked[p])
            seg.append(i)
    bounds = sum(1 for v in masked if v < vocab)
    seg.append(bounds)
    sw = None
    if mean or user_w is not None:
        sw = []
        for p in order:
            iw = torch.tensor(1.0) / torch.tensor(float(lengths[row_of[p]])) if mean \
                else torch.tensor(1.0)
            uw = torch.tensor(user_w[p], dtype=torch.float32) if user_w is not None \
                else torch.tensor(1.0)
            sw.append(float(iw * uw))
    return {"sorted_ids": [masked[p] for p in order], "sorted_pos": order,
            "srow": [row_of[p] for p in order], "sw": sw, "unique_ids": unique_ids,
            "seg": seg, "num_unique": len(unique_ids), "bounds": bounds}


@pytest.mark.parametrize("case", range(len(_TINY)))
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_matches_brute_force(case, mean, weighted):
    ids, lengths, vocab = _TINY[case]
    user_w = [0.5 + 0.37 * k for k in range(len(ids))] if weighted else None
    want = _brute_segments(ids, lengths, vocab, mean, user_w)
    got = ref_segments(torch.tensor(ids), torch.tensor(lengths), vocab, mean,
                       None if user_w is None else torch.tensor(user_w))
    for k in ("sorted_ids", "sorted_pos", "srow", "unique_ids", "seg"):
        assert got[k].dtype == torch.int64
        assert got[k].tolist() == want[k], k
    assert got["num_unique"] == want["num_unique"]
    assert got["bounds"] == want["bounds"]
    if want["sw"] is None:
        assert got["sw"] is None
    else:
        assert got["sw"].dtype == torch.float32
        assert got["sw"].tolist() == want["sw"]


def test_reference_sort_is_stable_and_masks_both_kinds():
    ids = torch.tensor([9, -2, 3, 10, 3, 9, 2 ** 40, 3, -(2 ** 40), 0])
    sorted_ids, sorted_pos = ref_sort(ids, 10)
    assert sorted_ids.tolist() == [0, 3, 3, 3, 9, 9, 10, 10, 10, 10]
    assert sorted_pos.tolist() == [9, 2, 4, 7, 0, 5, 1, 3, 6, 8]


def test_make_ids_covers_what_the_sort_tests_need():
    """The generated inputs really hold hot runs, both kinds of out-of-range
    id, vocab - 1 and (for the 32-bit vocab) ids with bit 31 set."""
    for vocab in _SORT_VOCABS:
        ids = _make_ids(3 * 512 + 17, vocab, seed=1)
        assert ids.dtype == torch.int64
        assert (ids < 0).any() and (ids >= vocab).any()
        assert (ids == vocab - 1).any()
        valid = ids[(ids >= 0) & (ids < vocab)]
        assert torch.bincount(torch.unique(valid, return_inverse=True)[1]).max() >= 8
        if vocab > 2 ** 31:
            assert ((valid >= 2 ** 31) & (valid < vocab - 1)).any()


# ---------------------------------------------------------------------------
# Inputs
# ---------------------------------------------------------------------------

# passes = ceil(log2_ceil(vocab + 1) / 8): 1, 1, 2, 2, 3, 4, 4
_SORT_VOCABS = [1, 255, 256, 65535, 2 ** 16, 2 ** 24, 2 ** 32 - 1]
_NUM_HOT = 32


def _make_ids(n, vocab, seed):
    """About half the ids fall in a few dozen hot values (long runs of equal
    keys across waves and tiles); the rest are uniform over [-3, vocab + 3)."""
    g = torch.Generator().manual_seed(seed)
    hot = torch.randint(0, vocab, (_NUM_HOT,), generator=g)
    hot[0] = vocab - 1                      # sits next to the sentinel `vocab`
    if vocab > 2 ** 31:
        hot[1] = 2 ** 31                    # bit 31 set
        hot[2] = 2 ** 31 + 123457
        hot[3] = vocab - 2
    ids = torch.randint(-3, vocab + 3, (n,), generator=g)
    pick = torch.rand(n, generator=g) < 0.5
    ids = torch.where(pick, hot[torch.randint(0, _NUM_HOT, (n,), generator=g)], ids)
    if n >= 16:                             # what a small draw could miss
        ids[n // 7] = -1
        ids[n // 5] = vocab + 2
        ids[n // 3] = vocab - 1
        if vocab > 2 ** 31:
            ids[n // 2] = 2 ** 31 + 5
    return ids


def _ext():
    from distributed_embeddings_amd.ops import _backend
    return _backend.ops()


def _check_sort(ext, n, vocab, variant, sort):
    ids = _make_ids(n, vocab, seed=n * 31 + vocab % 1009)
    want_ids, want_pos = ref_sort(ids, vocab)
    got_ids, got_pos = ext.debug_sort_ids(ids.cuda(), vocab, variant, sort)
    assert got_ids.dtype == torch.int64 and got_pos.dtype == torch.int32
    tag = f"n={n} vocab={vocab} variant={variant} sort={sort}"
    assert torch.equal(got_ids.cpu(), want_ids), f"sorted_ids differ: {tag}"
    # the positions prove stability: equal ids keep their input order
    assert torch.equal(got_pos.cpu().to(torch.int64), want_pos), f"sorted_pos differ: {tag}"


def _edge_sizes(tile):
    return [1, 63, 64, 65, tile - 1, tile, tile + 1, 3 * tile + 17]


# ---------------------------------------------------------------------------
# GPU: the sort, every variant
# ---------------------------------------------------------------------------

# variants 0..7 of the hand-written sort, its size dispatch, and rocPRIM.
# The rocPRIM row at vocab 2**32 - 1 is the one that found a bug: a bit range
# ending at bit 64 left the ids unsorted from n = 1025 on (sort_ids_dispatch
# now sorts the whole key there).
_SORTERS = [(v, "custom") for v in range(8)] + [(-1, "default"), (-1, "rocprim")]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("vocab", _SORT_VOCABS)
@pytest.mark.parametrize("sorter", _SORTERS, ids=lambda s: f"v{s[0]}-{s[1]}")
def test_sort_exact(sorter, vocab):
    ext = _ext()
    variant, sort = sorter
    tiles = ext.debug_sort_variant_tiles()
    assert len(tiles) == 8
    if variant >= 0:
        sizes = _edge_sizes(tiles[variant])
    else:   # the tile is not fixed: every variant's sizes
        sizes = sorted({n for t in tiles for n in _edge_sizes(t)})
    for n in sizes:
        _check_sort(ext, n, vocab, variant, sort)


@pytest.mark.gpu
@requires_gpu
def test_debug_bindings_reject_bad_arguments():
    ext = _ext()
    ids = torch.zeros(4, dtype=torch.int64, device="cuda")
    splits = torch.tensor([0, 4], device="cuda")
    with pytest.raises(RuntimeError):
        ext.debug_sort_ids(ids, 10, 8, "custom")
    with pytest.raises(RuntimeError):
        ext.debug_sort_ids(ids, 10, -2, "custom")
    with pytest.raises(RuntimeError):
        ext.debug_sort_ids(ids, 10, -1, "thrust")
    with pytest.raises(RuntimeError):
        ext.debug_sorted_segments(ids, splits, 10, False, None, False, 9, "custom")
    with pytest.raises(RuntimeError):
        ext.debug_sorted_segments(ids, torch.tensor([0, 5], device="cuda"), 10, False)


@pytest.mark.gpu
@requires_gpu
def test_debug_bindings_empty_input():
    ext = _ext()
    ids = torch.zeros(0, dtype=torch.int64, device="cuda")
    for sort in ("default", "custom", "rocprim"):
        sorted_ids, sorted_pos = ext.debug_sort_ids(ids, 10, -1, sort)
        assert sorted_ids.numel() == 0 and sorted_pos.numel() == 0
    splits = torch.zeros(3, dtype=torch.int64, device="cuda")
    for padded in (False, True):
        sorted_ids, srow, sw, seg, unique_ids, num_unique, bounds = \
            ext.debug_sorted_segments(ids, splits, 10, True, None, padded)
        assert sorted_ids.numel() == 0 and srow.numel() == 0 and sw.numel() == 0
        assert unique_ids.numel() == 0
        assert seg.tolist() == [0] and num_unique.item() == 0 and bounds.item() == 0


# ---------------------------------------------------------------------------
# GPU: scan and dispatch edges
# ---------------------------------------------------------------------------

@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n,vocab,variant", [
    # variant 5 (tile 512): 586 blocks, a table of 150 016 entries, chunk 74.
    # The smallest n of the smallest tile whose table passes 131 072 entries
    # with a chunk that is no multiple of 64 and leaves a ragged last chunk;
    # rs_scan_top loops over ~2028 partial sums.
    (300_001, 2 ** 16, 5),
    # default dispatch on both sides of the variant 4 / variant 7 threshold:
    # the largest n that takes variant 4 and the smallest that takes 7
    (524_288, 65535, -1),
    (524_289, 65535, -1),
    # default dispatch (variant 7), four passes, several tiles past the
    # threshold with a ragged last tile
    (600_000, 2 ** 24, -1),
])
def test_sort_scan_and_dispatch_edges(n, vocab, variant):
    _check_sort(_ext(), n, vocab, variant, "default")


# ---------------------------------------------------------------------------
# GPU: segment bookkeeping
# ---------------------------------------------------------------------------

_SEG_VOCAB = 7001


def _seg_case(name, n, seed):
    """(ids, row lengths, per-id weights) of one named case; rows are ragged."""
    g = torch.Generator().manual_seed(seed)
    vocab = _SEG_VOCAB
    if name == "all_oob":
        ids = torch.where(torch.rand(n, generator=g) < 0.5,
                          torch.randint(-50, 0, (n,), generator=g),
                          torch.randint(vocab, vocab + 50, (n,), generator=g))
        if n >= 2:
            ids[0], ids[-1] = -1, vocab          # negative and >= vocab at once
    elif name == "none_oob":
        ids = torch.randint(0, vocab, (n,), generator=g)
        ids[n // 2] = vocab - 1
    elif name == "all_equal":
        ids = torch.full((n,), vocab - 1)        # next to the sentinel
    elif name == "all_distinct":
        ids = torch.randperm(vocab, generator=g)[:n]
    elif name == "mixed":
        ids = torch.randint(-40, vocab + 40, (n,), generator=g)
        hot = torch.rand(n, generator=g) < 0.4
        ids = torch.where(hot, torch.randint(0, 16, (n,), generator=g) * 431, ids)
        if n >= 4:
            ids[0], ids[1], ids[2], ids[-1] = -7, vocab, vocab - 1, vocab + 3
    else:
        raise AssertionError(name)
    # a few long rows (the wave-per-row expansion) or many short ones with
    # empties among them (the thread-per-row expansion)
    num_rows = n // 40 + 1 if name in ("all_equal", "all_distinct") else n // 3 + 3
    rows = torch.randint(0, num_rows, (n,), generator=g)
    lengths = torch.bincount(rows, minlength=num_rows)
    if name == "mixed" and n > 1:
        assert (lengths == 0).any()
    user_w = torch.rand(n, generator=g) * 4 - 2
    return ids, lengths, user_w


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n", [1, 5003])
@pytest.mark.parametrize("name", ["all_oob", "none_oob", "all_equal", "all_distinct", "mixed"])
def test_sorted_segments_exact(name, n):
    ext = _ext()
    vocab = _SEG_VOCAB
    ids, lengths, user_w = _seg_case(name, n, seed=n + len(name))
    splits = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
    ids_d, splits_d, w_d = ids.cuda(), splits.cuda(), user_w.cuda()
    for mean in (False, True):
        for weighted in (False, True):
            want = ref_segments(ids, lengths, vocab, mean, user_w if weighted else None)
            nu = want["num_unique"]
            for padded in (False, True):
                tag = f"{name} n={n} mean={mean} weighted={weighted} padded={padded}"
                sorted_ids, srow, sw, seg, unique_ids, num_unique, bounds = \
                    ext.debug_sorted_segments(ids_d, splits_d, vocab, mean,
                                              w_d if weighted else None, padded)
                assert num_unique.item() == nu, tag
                assert bounds.item() == want["bounds"], tag
                assert torch.equal(sorted_ids.cpu(), want["sorted_ids"]), tag
                assert srow.dtype == torch.int64
                assert torch.equal(srow.cpu(), want["srow"]), tag
                assert torch.equal(unique_ids.cpu()[:nu], want["unique_ids"]), tag
                seg = seg.cpu()
                assert seg.dtype == torch.int64 and seg.numel() == n + 1
                if padded:
                    assert torch.equal(seg[:nu], want["seg"][:nu]), tag
                    assert bool((seg[nu:] == want["bounds"]).all()), tag
                else:
                    assert torch.equal(seg[:nu + 1], want["seg"]), tag
                if want["sw"] is None:
                    assert sw is None, tag
                else:
                    # fp32 iw * user_w in the kernel's order: bit-exact
                    assert sw.dtype == torch.float32
                    assert torch.equal(sw.cpu(), want["sw"]), tag


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("sorter", [(0, "custom"), (5, "custom"), (7, "custom"), (-1, "rocprim")],
                         ids=lambda s: f"v{s[0]}-{s[1]}")
def test_sorted_segments_pass_the_sort_choice_through(sorter):
    """build_sorted_segments hands variant and sort to the sort it runs."""
    ext = _ext()
    variant, sort = sorter
    ids, lengths, user_w = _seg_case("mixed", 5003, seed=77)
    splits = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
    want = ref_segments(ids, lengths, _SEG_VOCAB, True, user_w)
    sorted_ids, srow, sw, seg, unique_ids, num_unique, bounds = ext.debug_sorted_segments(
        ids.cuda(), splits.cuda(), _SEG_VOCAB, True, user_w.cuda(), False, variant, sort)
    nu = want["num_unique"]
    assert num_unique.item() == nu and bounds.item() == want["bounds"]
    assert torch.equal(sorted_ids.cpu(), want["sorted_ids"])
    assert torch.equal(srow.cpu(), want["srow"])
    assert torch.equal(sw.cpu(), want["sw"])
    assert torch.equal(seg.cpu()[:nu + 1], want["seg"])
    assert torch.equal(unique_ids.cpu()[:nu], want["unique_ids"])


@pytest.mark.gpu
@requires_gpu
def test_positions_ascend_within_id_segments():
    """The other half of test_kernel_determinism_short_segments: at its id
    distribution, equal ids keep ascending positions (a stable sort), so the
    reduction order is fixed by the input and not merely repeatable.  The
    position of each sorted id travels as its per-id weight: mean is off, so
    sw = 1.0f * position, exact in fp32 below 2^24."""
    ext = _ext()
    torch.manual_seed(11)
    vocab, rows, hot = 2_000_000, 5_000, 4
    n = rows * hot
    ids = torch.randint(0, vocab, (n,))
    splits = torch.arange(0, n + 1, hot)
    pos_w = torch.arange(n, dtype=torch.float32)
    out = ext.debug_sorted_segments(ids.cuda(), splits.cuda(), vocab, False, pos_w.cuda())
    sorted_ids, srow, pos = out[0].cpu(), out[1].cpu(), out[2].cpu().to(torch.int64)
    assert torch.equal(ids[pos], sorted_ids)              # a permutation of the input
    assert torch.equal(torch.sort(pos)[0], torch.arange(n))
    same = sorted_ids[1:] == sorted_ids[:-1]
    assert int(same.sum()) > 0                            # the case is not vacuous
    assert bool((sorted_ids[1:] >= sorted_ids[:-1]).all())
    assert bool((pos[1:][same] > pos[:-1][same]).all())
    assert torch.equal(srow, pos // hot)
    again = ext.debug_sorted_segments(ids.cuda(), splits.cuda(), vocab, False, pos_w.cuda())
    nu = int(out[5].item())
    assert torch.equal(out[5], again[5]) and torch.equal(out[6], again[6])
    for k in (0, 1, 2):
        assert torch.equal(out[k], again[k])
    # seg and unique_ids are set only up to num_unique
    assert torch.equal(out[3][:nu + 1], again[3][:nu + 1])
    assert torch.equal(out[4][:nu], again[4][:nu])


# ---------------------------------------------------------------------------
# GPU: the production path, exact
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_case(n, vocab, width, combiner):
    """Integer-valued inputs whose every partial sum is exact in fp32, and
    the int64 index_add_ reference.  Never mutated by the tests."""
    from distributed_embeddings_amd.utils.input_gen import power_law_ids
    g = torch.Generator().manual_seed(n + width)
    if combiner == "mean":
        # rows of length 1, 2 and 4 only: exact reciprocals
        lengths = torch.tensor([1, 2, 4])[torch.randint(0, 3, (n // 2,), generator=g)]
        keep = int((torch.cumsum(lengths, 0) <= n).sum())
        lengths = lengths[:keep]
        lengths = torch.cat([lengths, torch.ones(n - int(lengths.sum()), dtype=torch.int64)])
        mult = 4 // lengths                      # 4 * (1 / len)
    else:
        rows = torch.randint(0, n // 4, (n,), generator=g)
        lengths = torch.bincount(rows, minlength=n // 4)
        mult = torch.full_like(lengths, 4)
    assert int(lengths.sum()) == n
    num_rows = lengths.numel()
    ids = power_law_ids(vocab, (n,), generator=g)
    oob = torch.rand(n, generator=g) < 0.01
    ids = torch.where(oob, torch.where(torch.rand(n, generator=g) < 0.5,
                                       torch.full_like(ids, -1), ids + vocab), ids)
    ids[n // 2] = vocab - 1
    splits = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(lengths, 0)])
    grad_int = torch.randint(-8, 9, (num_rows, width), generator=g)
    w_int = torch.randint(-8, 9, (vocab, width), generator=g)

    row_of_position = torch.repeat_interleave(torch.arange(num_rows), lengths)
    valid = (ids >= 0) & (ids < vocab)
    unique_ids, inverse = torch.unique(ids[valid], return_inverse=True)
    contrib = (grad_int * mult[:, None])[row_of_position[valid]]      # 4 * true value
    acc4 = torch.zeros(unique_ids.numel(), width, dtype=torch.int64).index_add_(0, inverse, contrib)
    # Every partial sum, scaled by lr = 0.5 and added to a weight, is a
    # multiple of 1/8 below 2^21: 24 significant bits, exact in fp32 in any
    # order of summation.
    abs4 = torch.zeros(unique_ids.numel(), width, dtype=torch.int64).index_add_(
        0, inverse, contrib.abs())
    assert int(abs4.max()) // 4 + 8 < 2 ** 21
    unique_grad = (acc4.double() / 4).float()
    assert torch.equal(unique_grad.double() * 4, acc4.double())
    w_after = w_int.double()
    w_after[unique_ids] -= 0.5 * acc4.double() / 4
    w_after32 = w_after.float()
    assert torch.equal(w_after32.double(), w_after)
    return {"ids": ids, "splits": splits, "grad": grad_int.float(), "w0": w_int.float(),
            "unique_ids": unique_ids, "unique_grad": unique_grad, "w_after": w_after32}


# n = 20 000 (variant 4, power-law ids: short and long segments) at an even
# and an odd width, and n = 600 000 (variant 7) once at width 16
_EXACT = [(20_000, 100_000, 128, "sum"), (20_000, 100_000, 128, "mean"),
          (20_000, 100_000, 33, "sum"), (20_000, 100_000, 33, "mean"),
          (600_000, 2 ** 20, 16, "sum")]


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n,vocab,width,combiner", _EXACT)
def test_csr_lookup_backward_exact(n, vocab, width, combiner):
    c = _exact_case(n, vocab, width, combiner)
    unique_ids, unique_grad = _ext().csr_lookup_backward(
        c["grad"].cuda(), c["ids"].cuda(), c["splits"].cuda(), vocab, combiner == "mean")
    assert torch.equal(unique_ids.cpu(), c["unique_ids"])
    assert unique_grad.dtype == torch.float32
    assert torch.equal(unique_grad.cpu(), c["unique_grad"])


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("n,vocab,width,combiner", _EXACT)
def test_csr_fused_sgd_exact(n, vocab, width, combiner):
    c = _exact_case(n, vocab, width, combiner)
    weight = c["w0"].cuda()
    lr = torch.tensor([0.5], device="cuda")
    state = torch.empty(0, device="cuda")
    _ext().csr_fused_optimizer_apply(weight, state, c["ids"].cuda(), c["splits"].cuda(),
                                     c["grad"].cuda(), lr, combiner == "mean", False, 0.0)
    assert torch.equal(weight.cpu(), c["w_after"])
