"""IntegerLookup against a dictionary model, on the CPU path and the kernels.

The oracle is the history of every (key, output) pair a module has produced.
Which value a new key receives is not deterministic on the GPU (lanes race
for the free values), so the model pins down no particular assignment; it
holds every assignment to the invariants below, exactly, after every batch.
``check(lk, history)``:

1. Stable.  Every occurrence of a key, within a batch and across batches,
   carries one value.  (Without ``auto_grow`` a key that received 0 keeps 0;
   with it no key but -1 ever receives 0, by 3.)  Key -1 always carries 0.
2. Injective and dense.  Distinct keys with non-zero values have distinct
   values, and the values in use are exactly 1..k.
3. No value wasted.  k = min(distinct non-sentinel keys seen, max_tokens)
   without ``auto_grow``; with it k is the number of distinct non-sentinel
   keys and every output of a key other than -1 is positive.
4. Counts.  ``counts`` is the histogram of all outputs so far, plus the
   pre-claimed 1 in ``counts[0]``, compared as whole arrays.
5. Vocabulary.  ``get_vocabulary()`` is [-1] + the keys with value > 0 in
   value order, and its length is ``vocabulary_size()``.
6. Table well-formed, read from the buffers: no key twice, every occupied
   slot reachable from its key's home slot ``mix64(key) % capacity`` by
   linear probing over occupied slots only, the (key, value > 0) entries are
   the model's, and there are k of them.

Keys are picked by home slot with ``_mix64_np`` so that chains wrap through
slot 0 on purpose.  Everything is integer-exact; there is no tolerance.
"""

import numpy as np
import pytest
import torch

from distributed_embeddings_amd import IntegerLookup
from distributed_embeddings_amd.layers.integer_lookup import _mix64_np

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                                  reason="needs GPU")
_on_gpu = pytest.param("cuda", marks=[pytest.mark.gpu, requires_gpu])
_DEVICES = ["cpu", _on_gpu]

_I64_MIN = np.iinfo(np.int64).min
_I64_MAX = np.iinfo(np.int64).max


# --------------------------------------------------------------------------
# The model
# --------------------------------------------------------------------------

class History:
    """Every key looked up so far and the output it received, in order."""

    def __init__(self):
        self.keys = []
        self.outs = []

    def add(self, keys, outs):
        self.keys.append(np.asarray(keys, dtype=np.int64).reshape(-1))
        self.outs.append(np.asarray(outs, dtype=np.int64).reshape(-1))

    def flat(self):
        if not self.keys:
            z = np.empty(0, dtype=np.int64)
            return z, z
        return np.concatenate(self.keys), np.concatenate(self.outs)

    def mapping(self):
        """(distinct keys, their value) — the first output each received;
        invariant 1 says it is the only one."""
        k, o = self.flat()
        uniq, first = np.unique(k, return_index=True)
        return uniq, o[first]


def _home(keys, cap):
    return (_mix64_np(np.asarray(keys, dtype=np.int64)) %
            np.uint64(cap)).astype(np.int64)


def check_table(lk, live_keys, live_vals):
    """Invariant 6 against the model's (key, value > 0) pairs."""
    tk = lk.table_keys.cpu().numpy()
    tv = lk.table_values.cpu().numpy()
    cap = lk.capacity
    assert tk.shape == tv.shape == (cap,)
    assert cap == int(1.5 * (lk.max_tokens + 1))
    occ = tk != -1
    slots = np.flatnonzero(occ)
    keys = tk[slots]
    assert np.unique(keys).size == keys.size, "a key occupies two slots"
    assert ((tv[slots] >= 0) & (tv[slots] <= lk.max_tokens)).all()
    # reachable: no empty slot in the cyclic range [home, slot]
    empties = np.concatenate([[0], np.cumsum(~occ)])
    home = _home(keys, cap)
    straight = empties[slots + 1] - empties[home]
    wrapped = empties[cap] - empties[home] + empties[slots + 1]
    gaps = np.where(home <= slots, straight, wrapped)
    assert (gaps == 0).all(), \
        f"keys {keys[gaps != 0].tolist()} are cut off from their home slot"
    live = tv[slots] > 0
    got = sorted(zip(keys[live].tolist(), tv[slots][live].tolist()))
    want = sorted(zip(np.asarray(live_keys).tolist(),
                      np.asarray(live_vals).tolist()))
    assert got == want


def check(lk, history):
    all_k, all_o = history.flat()
    uniq, inv = np.unique(all_k, return_inverse=True)
    val = history.mapping()[1]
    # 1. stable
    bad = all_o != val[inv]
    assert not bad.any(), \
        f"keys {np.unique(all_k[bad]).tolist()} changed their value"
    assert (all_o[all_k == -1] == 0).all(), "key -1 must map to 0"
    # 2. injective and dense
    real = uniq != -1
    live = val > 0
    k = int(live.sum())
    assert sorted(val[live].tolist()) == list(range(1, k + 1))
    # 3. no value wasted
    distinct = int(real.sum())
    if lk.auto_grow:
        assert k == distinct
        assert (all_o[all_k != -1] > 0).all()
    else:
        assert k == min(distinct, lk.max_tokens)
    # 4. counts
    want = np.bincount(all_o, minlength=lk.max_tokens + 1)
    want[0] += 1
    assert lk.counts.cpu().tolist() == want.tolist()
    # 5. vocabulary
    order = np.argsort(val[live])
    assert lk.get_vocabulary() == [-1] + uniq[live][order].tolist()
    assert lk.vocabulary_size() == k + 1
    # 6. table
    check_table(lk, uniq[live], val[live])


def step(lk, history, keys, shape=None):
    """One forward on the module's device, recorded and checked."""
    keys = np.asarray(keys, dtype=np.int64)
    t = torch.from_numpy(keys.copy()).to(lk.table_keys.device)
    if shape is not None:
        t = t.reshape(shape)
    out = lk(t)
    assert out.shape == t.shape and out.dtype == torch.int64
    assert out.device == t.device
    out = out.cpu().numpy().reshape(-1)
    history.add(keys, out)
    check(lk, history)
    return out


# --------------------------------------------------------------------------
# Wrap-around and chains
# --------------------------------------------------------------------------

def _keys_homed_at(cap, slot, count):
    cand = np.arange(1, 100000, dtype=np.int64)
    hit = cand[_home(cand, cap) == slot]
    assert hit.size >= count, f"only {hit.size} keys home at slot {slot}"
    return hit[:count]


def _chain_keys(max_tokens, which):
    cap = int(1.5 * (max_tokens + 1))
    if which == "wrap":          # (a) runs over the end of the table
        return _keys_homed_at(cap, cap - 1, max_tokens + 2)
    if which == "chain3":        # (b) three keys sharing one home slot
        return _keys_homed_at(cap, cap - 2, 3)
    assert which == "every_slot"  # (c) one key per slot: the table fills
    return np.array([_keys_homed_at(cap, s, 1)[0] for s in range(cap)])


@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("order", ["one_batch", "one_per_batch", "reversed"])
@pytest.mark.parametrize("which", ["wrap", "chain3", "every_slot"])
@pytest.mark.parametrize("max_tokens", [1, 3, 7])
def test_chains(max_tokens, which, order, device):
    keys = _chain_keys(max_tokens, which)
    lk = IntegerLookup(max_tokens=max_tokens, device=device)
    h = History()
    if order == "one_batch":
        step(lk, h, keys)
    elif order == "one_per_batch":
        for key in keys:
            step(lk, h, [key])
    else:
        for key in keys[::-1]:
            step(lk, h, [key])
    # finds walk the same chains, duplicates included
    again = step(lk, h, np.concatenate([keys, keys[::-1]]))
    assert (again[:keys.size] == again[keys.size:][::-1]).all()


# --------------------------------------------------------------------------
# Batch sizes at wave and block edges
# --------------------------------------------------------------------------

def _pool():
    """200 distinct keys spread over the whole int64 range."""
    rng = np.random.default_rng(2024)
    pool = rng.integers(_I64_MIN, _I64_MAX, 200, dtype=np.int64,
                        endpoint=True)
    assert np.unique(pool).size == 200 and -1 not in pool
    assert (pool < 0).sum() > 50 and (pool > 0).sum() > 50
    return pool, rng


@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_batch_sizes(n, device):
    pool, rng = _pool()
    lk = IntegerLookup(max_tokens=300, device=device)
    h = History()
    first = pool[rng.integers(0, 200, n)]
    step(lk, h, first)
    step(lk, h, pool[rng.integers(0, 200, n)])
    step(lk, h, first)


@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("auto_grow", [False, True])
@pytest.mark.parametrize("shape", [(0,), (2, 0, 3)])
@pytest.mark.parametrize("prefill", [False, True])
def test_empty_batch(prefill, shape, auto_grow, device):
    pool, _ = _pool()
    lk = IntegerLookup(max_tokens=300, auto_grow=auto_grow, device=device)
    h = History()
    if prefill:
        step(lk, h, pool[:70])
    before = {k: v.clone() for k, v in lk.state_dict().items()}
    out = step(lk, h, np.empty(0, dtype=np.int64), shape=shape)
    assert out.size == 0
    after = lk.state_dict()
    assert before.keys() == after.keys()
    for name, t in before.items():
        assert torch.equal(t, after[name]), name


@pytest.mark.parametrize("device", _DEVICES)
def test_batch_3d(device):
    pool, rng = _pool()
    lk = IntegerLookup(max_tokens=300, device=device)
    h = History()
    keys = pool[rng.integers(0, 200, 1000)]
    out = step(lk, h, keys, shape=(10, 4, 25))
    assert (out == step(lk, h, keys)).all()


# --------------------------------------------------------------------------
# Key values
# --------------------------------------------------------------------------

_SPECIAL = [-1, 0, -2, -7, _I64_MIN, _I64_MAX, 2 ** 32]
_BIT_PAIRS = [
    (0x123456789ABCDEF0, 0x123456789ABCDEF0 - 2 ** 63),   # bit 63
    (12345, 12345 + 2 ** 32),                             # bit 32
    (-(2 ** 40), -(2 ** 40) + 2 ** 32),                   # bit 32, negative
    (1000, 1001),                                         # bit 0
    (_I64_MIN + 2, _I64_MIN + 3),                         # bit 0, negative
]


@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("auto_grow", [False, True])
def test_special_keys(auto_grow, device):
    pairs = [k for p in _BIT_PAIRS for k in p]
    for a, b in _BIT_PAIRS:
        assert bin((a ^ b) & (2 ** 64 - 1)).count("1") == 1
    lk = IntegerLookup(max_tokens=32, auto_grow=auto_grow, device=device)
    h = History()
    out = step(lk, h, _SPECIAL + pairs + _SPECIAL[::-1])
    assert out[0] == 0 and (out[1:len(_SPECIAL)] > 0).all()
    step(lk, h, pairs[::-1] + _SPECIAL + [-1, -1])


@pytest.mark.parametrize("device", _DEVICES)
def test_negative_keys_in_vocabulary(device):
    """Negative keys are ordinary keys and appear in the vocabulary."""
    lk = IntegerLookup(max_tokens=8, device=device)
    h = History()
    out = step(lk, h, [-1, 5, -7, -1, 5, _I64_MIN, _I64_MAX])
    vocab = lk.get_vocabulary()
    assert len(vocab) == lk.vocabulary_size() == 5
    assert vocab[0] == -1
    for key, v in zip([5, -7, _I64_MIN, _I64_MAX], out[[1, 2, 5, 6]]):
        assert vocab[v] == key


@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("auto_grow", [False, True])
def test_all_sentinel_batch(auto_grow, device):
    lk = IntegerLookup(max_tokens=16, auto_grow=auto_grow, device=device)
    h = History()
    out = step(lk, h, np.full(300, -1))
    assert (out == 0).all()
    assert int(lk.counts[0]) == 301 and int(lk.counts[1:].sum()) == 0
    assert (lk.table_keys.cpu() == -1).all()
    assert (lk.table_values.cpu() == 0).all()
    assert lk.max_tokens == 16
    assert step(lk, h, [-1, 40, -1]).tolist() == [0, 1, 0]


@pytest.mark.parametrize("device", _DEVICES)
def test_sentinel_draws_no_value(device):
    """-1 500 times next to exactly max_tokens new keys: all 16 get values."""
    rng = np.random.default_rng(16)
    new = np.arange(16, dtype=np.int64) * 1_000_003 + 17
    batch = np.concatenate([np.full(500, -1), new, new[:5]])
    rng.shuffle(batch)
    lk = IntegerLookup(max_tokens=16, device=device)
    h = History()
    out = step(lk, h, batch)
    assert sorted(set(out[batch != -1].tolist())) == list(range(1, 17))
    assert int(lk.counts[0]) == 501
    assert (out == step(lk, h, batch)).all()


@pytest.mark.parametrize("device", _DEVICES)
def test_auto_grow_sentinel_is_not_upgraded(device):
    """Under auto_grow -1 is neither a miss nor a value-0 entry to upgrade."""
    lk = IntegerLookup(max_tokens=16, auto_grow=True, device=device)
    h = History()
    first = step(lk, h, [-1, 5, -1])
    assert first[0] == first[2] == 0 and first[1] == 1
    second = step(lk, h, [-1, 9, 5])
    assert second.tolist() == [0, 2, 1]
    assert lk.get_vocabulary() == [-1, 5, 9]


# --------------------------------------------------------------------------
# Overflow-pinned entries
# --------------------------------------------------------------------------

def _pin(lk, key):
    """Writes (key, 0) where hash_insert leaves it when no value is free."""
    tk = lk.table_keys.cpu().numpy().copy()
    tv = lk.table_values.cpu().numpy().copy()
    slot = int(_home([key], lk.capacity)[0])
    while tk[slot] != -1:
        slot = (slot + 1) % lk.capacity
    tk[slot], tv[slot] = key, 0
    lk.table_keys.copy_(torch.from_numpy(tk))
    lk.table_values.copy_(torch.from_numpy(tv))


@pytest.mark.parametrize("device", _DEVICES)
def test_vocabulary_skips_pinned_entries(device):
    """A full GPU table pins an unseen key to value 0 in a slot of its own;
    the vocabulary must not list it.  On the CPU, whose forward leaves such
    keys out of the table, the entry is written as the kernel leaves it."""
    lk = IntegerLookup(max_tokens=2, device=device)
    h = History()
    step(lk, h, [10, 11])
    if device == "cpu":
        _pin(lk, 77)
        lk.counts[0] += 1
        h.add([77], [0])
        check(lk, h)
    else:
        assert step(lk, h, [77]).tolist() == [0]
        assert 77 in lk.table_keys.cpu().tolist()
    assert sorted(lk.get_vocabulary()[1:]) == [10, 11]
    assert step(lk, h, [77, 10, 11, 77])[[0, 3]].tolist() == [0, 0]


@pytest.mark.parametrize("device", _DEVICES)
def test_auto_grow_resolves_pinned_entry_across_growth(device):
    """A value-0 entry in a full auto_grow table (what the GPU forward has
    between retracting counts[0] and growing; also a checkpoint of a fixed
    table loaded with auto_grow=True): looking the key up grows the table
    and gives it a real value, in a slot of its own."""
    lk = IntegerLookup(max_tokens=2, auto_grow=False, device=device)
    h = History()
    step(lk, h, [10, 11])
    lk.auto_grow = True
    _pin(lk, 77)
    out = step(lk, h, [77, 10, 78, 77])
    assert out[0] == out[3] and out[0] > 0
    assert lk.max_tokens > 2


# --------------------------------------------------------------------------
# Heavy duplication in a nearly full table
# --------------------------------------------------------------------------

@pytest.mark.parametrize("device", _DEVICES)
def test_heavy_duplication_nearly_full(device):
    rng = np.random.default_rng(7)
    pool = np.unique(rng.integers(_I64_MIN, _I64_MAX, 130, dtype=np.int64))
    assert pool.size == 130 and -1 not in pool
    rng.shuffle(pool)
    old, new = pool[:90], pool[90:]
    lk = IntegerLookup(max_tokens=100, device=device)
    h = History()
    step(lk, h, old)
    batch = np.concatenate([pool, pool[rng.integers(0, 130, 50000 - 130)]])
    rng.shuffle(batch)
    out = step(lk, h, batch)
    is_new = np.isin(batch, new)
    _, first = np.unique(batch[is_new], return_index=True)
    new_vals = out[is_new][first]
    assert sorted(new_vals[new_vals > 0].tolist()) == list(range(91, 101))
    assert (new_vals == 0).sum() == 30
    assert (out == step(lk, h, batch)).all()


# --------------------------------------------------------------------------
# Rehash directly
# --------------------------------------------------------------------------

@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("max_tokens", [1, 3, 7])
def test_rehash(max_tokens, device):
    """_grow (hash_rehash on the GPU) on a table written by hand: the
    wrapping chain with values 1..max_tokens, its last two keys pinned to 0."""
    keys = _chain_keys(max_tokens, "wrap")
    vals = np.concatenate([np.arange(1, max_tokens + 1), [0, 0]])
    lk = IntegerLookup(max_tokens=max_tokens, device=device)
    cap = lk.capacity
    tk = np.full(cap, -1, dtype=np.int64)
    tv = np.zeros(cap, dtype=np.int64)
    for key, v in zip(keys, vals):
        slot = cap - 1
        while tk[slot] != -1:
            slot = (slot + 1) % cap
        tk[slot], tv[slot] = key, v
    assert tk[cap - 1] != -1 and tk[0] != -1          # the chain wraps
    assert (tk == -1).sum() == cap - (max_tokens + 2)
    lk.table_keys.copy_(torch.from_numpy(tk))
    lk.table_values.copy_(torch.from_numpy(tv))
    lk.counts[1:] = 1
    h = History()
    h.add(keys[:max_tokens], vals[:max_tokens])
    check(lk, h)

    lk._grow()
    assert lk.max_tokens == 2 * max_tokens
    assert lk.capacity == int(1.5 * (2 * max_tokens + 1))
    new_keys = lk.table_keys.cpu().numpy()
    assert sorted(new_keys[new_keys != -1].tolist()) == \
        sorted(keys[:max_tokens].tolist())             # pinned entries gone
    assert lk.counts.cpu().tolist() == [1] * (max_tokens + 1) + \
        [0] * max_tokens
    check(lk, h)
    # the formerly pinned keys now take real values
    out = step(lk, h, keys)
    assert out[:max_tokens].tolist() == vals[:max_tokens].tolist()
    # (max_tokens=1 grows to 2: one of the two finds no value left)
    assert sorted(out[max_tokens:].tolist()) == sorted(
        v if v <= lk.max_tokens else 0
        for v in (max_tokens + 1, max_tokens + 2))


# --------------------------------------------------------------------------
# Auto-grow
# --------------------------------------------------------------------------

@pytest.mark.parametrize("device", _DEVICES)
@pytest.mark.parametrize("max_tokens", [1, 4])
def test_auto_grow_fills_mid_batch(max_tokens, device):
    rng = np.random.default_rng(max_tokens)
    pool = np.unique(rng.integers(_I64_MIN, _I64_MAX, 1000, dtype=np.int64))
    assert pool.size == 1000 and -1 not in pool
    batch = np.concatenate([pool, pool[rng.integers(0, 1000, 2000)]])
    rng.shuffle(batch)
    batch[rng.choice(3000, 150, replace=False)] = -1
    n_sentinel = int((batch == -1).sum())
    assert np.unique(batch).size > 990
    lk = IntegerLookup(max_tokens=max_tokens, auto_grow=True, device=device)
    h = History()
    out = step(lk, h, batch)
    assert int(lk.counts[0]) == 1 + n_sentinel
    assert lk.max_tokens >= 1000
    assert (out == step(lk, h, batch)).all()
    assert int(lk.counts[0]) == 1 + 2 * n_sentinel


@pytest.mark.parametrize("device", _DEVICES)
def test_auto_grow_proactive_small_batches(device):
    """Many small batches, each crossing or nearing 80 % load."""
    rng = np.random.default_rng(99)
    pool = np.unique(rng.integers(_I64_MIN, _I64_MAX, 300, dtype=np.int64))
    assert pool.size == 300 and -1 not in pool
    lk = IntegerLookup(max_tokens=4, auto_grow=True, device=device)
    h = History()
    grown = set()
    for i in range(60):
        fresh = pool[5 * i:5 * i + 5]
        seen = pool[rng.integers(0, 5 * i + 1, 3)]
        step(lk, h, np.concatenate([fresh[:2], [-1], seen, fresh[2:]]))
        grown.add(lk.max_tokens)
    assert len(grown) >= 6 and lk.max_tokens >= 300
    step(lk, h, pool)


@pytest.mark.parametrize("device", _DEVICES)
def test_loaded_full_table_still_grows(device):
    """A checkpoint whose table is nearly full, loaded into a fresh
    auto_grow module: the next batch that overflows it must grow it."""
    src = IntegerLookup(max_tokens=4, auto_grow=True)
    h = History()
    step(src, h, np.arange(100, 111))
    free = src.max_tokens + 1 - src.vocabulary_size()
    # so few new keys that only an exact count of the loaded table can tell
    # that they overflow it
    assert 0 < free and free + 2 <= 0.8 * src.max_tokens
    lk = IntegerLookup(max_tokens=4, auto_grow=True, device=device)
    lk.load_state_dict(src.state_dict())
    assert lk.max_tokens == src.max_tokens
    check(lk, h)
    out = step(lk, h, np.arange(500, 500 + free + 1))
    assert (out > 0).all() and lk.max_tokens > src.max_tokens


# --------------------------------------------------------------------------
# CPU <-> GPU interop
# --------------------------------------------------------------------------

def _interop_keys():
    """Four keys of the wrapping chain, three negative keys and one more:
    eight distinct keys for max_tokens=7, so exactly one overflows."""
    chain = _chain_keys(7, "wrap")
    first = np.concatenate([chain[:4], [-2, -7, _I64_MIN], [2 ** 32]])
    assert np.unique(first).size == 8
    return first, np.concatenate([chain[4:7], [-3]])


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("auto_grow", [False, True])
@pytest.mark.parametrize("start", ["cuda", "cpu"])
def test_interop_device_moves(start, auto_grow):
    other = "cpu" if start == "cuda" else "cuda"
    first, more = _interop_keys()
    lk = IntegerLookup(max_tokens=7, auto_grow=auto_grow, device=start)
    h = History()
    out = step(lk, h, np.concatenate([first, [-1], first[:3]]))
    assert (out[:8] == 0).sum() == (0 if auto_grow else 1)
    lk = lk.to(other)
    step(lk, h, np.concatenate([first[::-1], more, [-1]]))
    lk = lk.to(start)
    step(lk, h, np.concatenate([more, first, [-1, 999, 999]]))


@pytest.mark.gpu
@requires_gpu
@pytest.mark.parametrize("auto_grow", [False, True])
@pytest.mark.parametrize("start", ["cuda", "cpu"])
def test_interop_state_dict(start, auto_grow):
    other = "cpu" if start == "cuda" else "cuda"
    first, more = _interop_keys()
    lk = IntegerLookup(max_tokens=7, auto_grow=auto_grow, device=start)
    h = History()
    step(lk, h, np.concatenate([first, [-1], first[:3]]))
    lk2 = IntegerLookup(max_tokens=7, auto_grow=auto_grow, device=other)
    lk2.load_state_dict(lk.state_dict())
    assert lk2.table_keys.device.type == other
    check(lk2, h)
    step(lk2, h, np.concatenate([more, first[::-1], [-1]]))
    step(lk2, h, np.arange(2000, 2040))
