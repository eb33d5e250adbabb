"""IntegerLookup semantics tests (CPU path; GPU path tested in test_gpu)."""

import torch

from distributed_embeddings_amd import IntegerLookup


def test_assigns_incremental_values():
    lk = IntegerLookup(max_tokens=10)
    out = lk(torch.tensor([100, 200, 100, 300]))
    assert out.tolist() == [1, 2, 1, 3]
    # same keys again -> same values
    out2 = lk(torch.tensor([300, 200, 100]))
    assert out2.tolist() == [3, 2, 1]


def test_oov_when_full():
    lk = IntegerLookup(max_tokens=2)
    out = lk(torch.tensor([10, 20, 30, 40]))
    assert out.tolist()[:2] == [1, 2]
    assert out.tolist()[2] == 0 and out.tolist()[3] == 0


def test_counts():
    lk = IntegerLookup(max_tokens=5)
    lk(torch.tensor([7, 7, 7, 9]))
    assert int(lk.counts[1]) == 3  # key 7 -> value 1 seen 3x
    assert int(lk.counts[2]) == 1


def test_get_vocabulary():
    lk = IntegerLookup(max_tokens=5)
    lk(torch.tensor([42, 17, 99]))
    vocab = lk.get_vocabulary()
    assert vocab == [-1, 42, 17, 99]
    assert lk.vocabulary_size() == 4  # incl. OOV slot
    # negative keys are ordinary keys; -1 is the OOV token and adds nothing
    out = lk(torch.tensor([-1, -5, 17, -1]))
    assert out.tolist() == [0, 4, 2, 0]
    vocab = lk.get_vocabulary()
    assert vocab == [-1, 42, 17, 99, -5]
    assert len(vocab) == lk.vocabulary_size() == 5


def test_nd_input_shape():
    lk = IntegerLookup(max_tokens=10)
    out = lk(torch.tensor([[5, 6], [5, 8]]))
    assert out.shape == (2, 2)
    assert out[0, 0] == out[1, 0]


def test_state_roundtrip_through_buffers():
    lk = IntegerLookup(max_tokens=5)
    lk(torch.tensor([42, 17]))
    sd = lk.state_dict()
    lk2 = IntegerLookup(max_tokens=5)
    lk2.load_state_dict(sd)
    out = lk2(torch.tensor([17, 42]))
    assert out.tolist() == [2, 1]


def test_state_dict_round_trip():
    """The hash lives in registered buffers: checkpoint + fresh module must
    resolve the same keys to the same values (no re-insertion)."""
    import torch
    from distributed_embeddings_amd import IntegerLookup
    lk = IntegerLookup(max_tokens=100)
    keys = torch.tensor([11, 22, 33, 44, 11])
    vals1 = lk(keys)
    sd = lk.state_dict()
    lk2 = IntegerLookup(max_tokens=100)
    lk2.load_state_dict(sd)
    vals2 = lk2(keys)
    assert torch.equal(vals1[:4], vals2[:4])
    assert lk2.vocabulary_size() == lk.vocabulary_size()
    # unseen key gets a NEW value, not a collision with restored ones
    v_new = int(lk2(torch.tensor([99]))[0])
    assert v_new not in vals2[:4].tolist()


def test_cpu_path_vectorized_1m_keys():
    """the CPU path must handle 1M keys in seconds (it is
    numpy-vectorized probing, not a per-element Python loop)."""
    import time
    lk = IntegerLookup(max_tokens=1_200_000)
    keys = torch.randint(0, 1 << 62, (1_000_000,))
    t0 = time.time()
    out = lk(keys)
    assert time.time() - t0 < 30.0
    assert torch.equal(out, lk(keys))
    assert lk.vocabulary_size() == len(set(keys.tolist())) + 1


def test_auto_grow_cpu():
    """auto_grow=True rehashes past the max_tokens guess instead of OOV."""
    lk = IntegerLookup(max_tokens=4, auto_grow=True)
    out = lk(torch.arange(100, 120))
    assert lk.max_tokens >= 20
    assert (out > 0).all()
    assert torch.equal(out, lk(torch.arange(100, 120)))


def test_auto_grow_preserves_assignments():
    lk = IntegerLookup(max_tokens=8, auto_grow=True)
    a = lk(torch.tensor([5, 6, 7]))
    lk(torch.arange(1000, 1030))  # force growth
    assert torch.equal(a, lk(torch.tensor([5, 6, 7])))
    # counts survive growth: keys 5/6/7 seen twice each
    for v in a.tolist():
        assert int(lk.counts[v]) == 2


def test_grown_state_dict_loads_into_fresh_module():
    lk = IntegerLookup(max_tokens=4, auto_grow=True)
    out = lk(torch.arange(50, 70))
    lk2 = IntegerLookup(max_tokens=4, auto_grow=True)
    lk2.load_state_dict(lk.state_dict())
    assert lk2.max_tokens == lk.max_tokens
    assert torch.equal(lk2(torch.arange(50, 70)), out)
