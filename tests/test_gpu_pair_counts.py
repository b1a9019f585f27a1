"""The pair-count hash table (``pair_counts.hip``) against the numpy arm.

The reference is ``device="cpu"``, which ``test_pair_probabilities`` holds to
an itertools oracle; equality is exact on keys and counts. The 6000-record
cluster is checked analytically on the device: it is the smallest size at
which an fp32 (or un-fixed-up) triangular root mis-decodes.
"""

import numpy as np
import pytest
import torch

import pair_chain_refs as pcr
from dblink_amd import ops
from dblink_amd.analysis import chain as chain_q

pytestmark = pytest.mark.gpu

BIG = 6000
BIG_PAIRS = BIG * (BIG - 1) // 2  # 17,997,000 > 2^24


def _both_arms(codes, offsets, **kw):
    codes = np.asarray(codes, dtype=np.int32)
    offsets = np.asarray(offsets, dtype=np.int64)
    ref = chain_q.pair_counts_from_codes(codes, offsets, device="cpu")
    got = chain_q.pair_counts_from_codes(codes, offsets, device="cuda", **kw)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(got[1], ref[1])
    return got


@pytest.fixture(scope="module")
def random_codes():
    table = pcr.chain_table(pcr.random_samples())
    _, codes, offsets, _ = chain_q._chain_rank_codes(table)
    return table, codes, offsets


@pytest.fixture(scope="module")
def big_keys():
    """Sorted keys of all pairs of codes 0..5999, built on the device."""
    iu = torch.triu_indices(BIG, BIG, 1, device="cuda")
    return (iu[0] << 32) | iu[1]  # row-major upper triangle: already sorted


def _add_once(codes, offsets):
    tab = ops.PairCountTable(device="cuda")
    tab.add(torch.as_tensor(codes, dtype=torch.int32, device="cuda"),
            torch.as_tensor(offsets, dtype=torch.int64, device="cuda"))
    assert tab.err == 0 and tab.occupied * 2 <= tab.capacity
    return tab


def test_triangular_decode_at_every_small_size():
    sizes = [0, 1, 2, 3, 4, 5, 63, 64, 65, 128, 129]
    offsets = np.r_[0, np.cumsum(sizes)]
    codes = np.random.default_rng(1).permutation(int(offsets[-1]))
    keys, counts = _both_arms(codes, offsets)
    assert len(keys) == sum(s * (s - 1) // 2 for s in sizes)
    assert (counts == 1).all()


def test_decode_beyond_fp32(big_keys):
    tab = _add_once(torch.arange(BIG), [0, BIG])
    assert tab.occupied == BIG_PAIRS
    keys, counts = tab.finish()
    assert keys.numel() == BIG_PAIRS
    assert bool((counts == 1).all())
    assert torch.equal(keys, big_keys)


def test_big_cluster_among_many_small_ones(big_keys):
    n_small = 100_000
    small = BIG + torch.arange(2 * n_small)  # codes above the big cluster's
    codes = torch.cat([small[:n_small], torch.arange(BIG), small[n_small:]])
    sizes = torch.cat([torch.full((n_small // 2,), 2), torch.tensor([BIG]),
                       torch.full((n_small // 2,), 2)])
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(sizes, 0)])
    tab = _add_once(codes, offsets)  # one call: 18,097,000 pair indices
    keys, counts = tab.finish()
    small_d = small.to("cuda").view(-1, 2)
    want = torch.cat([big_keys, (small_d[:, 0] << 32) | small_d[:, 1]])
    assert tab.occupied == want.numel() == BIG_PAIRS + n_small
    assert torch.equal(keys, want)  # every small key is above every big one
    assert bool((counts == 1).all())


def test_accumulation_across_samples_under_contention():
    S = 300
    base = np.arange(50, dtype=np.int32)
    offsets = np.arange(0, 50 * S + 1, 5)
    keys, counts = _both_arms(np.tile(base, S), offsets)
    assert len(keys) == 10 * 10 and (counts == S).all()
    # record 0 sits with 5..9 instead of 1..4 in every other sample
    moved = np.r_[1:5, 0, 5:50].astype(np.int32)
    codes = np.concatenate([base if s % 2 == 0 else moved for s in range(S)])
    offs = np.concatenate([(np.arange(0, 50, 5) if s % 2 == 0 else
                            np.r_[0, 4, np.arange(10, 50, 5)]) + 50 * s
                           for s in range(S)] + [[50 * S]])
    keys, counts = _both_arms(codes, offs)
    with_zero = (keys >> 32) == 0
    assert sorted((keys[with_zero] & 0xFFFFFFFF).tolist()) == list(range(1, 10))
    assert (counts[with_zero] == S // 2).all()
    assert (counts[~with_zero] == S).all() and (~with_zero).sum() == 6 + 10 + 8 * 10


def test_growth_rehash_and_never_full(random_codes):
    _, codes, offsets = random_codes
    seen = []

    def after_add(tab):
        assert tab.err == 0
        assert tab.occupied * 2 <= tab.capacity
        assert tab.capacity & (tab.capacity - 1) == 0
        seen.append((tab.capacity, tab.grow_count))

    keys, _ = _both_arms(codes, offsets, chunk_pairs=32, initial_capacity=16,
                         after_add=after_add)
    capacity, grow_count = seen[-1]
    assert capacity >= 2 * len(keys) and capacity & (capacity - 1) == 0
    assert grow_count > 1
    assert [c for c, _ in seen] == sorted(c for c, _ in seen)
    assert len(seen) > 100  # many chunks, each at most 32 pairs or one cluster


def test_order_independence(random_codes):
    _, codes, offsets = random_codes
    rng = np.random.default_rng(5)
    clusters = [codes[offsets[c]:offsets[c + 1]] for c in range(len(offsets) - 1)]
    shuffled = [rng.permutation(clusters[c]) for c in rng.permutation(len(clusters))]
    s_offsets = np.r_[0, np.cumsum([len(c) for c in shuffled])]
    a = _add_once(codes, offsets).finish()
    b = _add_once(np.concatenate(shuffled), s_offsets).finish()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_duplicate_member_codes_are_no_pair():
    keys, counts = _both_arms([3, 3, 5, 7, 7], [0, 3, 5])
    assert keys.tolist() == [(3 << 32) | 5] and counts.tolist() == [2]


def test_api_level_equality(random_codes):
    table, _, _ = random_codes
    cpu = chain_q.pairwise_link_probabilities(table, device="cpu")
    gpu = chain_q.pairwise_link_probabilities(table, device="cuda")
    assert len(cpu) > 0 and gpu.equals(cpu)
    half = chain_q.pairwise_link_probabilities(table, min_probability=0.5, device="cuda")
    assert half.equals(cpu[cpu.probability >= 0.5].reset_index(drop=True))
