"""The device cluster-count table (``ClusterCountTable``, the cluster kernels
of ``pair_counts.hip``) and the GPU engine's online sMPC.

The reference is a pure-Python count of the same samples,
``{frozenset(gids): (count, first iteration)}``; members are compared as
sets (the arena order is arbitrary), keys bitwise with the numpy arm, and
the end-to-end file with the chain queries over the run's own saved chain.
Every comparison is exact.
"""

import os

import numpy as np
import pytest
import torch

import cluster_chain_refs as ccr
from dblink_amd import ops
from dblink_amd.analysis import chain as chain_q

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.int64), device="cuda")  # a copy


def _add(tab, rec_ent, rec_gid, E, iteration):
    tab.add_links(_dev(rec_ent), _dev(rec_gid), E, iteration)
    assert tab.err == 0 and tab.occupied * 2 <= tab.capacity
    assert tab.arena_used <= tab.arena_capacity


def _finish(tab):
    out = tab.finish()
    assert [t.dtype for t in out] == [torch.int64] * 4 + [torch.int32]
    keys, counts, first, offsets, members = (t.cpu().numpy() for t in out)
    assert len(keys) == tab.occupied == len(counts) == len(first) == len(offsets) - 1
    assert np.array_equal(keys, np.unique(keys))  # sorted, distinct
    assert offsets[0] == 0 and offsets[-1] == len(members) == tab.arena_used
    return keys, counts, first, offsets, members


def _run(samples, E, **kw):
    tab = ops.ClusterCountTable(device="cuda", **kw)
    for rec_ent, rec_gid, iteration in samples:
        _add(tab, rec_ent, rec_gid, E, iteration)
    return tab, _finish(tab)


def _assert_exact(got, samples):
    """Member sets, counts and first iterations equal the Python reference;
    every key is the numpy arm's key of its member set, bitwise."""
    want = ccr.reference_counts(samples)
    assert ccr.triples(*got) == want
    host = ccr.host_counts(samples)
    for x, y in zip(got[:4], host[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)


R, E = 3000, 1200


@pytest.fixture(scope="module")
def five_samples():
    samples = ccr.relinked_samples(R, E, 5, 0.02, seed=31, first_iteration=4, step=3)
    for rec_ent, rec_gid, _ in samples:
        rec_ent.setflags(write=False)
        rec_gid.setflags(write=False)
    return samples


def test_hand_case():
    big = 2**31 - 2
    gids = [10, 4, 7, 2, 9, big]
    samples = [(np.array([0, 0, 1, 1, 2, 2]), np.array(gids), 5),
               (np.array([0, 0, 1, 2, 2, 2]), np.array(gids), 7),
               (np.array([2, 2, 1, 1, 0, 0]), np.array(gids), 9)]
    tab, got = _run(samples, 3)
    assert ccr.triples(*got) == {
        frozenset({10, 4}): (3, 5), frozenset({7, 2}): (2, 5),
        frozenset({9, big}): (2, 5), frozenset({7}): (1, 7),
        frozenset({2, 9, big}): (1, 7)}
    assert tab.occupied == 5 and tab.arena_used == 10
    # keys: _mpc_keys_numpy over the gids, bitwise
    sets = [[10, 4], [2, 7], [big, 9], [7], [9, 2, big]]
    codes = np.array([g for s in sets for g in s], dtype=np.uint64)
    off = np.r_[0, np.cumsum([len(s) for s in sets])].astype(np.int64)
    with np.errstate(over="ignore"):
        raw = chain_q._mpc_keys_numpy(codes, off, np.diff(off))
    assert np.array_equal(got[0], np.sort(raw.view(np.int64)))
    _assert_exact(got, samples)


def test_random_shape(five_samples):
    sizes = np.bincount(five_samples[0][0], minlength=E)
    assert (sizes == 0).any() and (sizes == 1).any() and sizes.max() >= 7
    tab, got = _run(five_samples, E)
    _assert_exact(got, five_samples)
    assert got[1].max() == 5 and got[1].min() == 1  # clusters came and went
    assert sorted(set(got[2].tolist())) == [4, 7, 10, 13, 16]
    assert tab.grow_count == 0


def test_growth(five_samples):
    tab, got = _run(five_samples, E, initial_capacity=2, initial_arena=1)
    _assert_exact(got, five_samples)
    assert tab.grow_count > 0 and tab.err == 0
    assert tab.capacity >= 2 * len(got[0]) and tab.arena_capacity >= len(got[4])
    assert tab.nbytes == tab.capacity * 28 + tab.arena_capacity * 4


def test_permutation_invariance(five_samples):
    rng = np.random.default_rng(32)
    relabel = rng.permutation(E)
    shuffled = []
    for rec_ent, rec_gid, iteration in five_samples:
        p = rng.permutation(R)
        shuffled.append((relabel[rec_ent[p]], rec_gid[p], iteration))
    _, a = _run(five_samples, E)
    _, b = _run(shuffled, E)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert ccr.triples(*a) == ccr.triples(*b)


def test_large_cluster():
    rng = np.random.default_rng(33)
    gid = rng.choice(10**6, size=1200, replace=False)
    ent = np.r_[np.full(700, 17), 100 + np.arange(500)]
    p = rng.permutation(1200)
    ent, gid = ent[p], gid[p]
    moved = ent.copy()
    moved[np.flatnonzero(ent == 17)[:3]] = 50  # 697 stay, 3 form a new cluster
    samples = [(ent, gid, 1), (moved, gid, 2), (ent, gid, 3)][:2]
    tab, got = _run(samples, 600, initial_arena=16)
    _assert_exact(got, samples)
    assert sorted(np.diff(got[3]).tolist())[-3:] == [3, 697, 700]
    assert len(got[0]) == 503 and tab.arena_used == 1900


def test_degenerate_inputs():
    tab = ops.ClusterCountTable(device="cuda")
    _add(tab, [], [], 5, 1)
    _add(tab, [], [], 0, 2)
    assert tab.occupied == 0 and all(t.numel() == 0 for t in tab.finish()[:3])
    assert tab.finish()[3].tolist() == [0]
    # every record a singleton, not in entity order, empty entities in between
    single = (np.arange(200)[::-1] * 3, np.arange(200) + 1000, 3)
    # every record in one entity, the last one
    gids = np.random.default_rng(34).permutation(1000)[:200]
    one = (np.full(200, 599), gids, 4)
    samples = [single, one, single]
    samples[2] = (single[0], single[1], 5)
    for rec_ent, rec_gid, iteration in samples:
        _add(tab, rec_ent, rec_gid, 600, iteration)
    got = _finish(tab)
    _assert_exact(got, samples)
    assert len(got[0]) == 201 and sorted(got[1].tolist())[:2] == [1, 2]


@pytest.mark.parametrize("what", ["gid", "entity"])
def test_bad_link_is_flagged_and_not_counted(five_samples, what):
    rec_ent, rec_gid, _ = five_samples[0]
    tab = ops.ClusterCountTable(device="cuda")
    _add(tab, rec_ent, rec_gid, E, 1)
    before = _finish(tab)
    bad_ent, bad_gid = rec_ent.copy(), rec_gid.copy()
    if what == "gid":
        bad_gid[5] = 2**31
    else:
        bad_ent[5] = E
    with pytest.raises(RuntimeError, match=r"error flag 4\b.*rec_gid"):
        tab.add_links(_dev(bad_ent), _dev(bad_gid), E, 2)
    assert tab.err & 4
    for x, y in zip(_finish(tab), before):
        assert np.array_equal(x, y)
    # the table goes on counting
    _add(tab, rec_ent, rec_gid, E, 3)
    after = _finish(tab)
    assert np.array_equal(after[1], 2 * before[1])
    for i in (0, 2, 3):
        assert np.array_equal(after[i], before[i])


def test_gpu_engine_end_to_end(tmp_path):
    out = str(tmp_path / "run")
    ccr.execute(ccr.conf(tmp_path, "run", out, engine="gpu"))
    want, table = ccr.chain_smpc(out)
    assert sorted(set(table["iteration"].to_pylist())) == list(range(3, 27, 2))
    got = ccr.written_smpc(out)
    assert got == want and len(got) > 100
    with np.load(os.path.join(out, "cluster-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12 and z["counts"].min() < 12 == z["counts"].max()


def test_gpu_engine_resume(tmp_path):
    out = str(tmp_path / "two")
    ccr.execute(ccr.conf(tmp_path, "a", out, engine="gpu", samples=6))
    ccr.execute(ccr.conf(tmp_path, "b", out, engine="gpu", samples=6, resume="true"))
    want, table = ccr.chain_smpc(out)
    assert len(set(table["iteration"].to_pylist())) == 12
    assert ccr.written_smpc(out) == want
    with np.load(os.path.join(out, "cluster-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12
