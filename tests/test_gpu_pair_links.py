"""Pair counts fed from links on the device (``PairCountTable.add_links``,
``pair_links_csr`` in ``pair_counts.hip``) and the GPU engine's online
accumulation.

The reference is ``pair_counts_from_codes(device="cpu")`` on the same links
grouped on the host; every comparison is exact on keys and counts, and the
end-to-end CSVs are compared byte for byte with the ones a summarize step
derives from the same run's saved chain.
"""

import os

import numpy as np
import pytest
import torch

from online_pair_refs import CSV, ON, conf, execute, read, summarized_csv
from dblink_amd import ops
from dblink_amd.analysis import chain as chain_q

pytestmark = pytest.mark.gpu


def _host_counts(rec_ent, rec_gid):
    """Reference counts of one sample: records grouped by entity on the host."""
    rec_ent, rec_gid = np.asarray(rec_ent, np.int64), np.asarray(rec_gid, np.int64)
    if len(rec_ent) == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    order = np.argsort(rec_ent, kind="stable")
    ent = rec_ent[order]
    offsets = np.r_[np.flatnonzero(np.r_[True, ent[1:] != ent[:-1]]), len(ent)]
    return chain_q.pair_counts_from_codes(rec_gid[order].astype(np.int32), offsets,
                                          device="cpu")


def _merged(samples):
    parts = [_host_counts(e, g) for e, g in samples]
    return chain_q._merge_key_counts(np.concatenate([k for k, _ in parts]),
                                     np.concatenate([c for _, c in parts]))


def _dev(a):
    return torch.as_tensor(np.array(a, dtype=np.int64), device="cuda")  # a copy


def _add(tab, rec_ent, rec_gid, E):
    tab.add_links(_dev(rec_ent), _dev(rec_gid), E)
    assert tab.err == 0 and tab.occupied * 2 <= tab.capacity


def _finish(tab):
    keys, counts = tab.finish()
    return keys.cpu().numpy(), counts.cpu().numpy()


def _assert_equal(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.int64
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1])


R, E = 3000, 4000
SIZES = [300, 64, 65] + [2] * 200 + [3] * 57 + [1] * 2000  # 3000 records


@pytest.fixture(scope="module")
def links():
    """(rec_ent, rec_gid): SIZES over entities drawn below 3900 (the last
    100 stay empty), records scrambled, gids a sparse subset of 10^6."""
    rng = np.random.default_rng(11)
    ents = rng.choice(E - 100, size=len(SIZES), replace=False)
    rec_ent = np.repeat(ents, SIZES)
    rec_gid = rng.choice(10**6, size=R, replace=False)
    p = rng.permutation(R)
    rec_ent, rec_gid = rec_ent[p].astype(np.int64), rec_gid[p].astype(np.int64)
    rec_ent.setflags(write=False)
    rec_gid.setflags(write=False)
    return rec_ent, rec_gid


def _relinked(rng, rec_ent, share=0.02):
    out = rec_ent.copy()
    moved = rng.choice(len(out), size=int(share * len(out)), replace=False)
    out[moved] = rng.integers(0, E, size=len(moved))
    return out


@pytest.fixture(scope="module")
def five_samples(links):
    rec_ent, rec_gid = links
    rng = np.random.default_rng(12)
    samples = [rec_ent]
    for _ in range(4):
        samples.append(_relinked(rng, samples[-1]))
    return [(e, rec_gid) for e in samples]


def test_hand_case():
    tab = ops.PairCountTable(device="cuda")
    big = 2**31 - 2
    _add(tab, [3, 3, 0, 5, 3, 0], [10, 4, 7, 2, 9, big], 6)
    keys, counts = _finish(tab)
    assert keys.tolist() == [(4 << 32) | 9, (4 << 32) | 10, (7 << 32) | big,
                             (9 << 32) | 10]
    assert counts.tolist() == [1, 1, 1, 1]
    assert tab.occupied == 4


def test_random_shape(links):
    rec_ent, rec_gid = links
    sizes = np.bincount(rec_ent, minlength=E)
    assert len(rec_ent) == R and sizes.shape == (E,)
    assert sorted(sizes[sizes > 3].tolist()) == [64, 65, 300]
    assert (sizes[-100:] == 0).all() and (sizes == 0).sum() > 1000
    assert (sizes == 1).sum() == 2000
    assert 300 * 299 // 2 == 44850 > 21 * 2048
    assert not (np.diff(rec_ent) >= 0).all()  # scrambled
    assert len(np.unique(rec_gid)) == R and rec_gid.max() > 10 * R
    tab = ops.PairCountTable(device="cuda")
    _add(tab, rec_ent, rec_gid, E)
    want = _host_counts(rec_ent, rec_gid)
    assert len(want[0]) == sum(s * (s - 1) // 2 for s in SIZES)
    _assert_equal(_finish(tab), want)
    assert tab.occupied == len(want[0])


def test_accumulation_and_growth(five_samples):
    tab = ops.PairCountTable(initial_capacity=2, device="cuda")
    for rec_ent, rec_gid in five_samples:
        _add(tab, rec_ent, rec_gid, E)
    want = _merged(five_samples)
    assert want[1].max() == 5 and want[1].min() < 5  # links moved between samples
    _assert_equal(_finish(tab), want)
    assert tab.grow_count > 0 and tab.capacity >= 2 * len(want[0])


def test_permutation_invariance(links):
    rec_ent, rec_gid = links
    p = np.random.default_rng(13).permutation(R)
    a = ops.PairCountTable(device="cuda")
    b = ops.PairCountTable(device="cuda")
    _add(a, rec_ent, rec_gid, E)
    _add(b, rec_ent[p], rec_gid[p], E)
    fa, fb = a.finish(), b.finish()
    assert torch.equal(fa[0], fb[0]) and torch.equal(fa[1], fb[1])


def test_degenerate_inputs():
    tab = ops.PairCountTable(device="cuda")
    _add(tab, [], [], 5)
    _add(tab, [], [], 0)
    assert tab.occupied == 0 and tab.finish()[0].numel() == 0
    # all singletons, not in entity order
    _add(tab, np.arange(200)[::-1] * 3, np.arange(200), 600)
    assert tab.occupied == 0 and tab.finish()[0].numel() == 0
    assert bool((tab.keys == -1).all()) and bool((tab.counts == 0).all())
    # all records in one entity, the last one
    gids = np.random.default_rng(14).permutation(1000)[:200]
    _add(tab, np.full(200, 599), gids, 600)
    want = _host_counts(np.zeros(200), gids)
    assert len(want[0]) == 200 * 199 // 2
    _assert_equal(_finish(tab), want)


def test_gid_out_of_range_is_flagged_and_not_counted(links):
    rec_ent, rec_gid = links
    tab = ops.PairCountTable(device="cuda")
    _add(tab, rec_ent, rec_gid, E)
    before = _finish(tab)
    bad = rec_gid.copy()
    bad[np.flatnonzero(rec_ent == rec_ent[0])[0]] = 2**31
    with pytest.raises(RuntimeError, match=r"error flag 4\b.*rec_gid"):
        tab.add_links(_dev(rec_ent), _dev(bad), E)
    assert tab.err & 4
    _assert_equal(_finish(tab), before)
    # the table goes on counting
    _add(tab, rec_ent, rec_gid, E)
    _assert_equal(_finish(tab), (before[0], 2 * before[1]))


def test_load_round_trip(five_samples):
    whole = ops.PairCountTable(device="cuda")
    first = ops.PairCountTable(device="cuda")
    for i, (rec_ent, rec_gid) in enumerate(five_samples):
        _add(whole, rec_ent, rec_gid, E)
        if i < 3:
            _add(first, rec_ent, rec_gid, E)
    keys, counts = first.finish()
    for saved in ((keys, counts), (keys.cpu().numpy(), counts.cpu().numpy())):
        resumed = ops.PairCountTable(initial_capacity=2, device="cuda")
        resumed.load(*saved)
        assert resumed.occupied == keys.numel()
        assert resumed.occupied * 2 <= resumed.capacity
        for rec_ent, rec_gid in five_samples[3:]:
            _add(resumed, rec_ent, rec_gid, E)
        _assert_equal(_finish(resumed), _finish(whole))
    # loading into a table that already holds the keys adds the counts
    first.load(keys, counts)
    _assert_equal(_finish(first), (keys.cpu().numpy(), 2 * counts.cpu().numpy()))


def test_gpu_engine_end_to_end(tmp_path):
    for name, extra, cutoff in (("all", ON, 0.0),
                                ("half", ON + ", minLinkProbability : 0.5", 0.5)):
        out = str(tmp_path / name)
        project = execute(conf(tmp_path, name, out, records=600, engine="gpu",
                               extra=extra))
        table = chain_q.load_chain(out, 0)
        assert sorted(set(table["iteration"].to_pylist())) == list(range(3, 27, 2))
        assert sorted(set(table["partitionId"].to_pylist())) == [0, 1]
        got = read(os.path.join(out, CSV))
        assert got.count(b"\n") > 10
        assert got == summarized_csv(project, cutoff)


def test_gpu_engine_resume(tmp_path):
    out = str(tmp_path / "two")
    execute(conf(tmp_path, "a", out, records=600, engine="gpu", samples=6))
    project = execute(conf(tmp_path, "b", out, records=600, engine="gpu", samples=6,
                           resume="true"))
    table = chain_q.load_chain(out, 0)
    assert len(set(table["iteration"].to_pylist())) == 12
    assert read(os.path.join(out, CSV)) == summarized_csv(project)
    with np.load(os.path.join(out, "pair-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12
