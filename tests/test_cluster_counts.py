"""Cluster counts taken during sampling (``OnlineClusterCounts``) and their
resolution into most probable clusters, on the host: the numpy arm against
``chain.most_probable_clusters`` / ``shared_most_probable_clusters`` over a
chain table of the same samples in iteration order, the merge of two
accumulators, the EMPTY-key remap, and the CPU engine end to end (resume,
stale files, no saved chain, world 2 under gloo, the default surface).

Every comparison is exact: sets of record ids, integer counts, and
frequencies that are one integer division."""

import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_chain_refs as ccr
from cluster_chain_refs import NO_CHAIN, ON, SMPC
from cluster_chain_refs import conf as _conf
from cluster_chain_refs import execute as _execute
from dblink_amd.analysis import chain as chain_q
from dblink_amd.api import project as prj
from dblink_amd.engine import sampler as sampler_m
from dblink_amd.engine.cluster_accumulator import OnlineClusterCounts
from dblink_amd.engine.cpu_engine import SamplerFlags
from dblink_amd.utils import hocon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A, B, C, D = 7, 2, 11, 5
# record A lies 3 times in {A, B} (first at iteration 1) and 3 times in
# {A, C} (first at iteration 2): a genuine tie, as is B's and C's
HAND = [
    (np.array([0, 0, 1, 2]), np.array([A, B, C, D]), 1),
    (np.array([0, 1, 0, 2]), np.array([A, B, C, D]), 2),
    (np.array([4, 1, 4, 2]), np.array([A, B, C, D]), 3),
    (np.array([3, 1, 3, 2]), np.array([C, B, A, D]), 4),
    (np.array([1, 1, 0, 2]), np.array([B, A, C, D]), 5),
    (np.array([2, 2, 0, 1]), np.array([A, B, C, D]), 6),
]


def _random():
    return ccr.relinked_samples(300, 120, 12, 0.05, seed=21, first_iteration=3, step=2)


# the same ties over gids far apart: the resolution's path without a dense
# table of positions
SPARSE = [(e, g * 10**8, it) for e, g, it in HAND]


@pytest.mark.parametrize("samples", [_random(), HAND, SPARSE],
                         ids=["random", "tie", "sparse-gids"])
def test_resolution_equals_the_chain_queries(samples):
    S = len(samples)
    merged = ccr.host_counts(samples)
    assert ccr.triples(*merged) == ccr.reference_counts(samples)
    assert np.array_equal(merged[0], np.unique(merged[0]))  # sorted, distinct
    table = ccr.chain_table(samples)
    ids = {int(g): str(g) for s in samples for g in s[1]}

    want = chain_q.most_probable_clusters(table)
    assert chain_q.mpc_dict(*merged, S, ids=ids) == want
    got = chain_q.smpc_from_cluster_counts(*merged, S, ids=ids)
    assert ccr.frozen(got) == ccr.frozen(chain_q.shared_most_probable_clusters(table))
    assert ccr.frozen(got) == ccr.frozen(chain_q.shared_most_probable_clusters_fast(table))

    gids, best_key, best_count, best_freq = chain_q.mpc_from_cluster_counts(*merged, S)
    assert gids.tolist() == sorted({int(g) for s in samples for g in s[1]})
    by_key = dict(zip(merged[0].tolist(), range(len(merged[0]))))
    for g, k, c, f in zip(gids.tolist(), best_key.tolist(), best_count.tolist(),
                          best_freq.tolist()):
        i = by_key[k]
        members = frozenset(str(m) for m in merged[4][merged[3][i]:merged[3][i + 1]])
        assert (members, f) == want[str(g)] and f == c / S and c == merged[1][i]


def test_tie_goes_to_the_cluster_seen_first():
    merged = ccr.host_counts(HAND)
    ref = ccr.reference_counts(HAND)
    assert ref[frozenset({A, B})] == (3, 1) and ref[frozenset({A, C})] == (3, 2)
    assert ref[frozenset({B})] == (3, 2) and ref[frozenset({C})] == (3, 1)
    mpc = chain_q.mpc_dict(*merged, 6)
    assert mpc[A] == (frozenset({A, B}), 0.5)
    assert mpc[B] == (frozenset({A, B}), 0.5)
    assert mpc[C] == (frozenset({C}), 0.5)
    assert ccr.frozen(chain_q.smpc_from_cluster_counts(*merged, 6)) == {
        frozenset({A, B}), frozenset({C}), frozenset({D})}
    # the order of the parts does not matter, only `first`
    back = chain_q.merge_cluster_counts(
        [ccr.host_counts([s]) for s in reversed(HAND)])
    assert chain_q.mpc_dict(*back, 6) == mpc


def test_merge_of_two_accumulators():
    samples = _random()
    whole, left, right = (OnlineClusterCounts(merge_every=5) for _ in range(3))
    for s, (rec_ent, rec_gid, it) in enumerate(samples):
        order = np.argsort(rec_ent, kind="stable")
        ent, gid = rec_ent[order], rec_gid[order]
        side = (ent + s) % 2 == 0  # alternates by entity, and from sample to sample
        for acc, keep in ((whole, np.ones(len(ent), bool)), (left, side), (right, ~side)):
            e = ent[keep]
            off = np.r_[np.flatnonzero(np.r_[True, e[1:] != e[:-1]]), len(e)]
            acc.add_host(gid[keep], off, it)
    a, b, w = left.local_counts(), right.local_counts(), whole.local_counts()
    # the same cluster was counted on both sides
    assert len(np.intersect1d(a[0], b[0])) > 50
    merged = chain_q.merge_cluster_counts([a, b])
    for x, y in zip(merged[:4], w[:4]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert ccr.triples(*merged) == ccr.triples(*w) == ccr.reference_counts(samples)
    assert chain_q.merge_cluster_counts([])[3].tolist() == [0]


def test_empty_key_is_remapped(monkeypatch):
    gids, off = np.array([4, 9, 1]), np.array([0, 2, 3])
    real = chain_q.cluster_keys_numpy(gids, off)
    with np.errstate(over="ignore"):
        raw = chain_q._mpc_keys_numpy(gids.astype(np.uint64), off, np.diff(off))
    assert np.array_equal(real.view(np.uint64), raw)  # nothing else changes a key

    def all_ones_first(codes, off64, sizes):
        out = raw.copy()
        out[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
        return out

    monkeypatch.setattr(chain_q, "_mpc_keys_numpy", all_ones_first)
    keys = chain_q.cluster_keys_numpy(gids, off)
    assert keys.dtype == np.int64
    assert keys.view(np.uint64).tolist() == [0xFFFFFFFFFFFFFFFE, int(raw[1])]
    part = chain_q.cluster_counts_of_sample(gids, off, 5)
    assert -1 not in part[0].tolist() and -2 in part[0].tolist()


# ---- CPU engine end to end -----------------------------------------------------


def test_cpu_engine_end_to_end(tmp_path):
    out = str(tmp_path / "run")
    _execute(_conf(tmp_path, "run", out))
    want, table = ccr.chain_smpc(out)
    assert sorted(set(table["iteration"].to_pylist())) == list(range(3, 27, 2))
    got = ccr.written_smpc(out)
    assert got == want and len(got) > 100
    assert sorted(r for c in got for r in c) == sorted(
        {r for row in table["linkageStructure"].to_pylist() for c in row for r in c})
    # clusters move during the run, or the counts would not test accumulation
    with np.load(os.path.join(out, "cluster-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12 and int(z["iteration"]) == 25
        assert z["counts"].min() < 12 == z["counts"].max()
        assert z["first"].min() == 3 < z["first"].max()


def test_resume_counts_the_whole_chain(tmp_path):
    out = str(tmp_path / "two")
    # a checkpoint between samples too: the counts file then trails the state
    _execute(_conf(tmp_path, "a", out, samples=6, ckpt=4))
    _execute(_conf(tmp_path, "b", out, samples=6, resume="true"))
    want, table = ccr.chain_smpc(out)
    assert len(set(table["iteration"].to_pylist())) == 12
    assert ccr.written_smpc(out) == want
    with np.load(os.path.join(out, "cluster-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12
        assert int(z["iteration"]) == max(table["iteration"].to_pylist())


def test_stale_or_missing_counts_are_refused(tmp_path):
    out = str(tmp_path / "run")
    _execute(_conf(tmp_path, "a", out, records=60, samples=3))
    path = os.path.join(out, "cluster-counts-rank0.npz")
    with np.load(path) as z:
        saved = {k: z[k] for k in z.files}
    rows = chain_q.load_chain(out, 0).num_rows
    again = _conf(tmp_path, "b", out, records=60, samples=2, resume="true")

    os.remove(path)
    with pytest.raises(ValueError, match=r"cluster-counts-rank0\.npz"):
        _execute(again)
    ahead = dict(saved, iteration=saved["iteration"] + 2)
    np.savez(path, **ahead)
    with pytest.raises(ValueError, match=r"cluster-counts-rank0\.npz"):
        _execute(again)
    behind = dict(saved, state_iteration=saved["state_iteration"] - 2,
                  iteration=saved["iteration"] - 2)
    np.savez(path, **behind)
    with pytest.raises(ValueError, match=r"cluster-counts-rank0\.npz"):
        _execute(again)
    # nothing was appended by the refused runs; the right file resumes
    assert chain_q.load_chain(out, 0).num_rows == rows
    np.savez(path, **saved)
    _execute(again)
    assert ccr.written_smpc(out) == ccr.chain_smpc(out)[0]


def test_run_without_a_saved_chain(tmp_path):
    kept, bare = str(tmp_path / "kept"), str(tmp_path / "bare")
    _execute(_conf(tmp_path, "kept", kept))
    _execute(_conf(tmp_path, "bare", bare, extra=ON + NO_CHAIN, steps=ccr.EVALUATE))
    assert os.path.isdir(os.path.join(kept, "linkage-chain.parquet"))
    assert not os.path.exists(os.path.join(bare, "linkage-chain.parquet"))
    with open(os.path.join(kept, SMPC), "rb") as f, \
            open(os.path.join(bare, SMPC), "rb") as g:
        assert f.read() == g.read()
    assert ccr.written_smpc(bare) == ccr.chain_smpc(kept)[0]
    # diagnostics and the state are written as before
    assert {"diagnostics.csv", "driver-state", "partitions-state-rank00000.npz",
            "cluster-counts-rank0.npz", "evaluation-results.txt"} <= set(os.listdir(bare))
    def diagnostics(out):  # without the wall-clock column
        with open(os.path.join(out, "diagnostics.csv")) as f:
            rows = [line.rstrip("\n").split(",") for line in f]
        assert rows[0][1] == "systemTime-ms" and len(rows) == 13
        return [r[:1] + r[2:] for r in rows]

    assert diagnostics(bare) == diagnostics(kept)
    with open(os.path.join(bare, "evaluation-results.txt")) as f:
        text = f.read()
    assert "Pairwise metrics" in text and "Cluster metrics" in text


def test_no_chain_and_no_summary_is_a_config_error(tmp_path):
    out = str(tmp_path / "none")
    bad = _conf(tmp_path, "bad", out, records=60, extra=NO_CHAIN)
    cfg = hocon.parse_file(bad)
    project = prj.Project(cfg, rank=0, world_size=1)
    with pytest.raises(ValueError, match="saveLinkageChain"):
        prj.parse_steps(cfg, project)
    # an online pair summary is enough
    ok = _conf(tmp_path, "ok", out, records=60,
               extra=NO_CHAIN + ", pairwiseLinkProbabilities : true")
    step = prj.parse_steps(hocon.parse_file(ok), project)[0]
    assert step.save_linkage_chain is False and step.pairwise_link_probabilities


def test_hocon_parameters_and_defaults(tmp_path):
    out = str(tmp_path / "off")
    on = _conf(tmp_path, "on", out, records=60, extra=ON + NO_CHAIN)
    cfg = hocon.parse_file(on)
    project = prj.Project(cfg, rank=0, world_size=1)
    step = prj.parse_steps(cfg, project)[0]
    assert step.shared_most_probable_clusters is True
    assert step.save_linkage_chain is False
    assert "shared most probable clusters" in step.mk_string()
    assert "not saving the linkage chain" in step.mk_string()

    off = _conf(tmp_path, "off", out, records=60, samples=2, extra="")
    step = prj.parse_steps(hocon.parse_file(off), project)[0]
    assert step.shared_most_probable_clusters is False
    assert step.save_linkage_chain is True
    assert "most probable" not in step.mk_string() and "chain from" in step.mk_string()
    project = _execute(off)
    assert sorted(os.listdir(out)) == [
        "diagnostics.csv", "driver-state", "linkage-chain.parquet",
        "partitions-state-rank00000.npz"]

    # sample() with the earlier positional arguments
    state = project.saved_state()
    before = state.iteration
    sampler_m.sample(project.engine(), state, 2, out, 0, 1, 20, 10,
                     SamplerFlags.for_sampler("PCG-I"), 0, True, None)
    assert state.iteration == before + 2
    assert not any(f.startswith("cluster-counts") or f == SMPC for f in os.listdir(out))


WORKER = r"""
import sys
sys.path.insert(0, "__ROOT__")
from dblink_amd.api.cli import main
raise SystemExit(main(["__CONF__"]))
"""


def _run_workers(script, world=2, timeout=600):
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(31500 + os.getpid() % 1000),
               WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo", DBLINK_BACKEND="gloo")
    procs = [subprocess.Popen([sys.executable, "-c", script],
                              env=dict(env, RANK=str(r), LOCAL_RANK=str(r)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=timeout)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, f"worker failed:\n{o}"


def test_world_two_merges_the_ranks(tmp_path):
    out = str(tmp_path / "w2")
    conf = _conf(tmp_path, "w2", out, levels=2, split='"fname_c1", "lname_c1"',
                 samples=8)
    _run_workers(WORKER.replace("__ROOT__", ROOT).replace("__CONF__", conf))
    want, table = ccr.chain_smpc(out)
    assert sorted(set(table["partitionId"].to_pylist())) == [0, 1, 2, 3]
    assert ccr.written_smpc(out) == want and len(want) > 100
    files = sorted(f for f in os.listdir(out) if f.startswith("cluster-counts-rank"))
    assert files == ["cluster-counts-rank0.npz", "cluster-counts-rank1.npz"]
    sizes = []
    for f in files:
        with np.load(os.path.join(out, f)) as z:
            assert int(z["S"]) == 8
            sizes.append(len(z["keys"]))
    assert min(sizes) > 0
