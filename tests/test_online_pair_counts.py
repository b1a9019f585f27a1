"""Pairwise link counts taken during sampling (``OnlinePairCounts``) on the
CPU engine: the CSV of ``pairwiseLinkProbabilities = true`` against the one
derived from the same run's saved chain, across a resume, with stale or
missing count files, at world 2 under gloo, and the default-off surface.

Every comparison is exact: bytes of the CSV, integer counts."""

import os
import subprocess
import sys

import numpy as np
import pytest

import pair_chain_refs as pcr
from online_pair_refs import CSV, ON
from online_pair_refs import conf as _conf
from online_pair_refs import execute as _execute
from online_pair_refs import read as _read
from online_pair_refs import summarized_csv as _summarized_csv
from dblink_amd.analysis import chain as chain_q
from dblink_amd.api import project as prj
from dblink_amd.engine import sampler as sampler_m
from dblink_amd.engine.cpu_engine import SamplerFlags
from dblink_amd.utils import hocon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chain_samples(table):
    """The chain table -> [(iteration, {pid: clusters})] for the oracle."""
    samples = {}
    for row in table.to_pylist():
        samples.setdefault(row["iteration"], {})[row["partitionId"]] = row["linkageStructure"]
    return sorted(samples.items())


def test_cpu_engine_end_to_end(tmp_path):
    out = str(tmp_path / "run")
    project = _execute(_conf(tmp_path, "run", out))
    table = chain_q.load_chain(out, 0)
    iterations = sorted(set(table["iteration"].to_pylist()))
    assert iterations == list(range(3, 27, 2))  # 12 samples, no iteration 0
    assert sorted(set(table["partitionId"].to_pylist())) == [0, 1]

    got = _read(os.path.join(out, CSV))
    assert got == _summarized_csv(project)
    rows = chain_q.read_pairwise_link_probabilities(out)
    want = pcr.rows_of(chain_q.pairwise_link_counts(table, device="cpu"))
    assert len(want) > 0 and want == pcr.oracle_counts(_chain_samples(table))
    assert list(zip(rows.recordId1, rows.recordId2)) == [w[:2] for w in want]
    assert rows.probability.tolist() == [w[2] / 12 for w in want]
    # pairs move during the run, or the counts would not test accumulation
    assert min(w[2] for w in want) < 12 == max(w[2] for w in want)

    half = str(tmp_path / "half")
    project = _execute(_conf(tmp_path, "half", half,
                             extra=ON + ", minLinkProbability : 0.5"))
    got = _read(os.path.join(half, CSV))
    assert got == _summarized_csv(project, 0.5)
    # this chain's links are all above 0.5; a cutoff of 1 drops some
    sure = str(tmp_path / "sure")
    project = _execute(_conf(tmp_path, "sure", sure,
                             extra=ON + ", minLinkProbability : 1.0"))
    got = _read(os.path.join(sure, CSV))
    assert got == _summarized_csv(project, 1.0)
    assert got != _summarized_csv(project, 0.0)
    assert "pairwise link probabilities" in prj.parse_steps(
        hocon.parse_file(str(tmp_path / "half.conf")), project)[0].mk_string()


def test_iteration_zero_sample_is_counted(tmp_path):
    out = str(tmp_path / "zero")
    project = _execute(_conf(tmp_path, "zero", out, records=60, samples=4, burnin=0))
    table = chain_q.load_chain(out, 0)
    assert sorted(set(table["iteration"].to_pylist())) == [0, 2, 4, 6, 8]
    assert _read(os.path.join(out, CSV)) == _summarized_csv(project)
    with np.load(os.path.join(out, "pair-counts-rank0.npz")) as z:
        assert int(z["S"]) == 5 and int(z["iteration"]) == 8


def test_resume_counts_the_whole_chain(tmp_path):
    out = str(tmp_path / "two")
    # a checkpoint between samples too: the counts file then trails the state
    _execute(_conf(tmp_path, "a", out, samples=6, ckpt=4))
    first = chain_q.load_chain(out, 0)
    project = _execute(_conf(tmp_path, "b", out, samples=6, resume="true"))
    table = chain_q.load_chain(out, 0)
    assert len(set(table["iteration"].to_pylist())) == 12
    assert max(table["iteration"].to_pylist()) > max(first["iteration"].to_pylist())
    assert _read(os.path.join(out, CSV)) == _summarized_csv(project)
    with np.load(os.path.join(out, "pair-counts-rank0.npz")) as z:
        assert int(z["S"]) == 12
        assert int(z["iteration"]) == max(table["iteration"].to_pylist())


def test_stale_or_missing_counts_are_refused(tmp_path):
    out = str(tmp_path / "run")
    _execute(_conf(tmp_path, "a", out, records=60, samples=3))
    path = os.path.join(out, "pair-counts-rank0.npz")
    with np.load(path) as z:
        saved = {k: z[k] for k in z.files}
    again = _conf(tmp_path, "b", out, records=60, samples=2, resume="true")

    os.remove(path)
    with pytest.raises(ValueError, match=r"pair-counts-rank0\.npz"):
        _execute(again)
    # counts that ran ahead of the state
    ahead = dict(saved, iteration=saved["iteration"] + 2)
    np.savez(path, **ahead)
    with pytest.raises(ValueError, match=r"pair-counts-rank0\.npz"):
        _execute(again)
    # counts saved with an earlier state (the chain went on without them)
    behind = dict(saved, state_iteration=saved["state_iteration"] - 2,
                  iteration=saved["iteration"] - 2)
    np.savez(path, **behind)
    with pytest.raises(ValueError, match=r"pair-counts-rank0\.npz"):
        _execute(again)
    # nothing was appended by the refused runs; the right file resumes
    np.savez(path, **saved)
    project = _execute(again)
    assert _read(os.path.join(out, CSV)) == _summarized_csv(project)


WORKER = r"""
import sys
sys.path.insert(0, "__ROOT__")
from dblink_amd.api.cli import main
raise SystemExit(main(["__CONF__"]))
"""


def _run_workers(script, world=2, timeout=600):
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(30500 + os.getpid() % 1000),
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
    table = chain_q.load_chain(out, 0)
    assert sorted(set(table["partitionId"].to_pylist())) == [0, 1, 2, 3]
    want = chain_q.pairwise_link_probabilities(table, device="cpu")
    got = chain_q.read_pairwise_link_probabilities(out)
    assert len(want) > 0 and got.equals(want)
    files = sorted(f for f in os.listdir(out) if f.startswith("pair-counts-rank"))
    assert files == ["pair-counts-rank0.npz", "pair-counts-rank1.npz"]
    # both ranks hold counts, so the merge on rank 0 had something to merge
    sizes = []
    for f in files:
        with np.load(os.path.join(out, f)) as z:
            assert int(z["S"]) == 8
            sizes.append(len(z["keys"]))
    assert min(sizes) > 0


def test_hocon_parameters_and_default_off(tmp_path):
    out = str(tmp_path / "off")
    conf = _conf(tmp_path, "on", out, records=60,
                 extra=ON + ", minLinkProbability : 0.25")
    cfg = hocon.parse_file(conf)
    project = prj.Project(cfg, rank=0, world_size=1)
    step = prj.parse_steps(cfg, project)[0]
    assert step.pairwise_link_probabilities is True
    assert step.min_link_probability == 0.25
    bad = _conf(tmp_path, "bad", out, records=60,
                extra=ON + ", minLinkProbability : 1.5")
    with pytest.raises(ValueError, match="minLinkProbability"):
        prj.parse_steps(hocon.parse_file(bad), project)

    off = _conf(tmp_path, "off", out, records=60, samples=2, extra="")
    cfg = hocon.parse_file(off)
    step = prj.parse_steps(cfg, project)[0]
    assert step.pairwise_link_probabilities is False and step.min_link_probability == 0.0
    project = _execute(off)
    assert sorted(os.listdir(out)) == [
        "diagnostics.csv", "driver-state", "linkage-chain.parquet",
        "partitions-state-rank00000.npz"]

    # sample() with today's positional arguments
    state = project.saved_state()
    before = state.iteration
    sampler_m.sample(project.engine(), state, 2, out, 0, 1, 20, 10,
                     SamplerFlags.for_sampler("PCG-I"), 0, True)
    assert state.iteration == before + 2
    assert not any(f.startswith("pair-counts") or f == CSV for f in os.listdir(out))
