"""Samples, oracles and project runs shared by the cluster-count tests
(``test_cluster_counts``, ``test_gpu_cluster_table``).

A sample is ``(rec_ent, rec_gid, iteration)``: record r has the gid
``rec_gid[r]`` and sits in the cluster of entity ``rec_ent[r]``."""

import os

import numpy as np
import pyarrow as pa

from dblink_amd.analysis import chain as chain_q
from dblink_amd.api import project as prj
from dblink_amd.engine.writers import LinkageChainWriter
from dblink_amd.utils import hocon
from dblink_amd.utils.synthdata import write_csv

SMPC = "shared-most-probable-clusters.csv"


def clusters_of(rec_ent, rec_gid):
    """One sample's clusters as lists of gids, in entity order."""
    groups = {}
    for e, g in zip(np.asarray(rec_ent).tolist(), np.asarray(rec_gid).tolist()):
        groups.setdefault(e, []).append(g)
    return [groups[e] for e in sorted(groups)]


def reference_counts(samples):
    """Pure-Python reference -> {frozenset(gids): (count, first iteration)}."""
    out = {}
    for rec_ent, rec_gid, iteration in samples:
        for cluster in clusters_of(rec_ent, rec_gid):
            fs = frozenset(cluster)
            count, first = out.get(fs, (0, iteration))
            out[fs] = (count + 1, min(first, iteration))
    return out


def chain_table(samples, name=str):
    """The linkage-chain table of the samples, rows in iteration order, one
    partition per sample; a record is named ``name(gid)``."""
    rows = {"iteration": [], "partitionId": [], "linkageStructure": []}
    for rec_ent, rec_gid, iteration in sorted(samples, key=lambda s: s[2]):
        rows["iteration"].append(iteration)
        rows["partitionId"].append(0)
        rows["linkageStructure"].append(
            [[name(g) for g in c] for c in clusters_of(rec_ent, rec_gid)])
    return pa.table(rows, schema=LinkageChainWriter.SCHEMA)


def triples(keys, counts, first, offsets, members):
    """A cluster-count tuple -> {frozenset(members): (count, first)}; fails
    when two entries hold the same member set."""
    out = {}
    for i in range(len(keys)):
        fs = frozenset(np.asarray(members)[offsets[i]:offsets[i + 1]].tolist())
        assert len(fs) == offsets[i + 1] - offsets[i] and fs not in out
        out[fs] = (int(counts[i]), int(first[i]))
    return out


def host_counts(samples):
    """The numpy arm over the samples, merged."""
    parts = []
    for rec_ent, rec_gid, iteration in samples:
        order = np.argsort(rec_ent, kind="stable")
        ent = np.asarray(rec_ent)[order]
        offsets = np.r_[np.flatnonzero(np.r_[True, ent[1:] != ent[:-1]]), len(ent)] \
            if len(ent) else np.zeros(1, np.int64)
        parts.append(chain_q.cluster_counts_of_sample(
            np.asarray(rec_gid)[order], offsets, iteration))
    return chain_q.merge_cluster_counts(parts)


def relinked_samples(num_records, num_entities, num_samples, share, seed,
                     first_iteration=1, step=1):
    """Random links, then ``share`` of the records relinked per sample."""
    rng = np.random.default_rng(seed)
    rec_gid = rng.permutation(num_records).astype(np.int64)
    rec_ent = rng.integers(0, num_entities, size=num_records).astype(np.int64)
    samples = []
    for s in range(num_samples):
        if s:
            rec_ent = rec_ent.copy()
            moved = rng.choice(num_records, size=max(1, int(share * num_records)),
                               replace=False)
            rec_ent[moved] = rng.integers(0, num_entities, size=len(moved))
        samples.append((rec_ent, rec_gid, first_iteration + s * step))
    return samples


# ---- project runs --------------------------------------------------------------

CONF = """
dblink : {
  pr : {alpha : 0.5, beta : 50.0}
  data : { path : "%(data)s", recordIdentifier : "rec_id", entityIdentifier : "ent_id",
           nullValue : "NA", matchingAttributes : [
    {name : "by", similarityFunction : {name : "ConstantSimilarityFn"}, distortionPrior : ${dblink.pr}},
    {name : "fname_c1", similarityFunction : {name : "LevenshteinSimilarityFn", parameters : {threshold : 7.0, maxSimilarity : 10.0}}, distortionPrior : ${dblink.pr}},
    {name : "lname_c1", similarityFunction : {name : "LevenshteinSimilarityFn", parameters : {threshold : 7.0, maxSimilarity : 10.0}}, distortionPrior : ${dblink.pr}} ] }
  randomSeed : 7
  engine : "%(engine)s"
  partitioner : {name : "KDTreePartitioner", parameters : {numLevels : %(levels)d, matchingAttributes : [%(split)s]}}
  outputPath : "%(out)s/"
  checkpointPath : "%(out)s/ckpt/"
  steps : [
    {name : "sample", parameters : {sampleSize : %(samples)d, burninInterval : %(burnin)d,
                                     thinningInterval : 2, resume : %(resume)s,
                                     checkpointInterval : %(ckpt)d %(extra)s}}
    %(steps)s
  ]
}
"""

ON = ", sharedMostProbableClusters : true"
NO_CHAIN = ", saveLinkageChain : false"
EVALUATE = ('{name : "evaluate", parameters : {metrics : ["pairwise", "cluster"], '
            'useExistingSMPC : true}}')


def conf(tmp_path, name, out, records=200, **kw):
    data = str(tmp_path / "data.csv")
    if not os.path.exists(data):
        write_csv(data, records, dup_fraction=0.3, seed=3)
    args = dict(data=data, out=out, levels=1, split='"fname_c1"', samples=12,
                burnin=3, resume="false", ckpt=0, extra=ON, engine="cpu", steps="")
    args.update(kw)
    conf = tmp_path / (name + ".conf")
    conf.write_text(CONF % args)
    return str(conf)


def execute(conf):
    cfg = hocon.parse_file(conf)
    project = prj.Project(cfg, rank=0, world_size=1)
    os.makedirs(project.output_path, exist_ok=True)
    for step in prj.parse_steps(cfg, project):
        step.execute()
    return project


def frozen(clusters):
    """A list of clusters -> set of frozensets; fails on a repeated cluster."""
    out = {frozenset(c) for c in clusters}
    assert len(out) == len(clusters)
    return out


def written_smpc(out):
    return frozen(chain_q.read_clusters_csv(os.path.join(out, SMPC)))


def chain_smpc(out):
    """The oracle over the run's saved chain, rows sorted by iteration."""
    table = chain_q.load_chain(out, 0)
    table = table.sort_by([("iteration", "ascending"), ("partitionId", "ascending")])
    return frozen(chain_q.shared_most_probable_clusters(table)), table
