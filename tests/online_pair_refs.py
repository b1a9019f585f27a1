"""Project runs shared by the online pair-count tests
(``test_online_pair_counts``, ``test_gpu_pair_links``): a config with
``pairwiseLinkProbabilities`` on, and the CSV a summarize step derives from
the same run's saved chain."""

import os

from dblink_amd.analysis import chain as chain_q
from dblink_amd.api import project as prj
from dblink_amd.utils import hocon
from dblink_amd.utils.synthdata import write_csv

CSV = chain_q.PAIR_PROB_FILE

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
  ]
}
"""

ON = ", pairwiseLinkProbabilities : true"


def conf(tmp_path, name, out, records=200, **kw):
    data = str(tmp_path / "data.csv")
    if not os.path.exists(data):
        write_csv(data, records, dup_fraction=0.3, seed=3)
    args = dict(data=data, out=out, levels=1, split='"fname_c1"', samples=12,
                burnin=3, resume="false", ckpt=0, extra=ON, engine="cpu")
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


def read(path):
    with open(path, "rb") as f:
        return f.read()


def summarized_csv(project, min_probability=0.0):
    """Bytes of the CSV a SummarizeStep writes from the saved chain; the
    online file is put back afterwards."""
    path = os.path.join(project.output_path, CSV)
    online = read(path)
    prj.SummarizeStep(project, quantities=["pairwise-link-probabilities"],
                      min_link_probability=min_probability).execute()
    offline = read(path)
    with open(path, "wb") as f:
        f.write(online)
    return offline
