"""Posterior pairwise link probabilities on the CPU: the numpy arm against
hand-written rows and a pure-Python oracle, chunk merging, the route, the
summarize quantity, and the precision/recall curve of the evaluate step."""

import math
import os
from types import SimpleNamespace

import numpy as np
import pytest

import pair_chain_refs as pcr
from dblink_amd import ops
from dblink_amd.analysis import chain as chain_q
from dblink_amd.analysis import metrics as metrics_m
from dblink_amd.api import project as prj
from dblink_amd.engine.writers import LinkageChainWriter
from dblink_amd.utils import hocon
from dblink_amd.utils.synthdata import write_csv


@pytest.fixture(scope="module")
def random_chain():
    samples = pcr.random_samples()
    return pcr.chain_table(samples), pcr.oracle_counts(samples)


def test_hand_chain_counts_order_and_threshold():
    table = pcr.chain_table(pcr.HAND_SAMPLES)
    result = chain_q.pairwise_link_counts(table, device="cpu")
    uniq_ids, a, b, count, S = result
    assert S == 4
    assert uniq_ids.tolist() == ["10", "9", "B", "a"]  # Python string order
    assert count.dtype == np.int64
    assert (a < b).all()
    assert pcr.rows_of(result) == pcr.HAND_ROWS

    df = chain_q.pairwise_link_probabilities(table, device="cpu")
    assert list(df.columns) == ["recordId1", "recordId2", "probability"]
    assert list(zip(df.recordId1, df.recordId2)) == [r[:2] for r in pcr.HAND_ROWS]
    assert df.probability.tolist() == [c / 4 for _, _, c in pcr.HAND_ROWS]
    assert (df.recordId1 < df.recordId2).all()

    half = chain_q.pairwise_link_probabilities(table, min_probability=0.5, device="cpu")
    assert list(zip(half.recordId1, half.recordId2, half.probability)) == [
        ("10", "9", 1.0), ("B", "a", 0.5)]


def test_hand_chain_through_the_parquet_writer(tmp_path):
    w = LinkageChainWriter(str(tmp_path), buffer_size=2)
    for it, parts in pcr.HAND_SAMPLES:
        w.append(it, parts)
    w.close()
    table = chain_q.load_chain(str(tmp_path), 0)
    assert pcr.rows_of(chain_q.pairwise_link_counts(table, device="cpu")) == pcr.HAND_ROWS
    # the cutoff drops samples, and S with them
    late = chain_q.load_chain(str(tmp_path), 30)
    result = chain_q.pairwise_link_counts(late, device="cpu")
    assert result[4] == 2
    assert pcr.rows_of(result) == [("10", "9", 2), ("10", "a", 1), ("9", "a", 1),
                                   ("B", "a", 1)]


def test_min_link_count_is_an_integer_comparison():
    assert chain_q.min_link_count(0.5, 4) == 2
    assert chain_q.min_link_count(0.0, 4) == 0
    assert chain_q.min_link_count(1.0, 7) == 7
    # 0.1 * 30 is 3.0000000000000004 in floats; one tenth of 30 is 3
    assert chain_q.min_link_count(0.1, 30) == 3
    assert chain_q.min_link_count(0.51, 4) == 3
    with pytest.raises(ValueError):
        chain_q.min_link_count(1.5, 4)


@pytest.mark.parametrize("chunk_pairs", [7, 64, None])
def test_against_itertools_oracle(random_chain, chunk_pairs):
    table, oracle = random_chain
    result = chain_q.pairwise_link_counts(table, device="cpu", chunk_pairs=chunk_pairs)
    assert result[4] == 25
    assert pcr.rows_of(result) == oracle
    assert max(len(c) for _, p in pcr.random_samples() for cs in p.values()
               for c in cs) == 17  # the mix's big cluster is in the chain


def test_chunk_size_invariance_and_lone_big_cluster(random_chain):
    table, _ = random_chain
    whole = chain_q.pairwise_link_counts(table, device="cpu")
    small = chain_q.pairwise_link_counts(table, device="cpu", chunk_pairs=7)
    for x, y in zip(whole[:4], small[:4]):
        assert np.array_equal(x, y)
    # chunks hold at most chunk_pairs pairs; a larger cluster goes alone
    offsets = np.array([0, 2, 19, 21, 24, 24, 25], dtype=np.int64)  # sizes 2 17 2 3 0 1
    pair_ptr = np.r_[0, np.cumsum(chain_q._pairs_per_cluster(offsets))]
    chunks = list(chain_q._pair_chunks(pair_ptr, 64))
    assert chunks == [(0, 1), (1, 2), (2, 6)]
    assert [int(pair_ptr[c1] - pair_ptr[c0]) for c0, c1 in chunks] == [1, 136, 4]
    codes = np.arange(25, dtype=np.int32)
    k64, c64 = chain_q.pair_counts_from_codes(codes, offsets, device="cpu", chunk_pairs=64)
    k, c = chain_q.pair_counts_from_codes(codes, offsets, device="cpu")
    assert np.array_equal(k64, k) and np.array_equal(c64, c)
    assert len(k) == 1 + 136 + 1 + 3 and (c == 1).all()


def test_triangular_decode_is_exact_beyond_fp32():
    # around 2^24 and 2^53-safe large indices, and every index of small rows
    t = np.r_[np.arange(0, 5000), (1 << 24) + np.arange(-3, 4),
              17_997_000 - 1 - np.arange(3), (1 << 40) + np.arange(5)].astype(np.int64)
    i, j = chain_q._tri_decode(t)
    assert ((0 <= i) & (i < j)).all()
    assert (j * (j - 1) // 2 + i == t).all()


def test_duplicate_member_codes_are_no_pair():
    codes = np.array([3, 3, 5, 7, 7], dtype=np.int32)
    offsets = np.array([0, 3, 5], dtype=np.int64)
    k, c = chain_q.pair_counts_from_codes(codes, offsets, device="cpu")
    assert k.tolist() == [(3 << 32) | 5] and c.tolist() == [2]


def test_too_many_ids_is_a_value_error():
    chain_q._check_id_count(2**31 - 1)
    with pytest.raises(ValueError, match="distinct record ids"):
        chain_q._check_id_count(2**31)


def test_route_function(monkeypatch):
    monkeypatch.delenv("DBLINK_PAIRS_GPU_MIN", raising=False)
    big = ops.PAIRS_GPU_MIN_DEFAULT
    assert ops.pair_counts_route(big * 1024, False) == "numpy"
    assert ops.pair_counts_route(0, True) == "numpy"
    monkeypatch.setattr(ops, "have_pair_table", lambda: True)
    assert ops.pair_counts_route(big, True) == "gpu"
    assert ops.pair_counts_route(big - 1, True) == "numpy"
    monkeypatch.setenv("DBLINK_PAIRS_GPU_MIN", "100")
    assert ops.pair_counts_route(100, True) == "gpu"
    assert ops.pair_counts_route(99, True) == "numpy"
    assert ops.pair_counts_route(10**9, False) == "numpy"
    monkeypatch.setattr(ops, "have_pair_table", lambda: False)
    assert ops.pair_counts_route(10**9, True) == "numpy"


CONF = """
dblink : {
  pr : {alpha : 0.5, beta : 50.0}
  data : { path : "%(data)s", recordIdentifier : "rec_id", entityIdentifier : "ent_id",
           nullValue : "NA", matchingAttributes : [
    {name : "by", similarityFunction : {name : "ConstantSimilarityFn"}, distortionPrior : ${dblink.pr}},
    {name : "fname_c1", similarityFunction : {name : "LevenshteinSimilarityFn", parameters : {threshold : 7.0, maxSimilarity : 10.0}}, distortionPrior : ${dblink.pr}},
    {name : "lname_c1", similarityFunction : {name : "LevenshteinSimilarityFn", parameters : {threshold : 7.0, maxSimilarity : 10.0}}, distortionPrior : ${dblink.pr}} ] }
  randomSeed : 7
  engine : "cpu"
  partitioner : {name : "KDTreePartitioner", parameters : {numLevels : 0, matchingAttributes : []}}
  outputPath : "%(out)s/"
  checkpointPath : "%(out)s/ckpt/"
  steps : [
    {name : "sample", parameters : {sampleSize : 6, burninInterval : 2, resume : false, checkpointInterval : 0}},
    {name : "summarize", parameters : {quantities : [%(quantities)s] %(extra)s}},
    {name : "evaluate", parameters : {metrics : [%(metrics)s]}}
  ]
}
"""


def _run(tmp_path, name, quantities, extra="", metrics='"pairwise"'):
    data = str(tmp_path / "data.csv")
    if not os.path.exists(data):
        write_csv(data, 60, dup_fraction=0.3, seed=3)
    out = str(tmp_path / name)
    conf = tmp_path / (name + ".conf")
    conf.write_text(CONF % dict(data=data, out=out, quantities=quantities,
                                extra=extra, metrics=metrics))
    cfg = hocon.parse_file(str(conf))
    project = prj.Project(cfg, rank=0, world_size=1)
    os.makedirs(project.output_path, exist_ok=True)
    for step in prj.parse_steps(cfg, project):
        step.execute()
    return out, str(conf)


def test_summarize_and_evaluate_steps_end_to_end(tmp_path, capsys):
    q = '"pairwise-link-probabilities"'
    out, _ = _run(tmp_path, "all", q, metrics='"pairwise", "pairwise-curve"')
    path = os.path.join(out, "pairwise-link-probabilities.csv")
    with open(path) as f:
        assert f.readline() == "recordId1,recordId2,probability\n"
    table = chain_q.load_chain(out, 0)
    want = chain_q.pairwise_link_probabilities(table)
    got = chain_q.read_pairwise_link_probabilities(path)
    assert len(want) > 0
    assert got.recordId1.tolist() == want.recordId1.tolist()
    assert got.recordId2.tolist() == want.recordId2.tolist()
    assert got.probability.tolist() == want.probability.tolist()  # repr-exact
    assert got.equals(chain_q.read_pairwise_link_probabilities(out))

    # the evaluate step wrote the curve and one line after the sMPC metrics
    with open(os.path.join(out, "pairwise-link-curve.csv")) as f:
        lines = f.read().splitlines()
    assert lines[0] == "threshold,predictedLinks,trueLinks,precision,recall,f1"
    assert len(lines) == 20
    with open(os.path.join(out, "evaluation-results.txt")) as f:
        text = f.read()
    base, _ = _run(tmp_path, "base", '"partition-sizes"')
    with open(os.path.join(base, "evaluation-results.txt")) as f:
        base_text = f.read()
    assert text.startswith(base_text)  # same chain (same seed): lines unchanged
    tail = text[len(base_text):].splitlines()
    assert len(tail) == 1 and tail[0].startswith("Pairwise link curve: ")
    # a config without the quantity / metric writes neither file
    assert not os.path.exists(os.path.join(base, "pairwise-link-probabilities.csv"))
    assert not os.path.exists(os.path.join(base, "pairwise-link-curve.csv"))

    # minLinkProbability keeps exactly the filtered rows
    half, _ = _run(tmp_path, "half", q, extra=", minLinkProbability : 0.5")
    got = chain_q.read_pairwise_link_probabilities(half)
    table = chain_q.load_chain(half, 0)
    full = chain_q.pairwise_link_probabilities(table)
    want = full[full.probability >= 0.5].reset_index(drop=True)
    assert len(want) > 0
    assert got.equals(want)
    assert got.equals(chain_q.pairwise_link_probabilities(table, min_probability=0.5))

    # --check rejects a probability outside [0, 1]
    bad = tmp_path / "bad.conf"
    bad.write_text(CONF % dict(data=str(tmp_path / "data.csv"), out=str(tmp_path / "bad"),
                               quantities=q, extra=", minLinkProbability : 1.5",
                               metrics='"pairwise"'))
    capsys.readouterr()
    assert prj.check_config(str(bad)) == 1
    assert "minLinkProbability" in capsys.readouterr().out
    ok = tmp_path / "ok.conf"
    ok.write_text(bad.read_text().replace("1.5", "0.01"))
    assert prj.check_config(str(ok)) == 0


# the hand chain with ("10", "9") apart in the last sample: its count is 3
CURVE_SAMPLES = pcr.HAND_SAMPLES[:3] + [(40, {0: [["B", "a"], []], 1: [["9"], ["10"]]})]
CURVE_TRUTH = [{"10", "9", "a"}, {"B"}]  # 3 true pairs


def test_curve_on_hand_chain(tmp_path):
    w = LinkageChainWriter(str(tmp_path))
    for it, parts in CURVE_SAMPLES:
        w.append(it, parts)
    w.close()
    stub = SimpleNamespace(ent_id_attribute="ent_id", rank=0, output_path=str(tmp_path),
                           true_clusters=lambda: CURVE_TRUTH)
    prj.EvaluateStep(stub, metrics=["pairwise-curve"]).execute()
    with open(os.path.join(str(tmp_path), "pairwise-link-curve.csv")) as f:
        lines = f.read().splitlines()
    assert lines[0] == "threshold,predictedLinks,trueLinks,precision,recall,f1"
    rows = [ln.split(",") for ln in lines[1:]]
    assert [float(r[0]) for r in rows] == [k / 20 for k in range(1, 20)]
    by_t = {float(r[0]): r for r in rows}
    # counts: (10,9) 3, (B,a) 2, (10,a) 1, (9,a) 1; S = 4
    # t = 0.25 keeps count >= 1: all four pairs, three of them true
    assert by_t[0.25][1:3] == ["4", "3"]
    assert float(by_t[0.25][3]) == 0.75 and float(by_t[0.25][4]) == 1.0
    # t = 0.5 keeps count >= 2: (10,9) true, (B,a) false
    assert by_t[0.5][1:3] == ["2", "1"]
    assert float(by_t[0.5][3]) == 0.5 and float(by_t[0.5][4]) == 1 / 3
    assert float(by_t[0.5][5]) == pytest.approx(0.4)
    # t = 0.95 needs count >= 4: nothing predicted -> precision and F1 are
    # NaN (as metrics.precision / f_measure), recall is 0
    assert by_t[0.95][1:3] == ["0", "0"]
    assert math.isnan(float(by_t[0.95][3])) and math.isnan(float(by_t[0.95][5]))
    assert float(by_t[0.95][4]) == 0.0

    rows = metrics_m.pairwise_link_curve(
        *chain_q.pairwise_link_counts(pcr.chain_table(CURVE_SAMPLES), device="cpu"),
        CURVE_TRUTH)
    best = metrics_m.best_f1_row(rows)
    # count >= 1 (t <= 0.25): P 0.75, R 1 -> F1 6/7, the best; lowest t wins ties
    assert best["threshold"] == 0.05 and best["f1"] == pytest.approx(6 / 7)
    with open(os.path.join(str(tmp_path), "evaluation-results.txt")) as f:
        assert f.read() == metrics_m.curve_summary_line(rows) + "\n"
    # ids the truth does not know are never true links
    rows = metrics_m.pairwise_link_curve(
        *chain_q.pairwise_link_counts(pcr.chain_table(CURVE_SAMPLES), device="cpu"),
        [{"10", "9"}])
    assert [r["trueLinks"] for r in rows][:5] == [1] * 5
