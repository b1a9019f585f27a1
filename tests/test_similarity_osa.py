"""Transposition-aware edit similarity (restricted Damerau-Levenshtein, OSA):
the oracle DP, ``DamerauLevenshteinSimilarityFn``, its config name, metric
dispatch in ``ops.sim_pairs`` and the native CPU sweep's ``transpositions``
flag.

The sweep comparisons use ``(threshold, maxSimilarity) = (5.0, 10.0)``: its
inclusion edge ``3d == la + lb`` has ``unit`` exactly 0.5 in fp32 and fp64
(see the module docstring of ``tests/test_gpu_sim_long.py``), so every
implementation excludes an edge pair identically.
"""

import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from dblink_amd import ops
from dblink_amd.models.attribute_index import AttributeIndex, _python_sim_pairs
from dblink_amd.models.similarity import (
    DamerauLevenshteinSimilarityFn as _damerau,
    LevenshteinSimilarityFn,
    SimilarityFn,
    levenshtein,
    osa_distance as _osa,
    similarity_fn_from_config,
)
from dblink_amd.utils import hocon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, MSIM = 5.0, 10.0


def _swap(s, k):
    return s[:k] + s[k + 1] + s[k] + s[k + 2:]


def _mutate(rng, s, alphabet, n_edits, max_len):
    """n_edits random edits; adjacent swaps are half of them."""
    s = list(s)
    for _ in range(n_edits):
        op = int(rng.integers(6))
        k = int(rng.integers(len(s))) if s else 0
        if op >= 3 and len(s) > 1:
            k = min(k, len(s) - 2)
            s[k], s[k + 1] = s[k + 1], s[k]
        elif op == 0 and s:
            s[k] = alphabet[int(rng.integers(len(alphabet)))]
        elif op == 1 and len(s) > 1:
            del s[k]
        elif len(s) < max_len:
            s.insert(k, alphabet[int(rng.integers(len(alphabet)))])
    return s


def _cluster_domain(seed, alphabet, clusters=20, copies=6, max_len=24):
    """clusters * copies distinct values of length <= max_len: each cluster a
    base and mutated copies of it."""
    rng = np.random.default_rng(seed)
    seen, out = set(), []
    for _ in range(clusters):
        n = int(rng.integers(3, max_len + 1))
        base = [alphabet[int(rng.integers(len(alphabet)))] for _ in range(n)]
        want = len(out) + copies
        cand = base
        while len(out) < want:
            if tuple(cand) not in seen:
                seen.add(tuple(cand))
                out.append("".join(cand))
            cand = _mutate(rng, base, alphabet, int(rng.integers(1, 4)), max_len)
    return out


def _encode(values, stride=None):
    """The [V, stride] symbol buffer and lengths that ops.sim_pairs builds."""
    import torch

    charset = sorted({ch for v in values for ch in v})
    vocab = {ch: i + 1 for i, ch in enumerate(charset)}
    wide = len(charset) > 255
    stride = stride or max(max(map(len, values)), 1)
    buf = np.zeros((len(values), stride), dtype=np.uint16 if wide else np.uint8)
    for i, v in enumerate(values):
        buf[i, : len(v)] = [vocab[ch] for ch in v]
    if wide:
        buf = buf.view(np.int16)
    lens = np.array([len(v) for v in values], dtype=np.int32)
    return torch.from_numpy(buf), torch.from_numpy(lens)


def _rows(row_ptr, col, expsim):
    row_ptr = np.asarray(row_ptr)
    return [dict(zip(col[row_ptr[v]:row_ptr[v + 1]].tolist(),
                     expsim[row_ptr[v]:row_ptr[v + 1]].tolist()))
            for v in range(len(row_ptr) - 1)]


# --------------------------------------------------------------------------
# oracle
# --------------------------------------------------------------------------

def test_osa_goldens():
    assert _osa("ab", "ba") == 1 and levenshtein("ab", "ba") == 2
    assert _osa("abcd", "acbd") == 1
    assert _osa("ca", "abc") == 3  # restricted: unrestricted Damerau gives 2
    assert _osa("", "abc") == 3 and _osa("abc", "") == 3
    assert _osa("", "") == 0
    for x in ("a", "ab", "jonh", "abcabc"):
        assert _osa(x, x) == 0
    assert _osa("jonh", "john") == 1


def test_osa_symmetric_and_bounded_by_levenshtein():
    rng = np.random.default_rng(5)
    alphabet = "abc"
    for _ in range(60):
        a = [alphabet[int(rng.integers(3))] for _ in range(int(rng.integers(0, 12)))]
        b = _mutate(rng, a, alphabet, int(rng.integers(0, 4)), 14)
        a, b = "".join(a), "".join(b)
        d = _osa(a, b)
        assert d == _osa(b, a)
        assert max(len(a), len(b)) >= levenshtein(a, b) >= d >= abs(len(a) - len(b))


def test_osa_equals_levenshtein_without_adjacent_swaps():
    """A transposition needs a[i-1] == b[j-2] and a[i-2] == b[j-1] for some
    i, j: with a over {a, b} and b over {c, d} plus a shared prefix symbol
    that never pairs up crosswise, no such i, j exist."""
    rng = np.random.default_rng(6)
    for _ in range(40):
        a = "x" + "".join("ab"[int(rng.integers(2))] for _ in range(int(rng.integers(0, 9))))
        b = "x" + "".join("cd"[int(rng.integers(2))] for _ in range(int(rng.integers(0, 9))))
        assert _osa(a, b) == levenshtein(a, b)
    # substitutions, deletions and insertions only, far apart
    assert _osa("abcdefgh", "abXdefg") == levenshtein("abcdefgh", "abXdefg") == 2


def test_similarity_value_by_hand():
    # d = 1, |a| + |b| = 8: unit = 1 - 2/9; t = 10/3
    want = (10.0 / 3.0) * (10.0 * (1.0 - 2.0 / 9.0) - 7.0)
    got = _damerau(7.0, 10.0).similarity("jonh", "john")
    assert got == pytest.approx(want, rel=1e-12)
    # Levenshtein: d = 2, unit = 1 - 4/10 = 0.6 < 0.7, truncated to 0
    lev = LevenshteinSimilarityFn(7.0, 10.0).similarity("jonh", "john")
    assert lev == 0.0 and got > lev
    assert _damerau().threshold == 7.0 and _damerau().max_similarity == 10.0


# --------------------------------------------------------------------------
# config, equality, declared metric
# --------------------------------------------------------------------------

def _parse_fn(name, params="threshold : 6.0, maxSimilarity : 12.0"):
    cfg = hocon.parse_string(
        'f : { name : "%s", parameters : { %s } }' % (name, params))
    return similarity_fn_from_config(cfg.get_config("f"))


def test_config_name_parses_and_round_trips():
    fn = _parse_fn("DamerauLevenshteinSimilarityFn")
    assert type(fn).__name__ == "DamerauLevenshteinSimilarityFn"
    assert (fn.threshold, fn.max_similarity) == (6.0, 12.0)
    assert fn.mk_string() == "DamerauLevenshteinSimilarityFn(threshold=6.0, maxSimilarity=12.0)"
    assert fn == _damerau(6.0, 12.0) and hash(fn) == hash(_damerau(6.0, 12.0))
    assert fn != _damerau(6.0, 11.0)
    lev = _parse_fn("LevenshteinSimilarityFn")
    assert fn != lev and lev != fn
    assert lev.mk_string() == "LevenshteinSimilarityFn(threshold=6.0, maxSimilarity=12.0)"
    with pytest.raises(ValueError, match="unsupported similarity function"):
        _parse_fn("JaroWinklerSimilarityFn")


def test_validation_matches_levenshtein():
    for bad in ((7.0, 0.0), (10.0, 10.0), (-1.0, 10.0)):
        with pytest.raises(ValueError):
            _damerau(*bad)
        with pytest.raises(ValueError):
            LevenshteinSimilarityFn(*bad)


def test_native_metric_declared():
    assert SimilarityFn.native_metric is None
    assert LevenshteinSimilarityFn.native_metric == "levenshtein"
    assert _damerau().native_metric == "osa"


# --------------------------------------------------------------------------
# native CPU sweep
# --------------------------------------------------------------------------

ASCII4 = list("abcd")
# more than 255 distinct characters: the 16-bit symbol path
WIDE = [chr(0x400 + k) for k in range(300)]


@functools.lru_cache(maxsize=None)
def _domain(kind):
    if kind == "ascii":
        values = _cluster_domain(41, ASCII4)
    else:
        # 17 clusters over 5 of the characters, so that mutated copies score
        # against each other, and 18 values that between them use all 300:
        # twelve runs of 24 consecutive characters and six swapped copies
        values = _cluster_domain(42, WIDE[:5], clusters=17)
        runs = ["".join(WIDE[k:k + 24]) for k in range(0, 288, 24)] + ["".join(WIDE[276:])]
        values += runs[:12] + [_swap(r, k) for r, k in zip(runs[:5], (0, 5, 11, 17, 22))]
        values.append(_swap(runs[12], 3))
        assert len(set(values)) == len(values) == 120
    osa = _python_sim_pairs(values, _damerau(THR, MSIM))
    lev = _python_sim_pairs(values, LevenshteinSimilarityFn(THR, MSIM))
    return values, osa, lev


def _differing_entries(a, b):
    ra, rb = _rows(a.row_ptr, a.col, a.expsim), _rows(b.row_ptr, b.col, b.expsim)
    return sum(1 for x, y in zip(ra, rb) for k in set(x) | set(y) if x.get(k) != y.get(k))


@pytest.mark.parametrize("kind", ["ascii", "wide"])
def test_cpu_sweep_matches_python_oracle(kind):
    values, osa, lev = _domain(kind)
    assert 110 <= len(values) <= 130 and max(map(len, values)) <= 24
    assert (len({ch for v in values for ch in v}) > 255) == (kind == "wide")
    # the two metrics disagree here: a sweep that ignores the flag cannot pass
    assert _differing_entries(osa, lev) >= 20
    buf, lens = _encode(values)
    assert buf.dtype.itemsize == (2 if kind == "wide" else 1)
    row_ptr, col, expsim = ops.native().sim_pairs_cpu(buf, lens, THR, MSIM, transpositions=True)
    np.testing.assert_array_equal(row_ptr.numpy(), osa.row_ptr)
    np.testing.assert_array_equal(col.numpy(), osa.col)
    assert expsim.numpy().tolist() == pytest.approx(osa.expsim.tolist(), rel=1e-6)
    # and the public entry point sends the new function to that sweep
    idx = ops.sim_pairs(values, _damerau(THR, MSIM))
    np.testing.assert_array_equal(idx.row_ptr, osa.row_ptr)
    np.testing.assert_array_equal(idx.col, osa.col)
    assert idx.expsim.tolist() == pytest.approx(osa.expsim.tolist(), rel=1e-6)


def test_cpu_sweep_long_values_imply_osa_distance():
    """A dozen pairs of 200..300 characters with swaps (and other edits): the
    distance implied by the native expsim is osa_distance."""
    rng = np.random.default_rng(44)
    alphabet = list("abcd")
    values, pairs = [], []
    while len(pairs) < 12:
        n = int(rng.integers(200, 297))
        a = [alphabet[int(rng.integers(4))] for _ in range(n)]
        b = list(a)
        for k in sorted(rng.choice(n - 1, size=int(rng.integers(2, 7)), replace=False)):
            b[k], b[k + 1] = b[k + 1], b[k]
        b = _mutate(rng, b, alphabet, int(rng.integers(0, 4)), 300)
        a, b = "".join(a), "".join(b)
        if a == b or a in values or b in values:
            continue
        pairs.append((len(values), len(values) + 1))
        values += [a, b]
    assert all(200 <= len(v) <= 300 for v in values)
    assert sum(_osa(values[i], values[j]) < levenshtein(values[i], values[j])
               for i, j in pairs) >= 10
    buf, lens = _encode(values)
    row_ptr, col, expsim = ops.native().sim_pairs_cpu(buf, lens, THR, MSIM, True)
    rows = _rows(row_ptr.numpy(), col.numpy(), expsim.numpy())
    scale = MSIM / (MSIM - THR)
    for i, j in pairs:
        assert j in rows[i] and i in rows[j]
        tot = len(values[i]) + len(values[j])
        # expsim = exp(scale * (MSIM * unit - THR)), unit = 1 - 2d / (tot + d)
        unit = (math.log(rows[i][j]) / scale + THR) / MSIM
        d = tot * (1.0 - unit) / (1.0 + unit)
        assert round(d) == _osa(values[i], values[j])
        assert abs(d - round(d)) < 1e-3  # fp32 expsim
        assert rows[j][i] == rows[i][j]


def test_cpu_sweep_default_is_levenshtein():
    values, _, lev = _domain("ascii")
    buf, lens = _encode(values)
    C = ops.native()
    four = C.sim_pairs_cpu(buf, lens, THR, MSIM)
    flag = C.sim_pairs_cpu(buf, lens, THR, MSIM, transpositions=False)
    for x, y in zip(four, flag):
        assert x.dtype == y.dtype and np.array_equal(x.numpy(), y.numpy())
    np.testing.assert_array_equal(four[1].numpy(), lev.col)
    np.testing.assert_array_equal(four[0].numpy(), lev.row_ptr)


# --------------------------------------------------------------------------
# dispatch
# --------------------------------------------------------------------------

class _FirstLetterFn(SimilarityFn):
    """Non-constant, no native metric; carries the attributes a Levenshtein
    sweep would read, so a dispatch that ignores the metric is caught."""

    threshold = 5.0
    max_similarity = 10.0

    def similarity(self, a, b):
        return 2.5 if a[:1] == b[:1] else 0.0

    def mk_string(self):
        return "FirstLetterFn"


def test_function_without_native_metric_takes_python_pass():
    values = ["anna", "anne", "arno", "bob", "bab", "bert", "carl", "cara", "dora", ""]
    fn = _FirstLetterFn()
    assert fn.native_metric is None and not fn.is_constant
    got = ops.sim_pairs(values, fn)
    want = _python_sim_pairs(values, fn)
    np.testing.assert_array_equal(got.row_ptr, want.row_ptr)
    np.testing.assert_array_equal(got.col, want.col)
    np.testing.assert_array_equal(got.expsim, want.expsim)
    assert got.nnz == 3 * 3 + 3 * 3 + 2 * 2 + 1 + 1
    assert set(got.expsim.tolist()) == {math.exp(2.5)}


def test_attribute_index_default_sweep_matches_python_sweep():
    values, _, _ = _domain("ascii")
    rng = np.random.default_rng(45)
    weights = {v: float(w) for v, w in zip(values, rng.integers(1, 9, size=len(values)))}
    fn = _damerau(THR, MSIM)
    default = AttributeIndex(weights, fn)
    python = AttributeIndex(weights, fn, pair_sweep=_python_sim_pairs)
    np.testing.assert_allclose(default.sim_norms, python.sim_norms, rtol=1e-6)
    lev = AttributeIndex(weights, LevenshteinSimilarityFn(THR, MSIM))
    assert not np.allclose(default.sim_norms, lev.sim_norms, rtol=1e-6)


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------

def test_example_project_with_damerau_runs_on_cpu_engine(tmp_path):
    from dblink_amd.api.project import Project, parse_steps

    out = tmp_path / "demo"
    subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "make_example.py"),
         "--records", "200", "--similarity", "damerau", "--out", str(out),
         "--samples", "10", "--burnin", "10", "--thin", "2"],
        check=True, capture_output=True, timeout=120)
    cfg = hocon.parse_file(str(out / "project.conf"))
    project = Project(cfg, rank=0, world_size=1)
    project.engine_kind = "cpu"
    for attr in project.matching_attributes:
        if attr.name in ("fname_c1", "lname_c1"):
            assert attr.similarity_fn == _damerau(7.0, 10.0)
    os.makedirs(project.output_path, exist_ok=True)
    with open(os.path.join(project.output_path, "run.txt"), "w") as f:
        f.write(project.mk_string())
    for step in parse_steps(cfg, project):
        step.execute()
    assert "DamerauLevenshteinSimilarityFn" in open(
        os.path.join(project.output_path, "run.txt")).read()
    lines = open(os.path.join(project.output_path, "diagnostics.csv")).read().splitlines()
    assert len(lines) >= 10
