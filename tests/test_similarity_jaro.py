"""Jaro similarity with the Winkler prefix boost: the Python oracle,
``JaroSimilarityFn``, its config name, metric dispatch in ``ops.sim_pairs``
and the native CPU sweep ``jaro_pairs_cpu``.

The CPU sweep forms the score in fp64 in the oracle's order of operations, so
its index is compared with the oracle's exactly (``row_ptr`` and ``col``), at
any threshold; ``expsim`` is stored in fp32 and compared to rel 1e-6.
"""

import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from dblink_amd import ops
from dblink_amd.models.attribute_index import AttributeIndex, _python_sim_pairs
from dblink_amd.models.similarity import (
    JaroSimilarityFn,
    LevenshteinSimilarityFn,
    jaro,
    jaro_parts,
    jaro_winkler,
    similarity_fn_from_config,
)
from dblink_amd.utils import hocon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR, MSIM = 7.3, 10.0


def _gate(a, b):
    """jaro > 0.7 as the integer inequality, from (m, t) and the lengths."""
    m, t = jaro_parts(a, b)
    la, lb = len(a), len(b)
    return 10 * (m * m * (la + lb) + (m - t) * la * lb) > 21 * m * la * lb


# --------------------------------------------------------------------------
# oracle
# --------------------------------------------------------------------------

GOLDEN = [
    # a, b, m, t, jaro, unit at p = 0.1
    ("MARTHA", "MARHTA", 6, 1, 17.0 / 18.0, 0.961111111111111),
    ("DIXON", "DICKSONX", 4, 0, 0.766666666666667, 0.813333333333333),
    ("DWAYNE", "DUANE", 4, 0, 0.822222222222222, 0.84),
    ("JONES", "JOHNSON", 4, 0, 0.790476190476190, 0.832380952380952),
    ("CRATE", "TRACE", 3, 0, 0.733333333333333, 0.733333333333333),  # no common prefix
]


@pytest.mark.parametrize("a,b,m,t,j,u", GOLDEN)
def test_goldens(a, b, m, t, j, u):
    assert jaro_parts(a, b) == (m, t) == jaro_parts(b, a)
    assert jaro(a, b) == pytest.approx(j, abs=1e-12)
    assert jaro_winkler(a, b, 0.1) == pytest.approx(u, abs=1e-12)


def test_empty_and_identical():
    assert jaro("", "") == 1.0 and jaro_winkler("", "", 0.1) == 1.0
    assert jaro("", "abc") == 0.0 and jaro("abc", "") == 0.0
    assert jaro_winkler("", "abc", 0.1) == 0.0
    fn = JaroSimilarityFn(7.0, 10.0, 0.1)
    for x in ("", "a", "ab", "martha", "aaaaaaaa"):
        assert jaro(x, x) == 1.0
        assert fn.similarity(x, x) == pytest.approx(10.0, rel=1e-12)
    assert fn.similarity("", "abc") == 0.0


def test_prefix_scale_zero_is_plain_jaro():
    rng = np.random.default_rng(3)
    fn = JaroSimilarityFn(0.0, 1.0, 0.0)  # sim == unit
    for _ in range(200):
        a = "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(0, 12))))
        b = "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(0, 12))))
        assert jaro_winkler(a, b, 0.0) == jaro(a, b)
        assert fn.similarity(a, b) == pytest.approx(jaro(a, b), abs=1e-15)


def test_prefix_is_capped_at_four():
    # differing only at position 3, 4, 5 or 7 of 10: common prefix 3, 4, 5, 7
    base = "abcdefghij"
    units = []
    for k in (3, 4, 5, 7):
        other = base[:k] + "X" + base[k + 1:]
        assert jaro(base, other) == pytest.approx((0.9 + 0.9 + 1.0) / 3.0, abs=1e-15)
        units.append(jaro_winkler(base, other, 0.1))
    j = jaro(base, base[:3] + "X" + base[4:])
    assert units[0] == pytest.approx(j + 3 * 0.1 * (1.0 - j), abs=1e-15)
    assert units[1] == pytest.approx(j + 4 * 0.1 * (1.0 - j), abs=1e-15)
    assert units[1] == units[2] == units[3] > units[0]


def test_boost_gate():
    # common prefix 1, jaro = (1/6 + 1/6 + 1) / 3 < 0.7: no boost
    assert jaro_parts("abcdef", "auvwxy") == (1, 0)
    assert not _gate("abcdef", "auvwxy")
    assert jaro_winkler("abcdef", "auvwxy", 0.25) == jaro("abcdef", "auvwxy") < 0.7
    # jaro = (11/20 + 11/20 + 1) / 3 is 0.7 exactly, common prefix 4: the
    # integer gate says "not above" whatever the fp64 quotient rounds to
    a = "abcdefghijklmnopqrst"
    b = "abcdefghijk" + "123456789"
    assert jaro_parts(a, b) == (11, 0) and not _gate(a, b)
    assert jaro_winkler(a, b, 0.1) == jaro(a, b) == pytest.approx(0.7, abs=1e-15)
    # one more match, jaro = (12/20 + 12/20 + 1) / 3 = 0.7333: boosted
    b = "abcdefghijkl" + "12345678"
    j = jaro(a, b)
    assert jaro_parts(a, b) == (12, 0) and _gate(a, b) and 0.7 < j < 0.74
    assert jaro_winkler(a, b, 0.1) == pytest.approx(j + 4 * 0.1 * (1.0 - j), abs=1e-15)
    # just above: (23/40 + 23/40 + 1) / 3 = 0.71667
    a = "".join(chr(0x61 + k) for k in range(26)) + "ABCDEFGHIJKLMN"
    b = a[:23] + "0123456789!@#$%^&"
    j = jaro(a, b)
    assert jaro_parts(a, b) == (23, 0) and _gate(a, b) and 0.7 < j < 0.72
    assert jaro_winkler(a, b, 0.1) > j
    # the gate is the integer inequality on random pairs with a shared prefix
    rng = np.random.default_rng(4)
    boosted = plain = 0
    for _ in range(2000):
        a = "a" + "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(1, 10))))
        b = "a" + "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(1, 10))))
        if jaro(a, b) == 1.0:  # the boost l * p * (1 - jaro) is 0
            continue
        got = jaro_winkler(a, b, 0.1) > jaro(a, b)
        assert got == _gate(a, b)
        boosted += got
        plain += not got
    assert boosted > 100 and plain > 100


def test_matching_is_symmetric():
    """Exhaustive over {a, b, c} up to length 5, plus 20k random pairs of up
    to 14 characters over 2..4 letters: (m, t) does not depend on which
    string drives the greedy matching."""
    strings = ["".join(p) for n in range(6) for p in itertools.product("abc", repeat=n)]
    for a, b in itertools.combinations(strings, 2):
        assert jaro_parts(a, b) == jaro_parts(b, a), (a, b)
    rng = np.random.default_rng(5)
    for _ in range(20000):
        k = int(rng.integers(2, 5))
        a = "".join("abcd"[x] for x in rng.integers(k, size=int(rng.integers(0, 15))))
        b = "".join("abcd"[x] for x in rng.integers(k, size=int(rng.integers(0, 15))))
        assert jaro_parts(a, b) == jaro_parts(b, a), (a, b)


def test_window_edge_swaps():
    """With all symbols distinct, swapping two symbols r apart keeps every
    match (at window distance exactly r) and costs one transposition; r + 1
    apart loses both matches. tests/test_gpu_sim_jaro.py builds on this."""
    base = [chr(0x100 + k) for k in range(130)]
    r = 130 // 2 - 1

    def swapped(k, k2):
        out = list(base)
        out[k], out[k2] = out[k2], out[k]
        return "".join(out)

    assert jaro_parts("".join(base), swapped(1, 1 + r)) == (130, 1)
    assert jaro_parts("".join(base), swapped(1, 2 + r)) == (128, 0)
    assert jaro_parts(swapped(1, 1 + r), "".join(base)) == (130, 1)


# --------------------------------------------------------------------------
# config, equality, declared metric
# --------------------------------------------------------------------------

def _parse_fn(name, params):
    cfg = hocon.parse_string(
        'f : { name : "%s", parameters : { %s } }' % (name, params))
    return similarity_fn_from_config(cfg.get_config("f"))


def test_config_parses_and_round_trips():
    fn = _parse_fn("JaroSimilarityFn", "threshold : 6.0, maxSimilarity : 12.0, prefixScale : 0.2")
    assert type(fn) is JaroSimilarityFn
    assert (fn.threshold, fn.max_similarity, fn.prefix_scale) == (6.0, 12.0, 0.2)
    assert fn.mk_string() == "JaroSimilarityFn(threshold=6.0, maxSimilarity=12.0, prefixScale=0.2)"
    default = _parse_fn("JaroSimilarityFn", "threshold : 6.0, maxSimilarity : 12.0")
    assert default.prefix_scale == 0.1
    assert default.mk_string() == \
        "JaroSimilarityFn(threshold=6.0, maxSimilarity=12.0, prefixScale=0.1)"
    assert default == JaroSimilarityFn(6.0, 12.0) and default != fn
    d = JaroSimilarityFn()
    assert (d.threshold, d.max_similarity, d.prefix_scale) == (7.0, 10.0, 0.1)
    for params in ("maxSimilarity : 12.0", "threshold : 6.0"):
        with pytest.raises(Exception):
            _parse_fn("JaroSimilarityFn", params)
    for name in ("JaroWinklerSimilarityFn", "CosineSimilarityFn"):
        with pytest.raises(ValueError, match="unsupported similarity function"):
            _parse_fn(name, "threshold : 6.0, maxSimilarity : 12.0")


def test_validation():
    for bad in ((7.0, 0.0), (10.0, 10.0), (11.0, 10.0), (-1.0, 10.0)):
        with pytest.raises(ValueError):
            JaroSimilarityFn(*bad)
    for bad in (-0.01, 0.26, 1.0):
        with pytest.raises(ValueError, match="prefixScale"):
            JaroSimilarityFn(7.0, 10.0, bad)
    with pytest.raises(ValueError, match="prefixScale"):
        _parse_fn("JaroSimilarityFn", "threshold : 6.0, maxSimilarity : 12.0, prefixScale : 0.3")
    JaroSimilarityFn(0.0, 10.0, 0.0)
    JaroSimilarityFn(7.0, 10.0, 0.25)


def test_equality_hash_and_metric():
    fn = JaroSimilarityFn(7.0, 10.0, 0.1)
    assert fn == JaroSimilarityFn(7.0, 10.0, 0.1)
    assert hash(fn) == hash(JaroSimilarityFn(7.0, 10.0, 0.1))
    assert fn != JaroSimilarityFn(7.0, 10.0, 0.2)
    assert fn != JaroSimilarityFn(6.0, 10.0, 0.1) and fn != JaroSimilarityFn(7.0, 11.0, 0.1)
    lev = LevenshteinSimilarityFn(7.0, 10.0)
    assert fn != lev and lev != fn
    assert len({fn, JaroSimilarityFn(7.0, 10.0, 0.1), JaroSimilarityFn(7.0, 10.0, 0.0), lev}) == 3
    assert fn.native_metric == "jaro" and JaroSimilarityFn.native_metric == "jaro"
    assert not fn.is_constant


# --------------------------------------------------------------------------
# native CPU sweep
# --------------------------------------------------------------------------

def _mutate(rng, s, alphabet, n_edits, max_len):
    """n_edits random edits: substitutions, deletions, insertions and swaps of
    two symbols up to four positions apart."""
    s = list(s)
    for _ in range(n_edits):
        op = int(rng.integers(5))
        k = int(rng.integers(len(s))) if s else 0
        if op >= 3 and len(s) > 1:
            k2 = min(len(s) - 1, k + int(rng.integers(1, 5)))
            s[k], s[k2] = s[k2], s[k]
        elif op == 0 and s:
            s[k] = alphabet[int(rng.integers(len(alphabet)))]
        elif op == 1 and len(s) > 1:
            del s[k]
        elif len(s) < max_len:
            s.insert(k, alphabet[int(rng.integers(len(alphabet)))])
    return s


def _cluster_domain(seed, alphabet, clusters=24, copies=6, max_len=24):
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


def _encode_ord(values, wide):
    """[V, stride] buffer of the characters' own code points, and lengths."""
    import torch

    stride = max(max(map(len, values)), 1)
    buf = np.zeros((len(values), stride), dtype=np.uint16 if wide else np.uint8)
    for i, v in enumerate(values):
        buf[i, : len(v)] = [ord(ch) for ch in v]
    if wide:
        buf = buf.view(np.int16)
    lens = np.array([len(v) for v in values], dtype=np.int32)
    return torch.from_numpy(buf), torch.from_numpy(lens)


ASCII4 = list("abcd")
# 16-bit ids, the upper five above 32768 (negative in int16 storage)
WIDE5 = [chr(c) for c in (300, 7000, 33000, 40000, 50000, 60000, 65535)]


@functools.lru_cache(maxsize=None)
def _domain(kind):
    """About 150 values in mutation clusters, with lengths 0, 1 and 2 and one
    value of 300 symbols with a mutated copy."""
    alphabet = ASCII4 if kind == "ascii" else WIDE5
    values = _cluster_domain(61 if kind == "ascii" else 62, alphabet)
    rng = np.random.default_rng(63)
    long = [alphabet[int(rng.integers(len(alphabet)))] for _ in range(300)]
    values += ["", alphabet[0], alphabet[1], alphabet[0] + alphabet[1], alphabet[1] + alphabet[0],
               "".join(long), "".join(_mutate(rng, long, alphabet, 6, 300))]
    values = sorted(set(values))
    assert 140 <= len(values) <= 160
    assert {0, 1, 2} <= set(map(len, values)) and max(map(len, values)) == 300
    return values


def _assert_index_equal(got_row_ptr, got_col, got_expsim, want):
    np.testing.assert_array_equal(np.asarray(got_row_ptr), want.row_ptr)
    np.testing.assert_array_equal(np.asarray(got_col), want.col)
    assert np.asarray(got_expsim).tolist() == pytest.approx(want.expsim.tolist(), rel=1e-6)


@pytest.mark.parametrize("kind", ["ascii", "wide"])
@pytest.mark.parametrize("prefix_scale", [0.1, 0.0])
def test_cpu_sweep_matches_python_oracle(kind, prefix_scale):
    values = _domain(kind)
    fn = JaroSimilarityFn(THR, MSIM, prefix_scale)
    want = _python_sim_pairs(values, fn)
    assert want.nnz > 4 * len(values)  # many scoring pairs beside the diagonal
    buf, lens = _encode_ord(values, wide=kind == "wide")
    assert buf.dtype.itemsize == (2 if kind == "wide" else 1)
    if kind == "wide":
        assert int(buf.min()) < 0  # ids above 32768
    row_ptr, col, expsim = ops.native().jaro_pairs_cpu(buf, lens, THR, MSIM, prefix_scale)
    _assert_index_equal(row_ptr.numpy(), col.numpy(), expsim.numpy(), want)
    # the 300-symbol value scores against its mutated copy: no length limit
    i = max(range(len(values)), key=lambda k: len(values[k]))
    assert row_ptr[i + 1] - row_ptr[i] >= 2


def test_cpu_sweep_honours_prefix_scale():
    values = _domain("ascii")
    buf, lens = _encode_ord(values, wide=False)
    a = ops.native().jaro_pairs_cpu(buf, lens, THR, MSIM, 0.1)
    b = ops.native().jaro_pairs_cpu(buf, lens, THR, MSIM, 0.0)
    assert a[1].numel() > b[1].numel() + 10  # the boost lifts pairs over the threshold


@functools.lru_cache(maxsize=None)
def _ladder_domain():
    """Three values of every length 1..40 over two letters, and the empty one."""
    rng = np.random.default_rng(64)
    values = {""}
    for n in range(1, 41):
        want = len(values) + (3 if n > 2 else 2)
        while len(values) < want:
            values.add("".join("ab"[k] for k in rng.integers(2, size=n)))
    return sorted(values)


@pytest.mark.parametrize("thr", [0.0, 1.0, 9.0])
@pytest.mark.parametrize("prefix_scale", [0.1, 0.0, 0.25])
def test_length_window_loses_no_pair(thr, prefix_scale):
    values = _ladder_domain()
    assert set(map(len, values)) == set(range(41))
    fn = JaroSimilarityFn(thr, MSIM, prefix_scale)
    want = _python_sim_pairs(values, fn)
    assert want.nnz > (1 if thr == 9.0 else 4) * len(values)
    buf, lens = _encode_ord(values, wide=False)
    row_ptr, col, expsim = ops.native().jaro_pairs_cpu(buf, lens, thr, MSIM, prefix_scale)
    _assert_index_equal(row_ptr.numpy(), col.numpy(), expsim.numpy(), want)


def test_cpu_sweep_rejects_bad_arguments():
    buf, lens = _encode_ord(["ab", "ba"], wide=False)
    with pytest.raises(RuntimeError, match="prefix_scale"):
        ops.native().jaro_pairs_cpu(buf, lens, THR, MSIM, 0.5)
    with pytest.raises(RuntimeError):
        ops.native().jaro_pairs_cpu(buf.to(__import__("torch").int32), lens, THR, MSIM, 0.1)


# --------------------------------------------------------------------------
# dispatch
# --------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["ascii", "wide"])
def test_public_entry_point_takes_the_native_cpu_sweep(kind, monkeypatch):
    values = _domain(kind)
    if kind == "wide":  # more than 255 distinct characters: 16-bit ids
        values = values + ["".join(chr(0x400 + k) for k in range(c, c + 30)) for c in range(0, 300, 30)]
        values = sorted(values)
    called = []
    C = ops.native()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(C, name)
            if name != "jaro_pairs_cpu":
                return fn

            def counted(*args):
                called.append(name)
                return fn(*args)

            return counted

    monkeypatch.setattr(ops, "_C", Spy())
    monkeypatch.setenv("DBLINK_SIM_GPU_MIN_V", "1000000")  # the CPU route, GPU or not
    fn = JaroSimilarityFn(THR, MSIM, 0.15)
    got = ops.sim_pairs(values, fn)
    assert called == ["jaro_pairs_cpu"]
    want = _python_sim_pairs(values, fn)
    _assert_index_equal(got.row_ptr, got.col, got.expsim, want)


def test_attribute_index_builds_from_the_jaro_sweep():
    values = _domain("ascii")
    rng = np.random.default_rng(65)
    weights = {v: float(w) for v, w in zip(values, rng.integers(1, 9, size=len(values)))}
    fn = JaroSimilarityFn(THR, MSIM, 0.1)
    default = AttributeIndex(weights, fn)
    python = AttributeIndex(weights, fn, pair_sweep=_python_sim_pairs)
    assert default.sim_index.nnz == python.sim_index.nnz > 4 * len(values)
    np.testing.assert_allclose(default.sim_norms, python.sim_norms, rtol=1e-6)
    lev = AttributeIndex(weights, LevenshteinSimilarityFn(THR, MSIM))
    assert not np.allclose(default.sim_norms, lev.sim_norms, rtol=1e-6)


# --------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------

def test_example_project_with_jaro_runs_on_cpu_engine(tmp_path):
    from dblink_amd.api.project import Project, parse_steps

    out = tmp_path / "demo"
    subprocess.run(
        [sys.executable, os.path.join(ROOT, "examples", "make_example.py"),
         "--records", "200", "--similarity", "jaro", "--out", str(out),
         "--samples", "10", "--burnin", "10", "--thin", "2"],
        check=True, capture_output=True, timeout=120)
    cfg = hocon.parse_file(str(out / "project.conf"))
    project = Project(cfg, rank=0, world_size=1)
    project.engine_kind = "cpu"
    seen = 0
    for attr in project.matching_attributes:
        if attr.name in ("fname_c1", "lname_c1"):
            assert attr.similarity_fn == JaroSimilarityFn(7.0, 10.0, 0.1)
            seen += 1
    assert seen == 2
    os.makedirs(project.output_path, exist_ok=True)
    with open(os.path.join(project.output_path, "run.txt"), "w") as f:
        f.write(project.mk_string())
    for step in parse_steps(cfg, project):
        step.execute()
    assert "JaroSimilarityFn(threshold=7.0, maxSimilarity=10.0, prefixScale=0.1)" in open(
        os.path.join(project.output_path, "run.txt")).read()
    lines = open(os.path.join(project.output_path, "diagnostics.csv")).read().splitlines()
    assert len(lines) >= 10
    assert os.path.exists(os.path.join(project.output_path, "cluster-size-distribution.csv"))
