"""GPU Jaro sweep with the Winkler prefix boost: ``jaro_pairs_gpu`` for
W = 1..4 pattern words and both symbol types.

The reference for long values is the native CPU sweep ``jaro_pairs_cpu``,
which ``tests/test_similarity_jaro.py`` holds to the pure-Python oracle; the
short domain is compared with that oracle directly. Rows are compared as sets
(the fill order is atomic), ``expsim`` to rel 1e-5 (fp32 ``__expf`` over an
argument formed in fp64).

All cases use ``(threshold, maxSimilarity) = (7.3, 10.0)``. Every test first
shows on the CPU reference that no pair scores within 1e-4 of the inclusion
edge ``unit == 0.73``: the CPU index is the same at thresholds 7.299 and
7.301. A pair of identical values has unit 1.
"""

import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)

THR, MSIM, P = 7.3, 10.0, 0.1
EDGE = 1e-4
ADJACENT = ((62, 63), (63, 64), (64, 65), (127, 128), (191, 192))
# 130 and 132 put the match window r at 64 and 65, beside 128/129 at 63
LENGTHS = {0, 1, 2, 63, 64, 65, 127, 128, 129, 130, 132, 192, 193, 255, 256}


def _swapped(seq, k, k2):
    out = list(seq)
    out[k], out[k2] = out[k2], out[k]
    return out


def _boundary_domain(seed, fresh, run_sym):
    """Symbol sequences around the 64/128/192 word boundaries.

    Lengths LENGTHS. The chain 256 > 193 > 132 > 130 > 129 > 65 is made of
    nested subsequences (pairs score across length classes); 255, 192, 128, 64
    and 127, 63 are neighbours with the third symbol deleted, which shifts
    every later word. Each long value s (window r = len(s) // 2 - 1 against a
    copy of itself) has

    - one copy per pair of ADJACENT it is long enough for: swaps on and beside
      the word boundaries of the pattern;
    - copies with the symbols at k and k + r swapped, and at k and k + r + 1:
      the first pair still matches, at window distance exactly r, the second
      lies one position outside
      (``tests/test_similarity_jaro.py::test_window_edge_swaps``). k is 1, 40
      and 70, so the far position falls into the same word as k, the next or
      the one after. r takes 31, 62, 63, 64, 65, 95, 126 and 127 (it cannot
      exceed 127 at 256 symbols), so it crosses 64, and windows [j-r, j+r]
      of one, two, three and four words occur, crossing bits 64, 128 and 192.

    Two single-symbol runs (129, 256) and a run with one foreign symbol give
    every window many candidate bits. ``fresh(avoid)`` draws a symbol
    different from ``avoid``.
    """
    rng = np.random.default_rng(seed)

    def drop(seq, n):
        keep = np.sort(rng.choice(len(seq), len(seq) - n, replace=False))
        return [seq[k] for k in keep]

    def delete_front(seq):
        return seq[:2] + seq[3:]

    b256 = []
    for _ in range(256):
        b256.append(fresh(b256[-1] if b256 else None))
    b193 = drop(b256, 63)
    b132 = drop(b193, 61)
    b130 = drop(b132, 2)
    b129 = drop(b130, 1)
    b65 = drop(b129, 64)
    b255, b192, b128, b64 = map(delete_front, (b256, b193, b129, b65))
    b127, b63 = delete_front(b128), delete_front(b64)
    longs = [b256, b255, b193, b192, b132, b130, b129, b128, b127, b65]
    seqs = longs + [b64, b63, b256[5:7], [b256[5]], []]
    n_base = len(seqs)
    for s in longs:
        seqs += [_swapped(s, k, k1) for k, k1 in ADJACENT if k1 < len(s) and s[k] != s[k1]]
        r = len(s) // 2 - 1
        for k in (1, 40, 70):
            for dist in (r, r + 1):
                if k + dist < len(s) and s[k] != s[k + dist]:
                    seqs.append(_swapped(s, k, k + dist))
    n_swapped = len(seqs) - n_base
    seqs += [[run_sym] * 129, [run_sym] * 256,
             [run_sym] * 100 + [b256[0] if b256[0] != run_sym else b256[1]] + [run_sym] * 91]
    seqs = list({tuple(s): s for s in seqs}.values())
    assert {len(s) for s in seqs} == LENGTHS
    return seqs, n_swapped


def _prefix_family(base, fresh):
    """Copies of ``base`` that differ from it in one symbol, at position 0, 1,
    3, 4 or 6: common prefixes of 0, 1, 3, 4 and 6 symbols with the base."""
    out = [list(base)]
    for k in (0, 1, 3, 4, 6):
        s = list(base)
        s[k] = fresh(s[k])
        out.append(s)
    return out


def _pack(seqs, stride, dtype):
    """[V, stride] symbol buffer (0-padded) and int32 lengths, on the host."""
    buf = np.zeros((len(seqs), stride), dtype=dtype)
    for i, s in enumerate(seqs):
        buf[i, : len(s)] = s
    if dtype == np.uint16:
        buf = buf.view(np.int16)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    return torch.from_numpy(buf), torch.from_numpy(lens)


def _rows(row_ptr, col, expsim):
    row_ptr, col, expsim = (np.asarray(x.cpu()) for x in (row_ptr, col, expsim))
    return [dict(zip(col[row_ptr[v]:row_ptr[v + 1]].tolist(),
                     expsim[row_ptr[v]:row_ptr[v + 1]].tolist()))
            for v in range(len(row_ptr) - 1)]


def _gpu_rows(buf, lens, p=P):
    return _rows(*C.jaro_pairs_gpu(buf.to(DEV), lens.to(DEV), THR, MSIM, p))


def _cpu_rows(buf, lens, p=P):
    """CPU-sweep rows, after showing that no pair lies within EDGE of the
    inclusion edge (module docstring)."""
    below = C.jaro_pairs_cpu(buf, lens, THR - EDGE * MSIM, MSIM, p)
    above = C.jaro_pairs_cpu(buf, lens, THR + EDGE * MSIM, MSIM, p)
    assert torch.equal(below[0], above[0]) and torch.equal(below[1], above[1]), \
        "a pair scores within 1e-4 of the inclusion edge: change the seed"
    at = C.jaro_pairs_cpu(buf, lens, THR, MSIM, p)
    assert torch.equal(at[0], above[0]) and torch.equal(at[1], above[1])
    return _rows(*at)


def _assert_rows_match(got, want):
    assert len(got) == len(want)
    for v, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), f"row {v}: column sets differ"
        for k in w:
            assert g[k] == pytest.approx(w[k], rel=1e-5), f"row {v} col {k}"


def _differing_entries(a, b):
    return sum(1 for x, y in zip(a, b) for k in set(x) | set(y) if x.get(k) != y.get(k))


@functools.lru_cache(maxsize=None)
def _ascii_case():
    """(strings, buffer, lengths) of the uint8 boundary domain."""
    rng = np.random.default_rng(71)
    letters = "abcd"

    def fresh(avoid):
        while True:
            ch = letters[rng.integers(4)]
            if ch != avoid:
                return ch

    seqs, n_swapped = _boundary_domain(72, fresh, "a")
    assert n_swapped >= 40, n_swapped
    seqs += _prefix_family(seqs[0][:20], fresh) + _prefix_family(seqs[0][30:39], fresh)
    seqs = list({tuple(s): s for s in seqs}.values())
    values = ["".join(s) for s in seqs]
    buf, lens = _pack([list(v.encode()) for v in values], 256, np.uint8)
    return values, buf, lens


@functools.lru_cache(maxsize=None)
def _wide_case():
    """The same construction over 16-bit ids drawn without replacement from
    all of 1..65535: most exceed 8 bits, about half have bit 15 set."""
    rng = np.random.default_rng(73)
    pool = iter(rng.permutation(np.arange(1, 65536)).tolist())
    fresh = lambda avoid: next(pool)  # noqa: E731
    seqs, n_swapped = _boundary_domain(74, fresh, next(pool))
    assert n_swapped >= 70, n_swapped  # every swap applies: all symbols are distinct
    seqs += _prefix_family(seqs[0][:20], fresh) + _prefix_family(seqs[0][30:39], fresh)
    ids = {x for s in seqs for x in s}
    assert len(ids) > 250 and max(ids) > 32768 and sum(x > 255 for x in ids) > 200
    buf, lens = _pack(seqs, 256, np.uint16)
    assert buf.dtype == torch.int16
    return seqs, buf, lens


@functools.lru_cache(maxsize=None)
def _reference(case, p):
    _, buf, lens = _ascii_case() if case == "ascii" else _wide_case()
    want = _cpu_rows(buf, lens, p)
    assert sum(len(w) for w in want) > 4 * len(want)  # many scoring pairs
    return want


@gpu
@pytest.mark.parametrize("case", ["ascii", "wide"])
def test_word_boundaries_match_cpu_sweep(case):
    _, buf, lens = _ascii_case() if case == "ascii" else _wide_case()
    want = _reference(case, P)
    got = _gpu_rows(buf, lens, P)
    _assert_rows_match(got, want)


@gpu
@pytest.mark.parametrize("case", ["ascii", "wide"])
def test_prefix_scale_is_honoured(case):
    _, buf, lens = _ascii_case() if case == "ascii" else _wide_case()
    boosted, plain = _reference(case, P), _reference(case, 0.0)
    assert _differing_entries(boosted, plain) >= 10
    got_boosted, got_plain = _gpu_rows(buf, lens, P), _gpu_rows(buf, lens, 0.0)
    _assert_rows_match(got_boosted, boosted)
    _assert_rows_match(got_plain, plain)
    assert _differing_entries(got_boosted, got_plain) >= 10


@gpu
def test_prefix_lengths_score_as_on_the_cpu():
    """Common prefixes of 0, 1, 3, 4 and 6 symbols: five distinct boosts, the
    last two equal (cap at 4), on the GPU as in the reference."""
    seqs, buf, lens = _wide_case()
    want, got = _reference("wide", P), _gpu_rows(buf, lens, P)
    index = {tuple(s): v for v, s in enumerate(seqs)}
    for lo, hi in ((0, 20), (30, 39)):
        base = seqs[0][lo:hi]
        b = index[tuple(base)]
        variants = [v for v, s in enumerate(seqs)
                    if len(s) == len(base) and sum(x != y for x, y in zip(s, base)) == 1]
        by_prefix = {}
        for v in variants:
            k = next(k for k in range(len(base)) if seqs[v][k] != base[k])
            by_prefix[k] = v
        assert sorted(by_prefix) == [0, 1, 3, 4, 6]
        sims = [got[b][by_prefix[k]] for k in (0, 1, 3, 4, 6)]
        assert sims[0] < sims[1] < sims[2] < sims[3] and sims[3] == sims[4]
        for k, s in zip((0, 1, 3, 4, 6), sims):
            assert s == pytest.approx(want[b][by_prefix[k]], rel=1e-5)


RANDOM_SEED = 75
# (two of the four letters, base lengths) of each group of five clusters
RANDOM_GROUPS = (
    ((1, 2), (1, 2, 2, 3, 3)),
    ((3, 4), (8, 9, 9, 10, 10)),
    ((1, 3), (30, 32, 33, 35, 36)),
    ((2, 4), (63, 64, 65, 66, 70)),
    ((1, 4), (127, 128, 129, 130, 140)),
    ((2, 3), (192, 193, 230, 255, 256)),
)


def _random_domain(seed):
    """V = 300 in 30 clusters of mutated copies, lengths 1..256, 4 letters.

    Unrelated random strings over four letters score all over 0.6..0.9
    (the match window is wide), so among the 90000 pairs of 30 such clusters
    dozens land within 1e-4 of the inclusion edge whatever the seed. The
    clusters are therefore laid out so that unrelated pairs stay clear of it:
    each cluster draws a balanced base from two of the four letters, and the
    five clusters that share a letter pair have lengths within a quarter of
    each other (jaro about 0.9, with many transpositions), while clusters of
    different groups share at most one letter (m about half the shorter
    value, t = 0: jaro below 0.7) and differ in length by 2x or more.
    """
    rng = np.random.default_rng(seed)
    seqs = []
    for letters, base_lens in RANDOM_GROUPS:
        for n in base_lens:
            base = [letters[k % 2] for k in rng.permutation(n)]
            seqs.append(base)
            for _ in range(9):
                s = list(base)
                for _ in range(int(rng.integers(0, 1 + max(1, n // 8)))):
                    op, k = rng.integers(5), int(rng.integers(len(s)))
                    if op >= 3 and len(s) > 1:
                        k2 = int(rng.integers(len(s)))
                        s[k], s[k2] = s[k2], s[k]
                    elif op == 0:
                        s[k] = letters[int(rng.integers(2))]
                    elif op == 1 and len(s) > 1:
                        del s[k]
                    elif len(s) < 256:
                        s.insert(k, letters[int(rng.integers(2))])
                seqs.append(s)
    assert len(seqs) == 300 and all(1 <= len(s) <= 256 for s in seqs)
    assert {x for s in seqs for x in s} == {1, 2, 3, 4}
    return seqs


@gpu
def test_randomized_lengths_match_cpu_sweep():
    seqs = _random_domain(RANDOM_SEED)
    buf, lens = _pack(seqs, 256, np.uint8)
    want = _cpu_rows(buf, lens)
    assert sum(len(w) for w in want) > 10 * len(seqs)
    _assert_rows_match(_gpu_rows(buf, lens), want)


@gpu
def test_short_domain_matches_python_oracle():
    """60 values of at most 16 characters, straight against the oracle."""
    from dblink_amd.models.attribute_index import _python_sim_pairs
    from dblink_amd.models.similarity import JaroSimilarityFn, jaro_winkler

    rng = np.random.default_rng(76)
    values = set()
    while len(values) < 60:
        base = "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(1, 15))))
        values.add(base)
        for _ in range(5):
            s = list(base)
            for _ in range(int(rng.integers(1, 4))):
                op, k = int(rng.integers(5)), int(rng.integers(len(s)))
                if op >= 3 and len(s) > 1:
                    k2 = int(rng.integers(len(s)))
                    s[k], s[k2] = s[k2], s[k]
                elif op == 0:
                    s[k] = "abc"[rng.integers(3)]
                elif op == 1 and len(s) > 1:
                    del s[k]
                elif len(s) < 16:
                    s.insert(k, "abc"[rng.integers(3)])
            values.add("".join(s))
    values = sorted(values)[:59] + [""]
    assert max(map(len, values)) <= 16
    for a in values:
        for b in values:
            assert a == b or abs(jaro_winkler(a, b, P) - THR / MSIM) >= EDGE, (a, b)
    ref = _python_sim_pairs(values, JaroSimilarityFn(THR, MSIM, P))
    want = [dict(zip(ref.col[ref.row_ptr[v]:ref.row_ptr[v + 1]].tolist(),
                     ref.expsim[ref.row_ptr[v]:ref.row_ptr[v + 1]].tolist()))
            for v in range(len(values))]
    assert sum(len(w) for w in want) > 4 * len(values)
    buf, lens = _pack([list(v.encode()) for v in values], 64, np.uint8)
    _assert_rows_match(_gpu_rows(buf, lens), want)


@gpu
def test_public_route_sends_jaro_to_the_gpu(monkeypatch):
    from dblink_amd.models.similarity import JaroSimilarityFn

    values, buf, lens = _ascii_case()
    _reference("ascii", P)  # the inclusion-edge condition
    monkeypatch.setenv("DBLINK_SIM_GPU_MIN_V", "0")
    charset = {ch for v in values for ch in v}
    assert ops.sim_pairs_route(len(values), max(map(len, values)), len(charset),
                               torch.cuda.is_available()) == "gpu"
    idx = ops.sim_pairs(values, JaroSimilarityFn(THR, MSIM, P))
    row_ptr, col, expsim = C.jaro_pairs_cpu(buf, lens, THR, MSIM, P)
    assert col.numel() > 4 * len(values)
    np.testing.assert_array_equal(idx.row_ptr, row_ptr.numpy())
    np.testing.assert_array_equal(idx.col, col.numpy())  # rows sorted by column
    np.testing.assert_allclose(idx.expsim, expsim.numpy(), rtol=1e-5)


@gpu
def test_gpu_sweep_rejects_bad_arguments():
    _, buf, lens = _ascii_case()
    with pytest.raises(RuntimeError, match="prefix_scale"):
        C.jaro_pairs_gpu(buf.to(DEV), lens.to(DEV), THR, MSIM, 0.3)
    long = torch.zeros((2, 320), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="limit of 256"):
        C.jaro_pairs_gpu(long, torch.tensor([300, 2], dtype=torch.int32, device=DEV),
                         THR, MSIM, P)
