"""GPU similarity sweep with transpositions (restricted Damerau-Levenshtein,
OSA): ``sim_pairs_gpu(..., transpositions=True)`` for W = 1..4 Myers words
and both symbol types.

The reference for long values is the native CPU sweep with
``transpositions=True``, which ``tests/test_similarity_osa.py`` holds to the
pure-Python oracle; the short domain is compared with that oracle directly.
All cases use ``(threshold, maxSimilarity) = (5.0, 10.0)``, whose inclusion
edge ``3d == la + lb`` is exact in fp32 and fp64 (see the module docstring of
``tests/test_gpu_sim_long.py``). Rows are compared as sets (the fill order is
atomic), ``expsim`` to rel 1e-5 (fp32 ``__expf``).
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

THR, MSIM = 5.0, 10.0
SWAPS = ((62, 63), (63, 64), (64, 65), (127, 128), (191, 192))
LENGTHS = {0, 1, 2, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256}


def _fn():
    from dblink_amd.models.similarity import DamerauLevenshteinSimilarityFn

    return DamerauLevenshteinSimilarityFn(THR, MSIM)


def _swapped(seq, k):
    out = list(seq)
    out[k], out[k + 1] = out[k + 1], out[k]
    return out


def _boundary_domain(seed, fresh, run_sym):
    """Symbol sequences around the 64/128/192 word boundaries, with swaps.

    Lengths LENGTHS. The chain 256 > 193 > 129 > 65 is made of nested
    subsequences (so pairs score across word classes); 255, 192, 128, 64 and
    127, 63 are their neighbours with the third symbol deleted, which shifts
    every later word. Each of the eight long values has one copy per pair of
    SWAPS that it is long enough for and whose two symbols differ: (63, 64),
    (127, 128) and (191, 192) straddle a word boundary of the pattern, the
    others sit on either side of one. One more copy swaps the pair directly
    after a deletion, and two single-symbol runs (129, 256) are values in
    which a swap changes nothing. ``fresh(avoid)`` draws a symbol different
    from ``avoid``.
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
    b129 = drop(b193, 64)
    b65 = drop(b129, 64)
    b255, b192, b128, b64 = map(delete_front, (b256, b193, b129, b65))
    b127, b63 = delete_front(b128), delete_front(b64)
    longs = [b256, b255, b193, b192, b129, b128, b127, b65]
    seqs = longs + [b64, b63, b256[5:7], [b256[5]], []]
    n_base = len(seqs)
    for s in longs:
        seqs += [_swapped(s, k) for k, k1 in SWAPS if k1 < len(s) and s[k] != s[k1]]
    n_swapped = len(seqs) - n_base
    cut = b256[:100] + b256[101:]
    k = next(k for k in range(100, 120) if cut[k] != cut[k + 1])
    seqs.append(_swapped(cut, k))
    seqs += [[run_sym] * 129, [run_sym] * 256]
    assert len({tuple(s) for s in seqs}) == len(seqs)
    assert {len(s) for s in seqs} == LENGTHS
    return seqs, n_swapped


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


def _gpu_rows(buf, lens, *flag):
    return _rows(*C.sim_pairs_gpu(buf.to(DEV), lens.to(DEV), THR, MSIM, *flag))


def _cpu_rows(buf, lens):
    return _rows(*C.sim_pairs_cpu(buf, lens, THR, MSIM, True))


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
    """(strings, buffer, lengths, CPU-sweep rows) of the uint8 boundary domain."""
    rng = np.random.default_rng(51)
    letters = "abcd"

    def fresh(avoid):
        while True:
            ch = letters[rng.integers(4)]
            if ch != avoid:
                return ch

    seqs, n_swapped = _boundary_domain(52, fresh, "a")
    assert n_swapped >= 20, n_swapped
    values = ["".join(s) for s in seqs]
    buf, lens = _pack([list(v.encode()) for v in values], 256, np.uint8)
    return values, buf, lens, _cpu_rows(buf, lens)


@functools.lru_cache(maxsize=None)
def _wide_case():
    """The same construction over 16-bit ids drawn without replacement from
    all of 1..65535: most exceed 8 bits, about half have bit 15 set."""
    rng = np.random.default_rng(53)
    pool = iter(rng.permutation(np.arange(1, 65536)).tolist())
    seqs, n_swapped = _boundary_domain(54, lambda avoid: next(pool), next(pool))
    assert n_swapped == 31  # every swap applies: all symbols are distinct
    ids = {x for s in seqs for x in s}
    assert len(ids) > 250 and max(ids) > 32768 and sum(x > 255 for x in ids) > 200
    buf, lens = _pack(seqs, 256, np.uint16)
    assert buf.dtype == torch.int16
    return buf, lens, _cpu_rows(buf, lens)


@gpu
def test_word_boundaries_uint8_match_cpu_sweep():
    values, buf, lens, want = _ascii_case()
    assert sum(len(w) for w in want) > 4 * len(values)  # many scoring pairs
    got = _gpu_rows(buf, lens, True)
    _assert_rows_match(got, want)
    # the flag is honoured: Levenshtein on the same buffers differs
    assert _differing_entries(got, _gpu_rows(buf, lens, False)) >= 10


@gpu
def test_word_boundaries_16bit_symbols_match_cpu_sweep():
    buf, lens, want = _wide_case()
    got = _gpu_rows(buf, lens, True)
    _assert_rows_match(got, want)
    assert _differing_entries(got, _gpu_rows(buf, lens, False)) >= 10


@gpu
def test_randomized_lengths_match_cpu_sweep():
    """V = 300 in 30 clusters of mutated copies, lengths 1..256, 4 letters,
    a third of the mutations adjacent swaps."""
    rng = np.random.default_rng(55)
    base_lens = [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256] + \
        rng.integers(1, 257, size=19).tolist()
    seqs = []
    for n in base_lens:
        base = rng.integers(1, 5, size=n).tolist()
        seqs.append(base)
        for _ in range(9):
            s = list(base)
            for _ in range(int(rng.integers(0, 1 + max(1, n // 8)))):
                op, k = rng.integers(5), int(rng.integers(len(s))) if s else 0
                if op >= 3 and len(s) > 1:
                    k = min(k, len(s) - 2)
                    s[k], s[k + 1] = s[k + 1], s[k]
                elif op == 0 and s:
                    s[k] = int(rng.integers(1, 5))
                elif op == 1 and len(s) > 1:
                    del s[k]
                elif len(s) < 256:
                    s.insert(k, int(rng.integers(1, 5)))
            seqs.append(s)
    assert len(seqs) == 300 and all(1 <= len(s) <= 256 for s in seqs)
    buf, lens = _pack(seqs, 256, np.uint8)
    want = _cpu_rows(buf, lens)
    assert sum(len(w) for w in want) > 10 * len(seqs)
    got = _gpu_rows(buf, lens, True)
    _assert_rows_match(got, want)
    assert _differing_entries(got, _gpu_rows(buf, lens, False)) >= 10


@gpu
def test_short_domain_matches_python_oracle():
    """60 values of at most 16 characters, straight against the DP oracle."""
    from dblink_amd.models.attribute_index import _python_sim_pairs

    rng = np.random.default_rng(56)
    values = set()
    while len(values) < 60:
        base = "".join("abc"[k] for k in rng.integers(3, size=int(rng.integers(1, 15))))
        values.add(base)
        for _ in range(5):
            s = list(base)
            for _ in range(int(rng.integers(1, 4))):
                op, k = int(rng.integers(5)), int(rng.integers(len(s)))
                if op >= 3 and len(s) > 1:
                    k = min(k, len(s) - 2)
                    s[k], s[k + 1] = s[k + 1], s[k]
                elif op == 0:
                    s[k] = "abc"[rng.integers(3)]
                elif op == 1 and len(s) > 1:
                    del s[k]
                elif len(s) < 16:
                    s.insert(k, "abc"[rng.integers(3)])
            values.add("".join(s))
    values = sorted(values)[:59] + [""]
    assert max(map(len, values)) <= 16
    ref = _python_sim_pairs(values, _fn())
    want = [dict(zip(ref.col[ref.row_ptr[v]:ref.row_ptr[v + 1]].tolist(),
                     ref.expsim[ref.row_ptr[v]:ref.row_ptr[v + 1]].tolist()))
            for v in range(len(values))]
    assert sum(len(w) for w in want) > 4 * len(values)
    buf, lens = _pack([list(v.encode()) for v in values], 64, np.uint8)
    _assert_rows_match(_gpu_rows(buf, lens, True), want)


@gpu
def test_default_is_unchanged_levenshtein():
    """The four-argument call and transpositions=False: the same bits."""
    _, buf, lens, _ = _ascii_case()
    buf, lens = buf.to(DEV), lens.to(DEV)

    def canonical(row_ptr, col, expsim):
        V = row_ptr.numel() - 1
        row_of = torch.repeat_interleave(torch.arange(V, device=DEV), row_ptr[1:] - row_ptr[:-1])
        order = torch.argsort(row_of * V + col.to(torch.int64))
        return (row_ptr.cpu().numpy(), col[order].cpu().numpy(),
                expsim[order].cpu().numpy().view(np.int32))

    four = canonical(*C.sim_pairs_gpu(buf, lens, THR, MSIM))
    flag = canonical(*C.sim_pairs_gpu(buf, lens, THR, MSIM, transpositions=False))
    assert four[1].size > 4 * lens.numel()
    for x, y in zip(four, flag):
        np.testing.assert_array_equal(x, y)


@gpu
def test_public_route_sends_damerau_to_the_gpu(monkeypatch):
    values, buf, lens, _ = _ascii_case()
    monkeypatch.setenv("DBLINK_SIM_GPU_MIN_V", "0")
    charset = {ch for v in values for ch in v}
    assert ops.sim_pairs_route(len(values), max(map(len, values)), len(charset),
                               torch.cuda.is_available()) == "gpu"
    idx = ops.sim_pairs(values, _fn())
    row_ptr, col, expsim = C.sim_pairs_cpu(buf, lens, THR, MSIM, True)
    np.testing.assert_array_equal(idx.row_ptr, row_ptr.numpy())
    np.testing.assert_array_equal(idx.col, col.numpy())  # rows sorted by column
    np.testing.assert_allclose(idx.expsim, expsim.numpy(), rtol=1e-5)
