"""GPU similarity sweep beyond one Myers word: values up to 256 characters
(W = 1..4 words per pattern, one kernel instance per row-length class) and
16-bit symbol ids.

All cases use ``LevenshteinSimilarityFn(5.0, 10.0)``: its inclusion edge
``3d == la + lb`` has ``unit`` exactly 0.5 in fp32 and fp64, so the kernel
and every reference exclude an edge pair identically. Rows are compared as
sets (the fill order is atomic), ``expsim`` to rel 1e-5 (fp32 ``__expf``).
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


def _fn():
    from dblink_amd.models.similarity import LevenshteinSimilarityFn

    return LevenshteinSimilarityFn(THR, MSIM)


def _boundary_domain(seed, fresh, run_sym):
    """23 symbol sequences around the 64/128/192 word boundaries.

    Lengths {0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256}. The four
    chains 256 > 193 > 129 > 65 are nested subsequences (so pairs score
    across word classes); within a chain each shorter neighbour is the longer
    one with its third symbol deleted, which shifts every later word. Each
    long value also has a copy with one substitution at index 63 or 64 and
    one at 127 or 128 (where it is that long). Three single-symbol runs
    (129, 130, 256) drive the add-carry through every word.
    ``fresh(avoid)`` draws a symbol different from ``avoid``.
    """
    rng = np.random.default_rng(seed)

    def drop(seq, n):
        keep = np.sort(rng.choice(len(seq), len(seq) - n, replace=False))
        return [seq[k] for k in keep]

    def delete_front(seq):
        return seq[:2] + seq[3:]

    def substitute(seq, idxs):
        out = list(seq)
        for k in idxs:
            if k < len(out):
                out[k] = fresh(out[k])
        return out

    b256 = [fresh(None) for _ in range(256)]
    b193 = drop(b256, 63)
    b129 = drop(b193, 64)
    b65 = drop(b129, 64)
    b255, b192, b128, b64 = map(delete_front, (b256, b193, b129, b65))
    b127, b63 = delete_front(b128), delete_front(b64)
    longs = [(b256, (63, 127)), (b255, (64, 128)), (b193, (63, 128)), (b192, (64, 127)),
             (b129, (64, 128)), (b128, (63, 127)), (b127, (64,)), (b65, (63,))]
    seqs = [s for s, _ in longs] + [b64, b63, [b256[5]], []]
    seqs += [substitute(s, idxs) for s, idxs in longs]
    seqs += [[run_sym] * 130, [run_sym] * 129, [run_sym] * 256]
    assert len({tuple(s) for s in seqs}) == len(seqs) == 23
    assert {len(s) for s in seqs} >= {0, 1, 63, 64, 65, 127, 128, 129, 192, 193, 255, 256}
    return seqs


@functools.lru_cache(maxsize=None)
def _ascii_case():
    """(values, oracle) for the uint8 word-boundary domain."""
    from dblink_amd.models.attribute_index import _python_sim_pairs

    rng = np.random.default_rng(11)
    letters = "abcd"

    def fresh(avoid):
        while True:
            ch = letters[rng.integers(4)]
            if ch != avoid:
                return ch

    values = ["".join(s) for s in _boundary_domain(12, fresh, "a")]
    return values, _python_sim_pairs(values, _fn())


@functools.lru_cache(maxsize=None)
def _wide_case():
    """(id sequences, oracle) for the 16-bit word-boundary domain: ids drawn
    without replacement from all of 1..65535, so most exceed 8 bits and about
    half have bit 15 set (negative as int16)."""
    from dblink_amd.models.attribute_index import _python_sim_pairs

    rng = np.random.default_rng(13)
    pool = iter(rng.permutation(np.arange(1, 65536)).tolist())
    seqs = _boundary_domain(14, lambda avoid: next(pool), next(pool))
    ids = {x for s in seqs for x in s}
    assert len(ids) > 250 and max(ids) > 32768 and sum(x > 255 for x in ids) > 200
    # one astral character per id: distinct ids <-> distinct characters
    values = ["".join(chr(0x10000 + x) for x in s) for s in seqs]
    return seqs, _python_sim_pairs(values, _fn())


def _pack(seqs, stride, dtype):
    """[V, stride] symbol buffer (0-padded) and int32 lengths, on the GPU."""
    buf = np.zeros((len(seqs), stride), dtype=dtype)
    for i, s in enumerate(seqs):
        buf[i, : len(s)] = s
    if dtype == np.uint16:
        buf = buf.view(np.int16)
    lens = np.array([len(s) for s in seqs], dtype=np.int32)
    return torch.from_numpy(buf), torch.from_numpy(lens)


def _rows(row_ptr, col, expsim):
    row_ptr = np.asarray(row_ptr)
    return [dict(zip(col[row_ptr[v]:row_ptr[v + 1]].tolist(),
                     expsim[row_ptr[v]:row_ptr[v + 1]].tolist()))
            for v in range(len(row_ptr) - 1)]


def _gpu_rows(buf, lens):
    row_ptr, col, expsim = C.sim_pairs_gpu(buf.to(DEV), lens.to(DEV), THR, MSIM)
    return _rows(row_ptr.cpu().numpy(), col.cpu().numpy(), expsim.cpu().numpy())


def _assert_rows_match(got, want):
    assert len(got) == len(want)
    for v, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), f"row {v}: column sets differ"
        for k in w:
            assert g[k] == pytest.approx(w[k], rel=1e-5), f"row {v} col {k}"


@gpu
def test_word_boundaries_uint8_match_oracle():
    values, ref = _ascii_case()
    buf, lens = _pack([list(v.encode()) for v in values], 256, np.uint8)
    got = _gpu_rows(buf, lens)
    want = _rows(ref.row_ptr, ref.col, ref.expsim)
    assert sum(len(w) for w in want) > 4 * len(values)  # many scoring pairs
    _assert_rows_match(got, want)


@gpu
def test_randomized_lengths_match_cpu_sweep():
    """V = 300 in 30 clusters of mutated copies, lengths 1..256, 4 letters,
    against the rolling-array DP of sim_pairs_cpu."""
    rng = np.random.default_rng(21)
    base_lens = [1, 2, 63, 64, 65, 128, 129, 192, 193, 255, 256] + \
        rng.integers(1, 257, size=19).tolist()
    seqs = []
    for n in base_lens:
        base = rng.integers(1, 5, size=n).tolist()
        seqs.append(base)
        for _ in range(9):
            s = list(base)
            for _ in range(int(rng.integers(0, 1 + max(1, n // 8)))):
                op, k = rng.integers(3), int(rng.integers(len(s))) if s else 0
                if op == 0 and s:
                    s[k] = int(rng.integers(1, 5))
                elif op == 1 and len(s) > 1:
                    del s[k]
                elif len(s) < 256:
                    s.insert(k, int(rng.integers(1, 5)))
            seqs.append(s)
    assert len(seqs) == 300 and all(1 <= len(s) <= 256 for s in seqs)
    buf, lens = _pack(seqs, 256, np.uint8)
    row_ptr, col, expsim = C.sim_pairs_cpu(buf, lens, THR, MSIM)
    want = _rows(row_ptr.numpy(), col.numpy(), expsim.numpy())
    assert sum(len(w) for w in want) > 10 * len(seqs)
    _assert_rows_match(_gpu_rows(buf, lens), want)


@gpu
def test_word_boundaries_16bit_symbols_match_oracle():
    seqs, ref = _wide_case()
    buf, lens = _pack(seqs, 256, np.uint16)
    assert buf.dtype == torch.int16
    _assert_rows_match(_gpu_rows(buf, lens), _rows(ref.row_ptr, ref.col, ref.expsim))


@gpu
def test_16bit_symbols_are_not_truncated_to_8_bits():
    """Ids equal modulo 256 are different symbols."""
    from dblink_amd.models.attribute_index import _python_sim_pairs

    seqs = [[5], [261], [5, 300, 7, 9], [261, 300, 7, 9], [5 + 512, 300, 7, 9],
            [44, 300, 7, 9 + 256], [5, 300 + 256, 7, 9], []]
    values = ["".join(chr(0x10000 + x) for x in s) for s in seqs]
    ref = _python_sim_pairs(values, _fn())
    want = _rows(ref.row_ptr, ref.col, ref.expsim)
    assert 3 in want[2] and 1 not in want[0]  # d = 1: scoring at length 4, not at length 1
    buf, lens = _pack(seqs, 64, np.uint16)
    _assert_rows_match(_gpu_rows(buf, lens), want)


@gpu
def test_short_rows_unchanged_by_long_values():
    """Rows of <= 64 characters run the one-word instance whatever else the
    domain holds: same columns and same expsim bits as a [V, 64] run."""
    short = sorted({
        "Australian Capital Territory", "New South Wales", "Northern Territory",
        "Queensland", "South Australia", "Tasmania", "Victoria", "Western Australia",
        "ANNA", "ANNE", "ANNAH", "BOB", "BORB", "",
    })
    rng = np.random.default_rng(31)
    long_base = "".join(rng.choice(list("ANEBO rst"), size=200))
    longs = [long_base, long_base[:99] + "#" + long_base[100:], long_base[::-1]]
    mixed = longs[:1] + short[:7] + longs[1:2] + short[7:] + longs[2:]
    new_id = {mixed.index(v): i for i, v in enumerate(short)}

    def run(values, stride):
        buf, lens = _pack([list(v.encode()) for v in values], stride, np.uint8)
        row_ptr, col, expsim = C.sim_pairs_gpu(buf.to(DEV), lens.to(DEV), THR, MSIM)
        return _rows(row_ptr.cpu().numpy(), col.cpu().numpy(),
                     expsim.cpu().numpy().view(np.int32))

    alone = run(short, 64)
    both = run(mixed, 256)
    assert sum(len(r) for r in alone) > len(short)
    for m, i in new_id.items():
        remapped = {new_id[c]: bits for c, bits in both[m].items() if c in new_id}
        assert len(remapped) == len(both[m])  # no long value is similar to a short one
        assert remapped == alone[i]
    # the long rows found each other
    assert mixed.index(longs[1]) in both[mixed.index(longs[0])]


@gpu
def test_public_route_takes_long_values_to_the_gpu(monkeypatch):
    values, ref = _ascii_case()
    monkeypatch.setenv("DBLINK_SIM_GPU_MIN_V", "0")
    charset = {ch for v in values for ch in v}
    assert ops.sim_pairs_route(len(values), max(map(len, values)), len(charset),
                               torch.cuda.is_available()) == "gpu"
    idx = ops.sim_pairs(values, _fn())
    np.testing.assert_array_equal(idx.row_ptr, ref.row_ptr)
    np.testing.assert_array_equal(idx.col, ref.col)  # rows sorted by column
    np.testing.assert_allclose(idx.expsim, ref.expsim, rtol=1e-5)


@gpu
def test_stride_above_256_is_rejected():
    buf = torch.zeros((2, 257), dtype=torch.uint8, device=DEV)
    lens = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="256"):
        C.sim_pairs_gpu(buf, lens, THR, MSIM)
