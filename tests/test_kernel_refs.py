"""The references of ``kernel_refs`` against the per-record CPU oracle.

The GPU tests compare kernels with formulas written for the tests; a formula
misread the same way as the kernel would pass there. Here each formula is
held to ``cpu_engine``'s per-record update (a third, independently written
implementation): draws from the oracle, frequencies against the formula's
exact probabilities, under the same calibrated bound the GPU tests use. The
numpy index reference is held to ``_build_inverted_index``, the numpy Philox
to the Random123 known-answer vectors and to the CPU sampler's Philox. No GPU
needed.
"""

import types

import numpy as np
import pytest

import kernel_refs as kr
import test_gpu_dense_seq as ds
import test_gpu_value_dist as vd
from test_gpu import make_model

torch = pytest.importorskip("torch")

from dblink_amd.engine import cpu_engine as ce  # noqa: E402


@pytest.fixture(scope="module")
def attrs():
    cache, _ = make_model(torch.device("cpu"))
    return cache.indexed_attributes


def _assert_oracle_matches(label, draws, exact, seed, group=None, ngroups=None):
    n = len(draws)
    emp = np.bincount(draws, minlength=len(exact)) / n
    if group is not None:
        emp = kr.group_probs(emp, group, ngroups)
        exact = kr.group_probs(exact, group, ngroups)
    worst, bound = kr.calibrated_bound(exact, n, seed=seed)
    got = kr.tv(emp, exact)
    assert got < bound, (label, got, worst, bound)


@pytest.mark.parametrize("k", range(4))
def test_collapsed_link_formula_matches_oracle(attrs, k):
    cls = ds.COLLAPSED_CLASSES[k]
    _, rv, f, p = cls
    ev = ds._dense_entities()
    e0, e1 = int(ds.ENT_PTR[p]), int(ds.ENT_PTR[p + 1])
    exact = ds._class_exact(attrs, ev, ds.ENT_PTR, cls, 1)[e0:e1]
    rng = np.random.default_rng(40 + k)
    theta = lambda a, file_id: float(ds.THETA[a, file_id])  # noqa: E731
    draws = np.array([
        ce._update_entity_id_collapsed(rng, np.array(rv), ev[e0:e1], attrs, theta, f)
        for _ in range(8000)])
    group, ng = ds._profile_groups(ev[e0:e1], rv, 0, np.array([0, e1 - e0]))
    _assert_oracle_matches(cls[0], draws, exact, 300 + k, group, ng)


@pytest.mark.parametrize("k", range(4))
def test_seq_link_formula_matches_oracle(attrs, k):
    cls = ds.SEQ_CLASSES[k]
    _, rv, rd, p = cls
    ev = ds._dense_entities()
    e0, e1 = int(ds.ENT_PTR[p]), int(ds.ENT_PTR[p + 1])
    exact = ds._class_exact(attrs, ev, ds.ENT_PTR, cls, 0)[e0:e1]
    if k != 1:  # every class but 'both distorted' excludes some entity
        assert (exact == 0).any()
    rng = np.random.default_rng(50 + k)
    draws = np.array([
        ce._update_entity_id_seq(rng, np.array(rv), np.array(rd), ev[e0:e1], attrs)
        for _ in range(3000)])
    group, ng = ds._profile_groups(ev[e0:e1], rv, 0, np.array([0, e1 - e0]))
    _assert_oracle_matches(cls[0], draws, exact, 310 + k, group, ng)


def test_seq_value_formula_matches_oracle(attrs):
    year, name = attrs
    x1, x2 = 0, 2
    # records: 0, 1 two distorted; 2 name missing; 3 distorted, 4 held
    part = types.SimpleNamespace(
        rec_values=np.array([[3, x1], [5, x2], [6, -1], [3, x1], [5, x2]]),
        rec_dist=np.array([[1, 1], [1, 1], [1, 1], [0, 1], [1, 0]], dtype=np.uint8))
    rng = np.random.default_rng(60)
    n = 20000

    def draw(a, ia, linked):
        return np.array([ce._update_entity_value_seq(rng, a, ia, part, linked)
                         for _ in range(n)])

    two = kr.seq_value_probs(name, [x1, x2])
    _assert_oracle_matches("two distorted", draw(1, name, [0, 1]), two, 320)
    _assert_oracle_matches("plus missing", draw(1, name, [0, 1, 2]), two, 321)
    phi = kr.seq_value_probs(name, [])
    _assert_oracle_matches("no record", draw(1, name, []), phi, 322)
    _assert_oracle_matches("missing only", draw(1, name, [2]), phi, 323)
    _assert_oracle_matches("constant", draw(0, year, [0, 1]),
                           kr.seq_value_probs(year, [3, 5]), 324)
    assert (draw(1, name, [3, 4])[:50] == x2).all()
    assert (draw(0, year, [3, 4])[:50] == 3).all()


# ---- Philox with the GPU keying ------------------------------------------------------

# (counter words, key words, output words): the Random123 known-answer vectors
# of philox4x32_10
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("ctr, key, want", PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    from dblink_amd.engine import cpu_fast as cf

    seed = key[0] | (key[1] << 32)
    got = kr.philox4x32(seed, *ctr)
    assert [int(np.asarray(w).reshape(-1)[0]) for w in got] == list(want)
    # the CPU sampler's Philox puts the draw in word 2 and the iteration in
    # word 3, and folds phase and rank into the key: nothing at phase 0, rank 0
    ids = np.array([ctr[0] | (ctr[1] << 32)], dtype=np.uint64)
    us = cf._philox_uniform4(seed, ctr[3], 0, ids, ctr[2], 0)
    assert [int(u[0] * 2.0 ** 32 - 0.5) for u in us] == list(want)


def test_philox_is_vectorised_and_gpu_uniform_keys_it():
    rng = np.random.default_rng(5)
    seed = 0x9E3779B97F4A7C15
    elem = rng.integers(0, 1 << 45, size=64).astype(np.uint64)
    elem[0] = (1 << 32) - 1        # all-ones low word
    elem[1] = 1 << 32              # low word 0, high word 1
    it, phase, draw = 77, 4, 0xFFFF0000
    c2 = it ^ (phase << 24)
    whole = kr.philox4x32(seed, elem & np.uint64(0xFFFFFFFF), elem >> np.uint64(32),
                          c2, draw)
    for i in (0, 1, 2, 63):
        lo, hi = int(elem[i]) & 0xFFFFFFFF, int(elem[i]) >> 32
        one = kr.philox4x32(seed, lo, hi, c2, draw)
        assert [int(w[i]) for w in whole] == [int(w) for w in one]
    for word in range(4):
        u = kr.gpu_uniform(seed, it, phase, elem, draw, word)
        assert u.dtype == np.float64 and (u > 0).all() and (u < 1).all()
        np.testing.assert_array_equal(
            u, (whole[word].astype(np.float64) + 0.5) * 2.0 ** -32)
    # the phase sits in bits 24.. of counter word 2, not in the key
    assert not np.array_equal(kr.gpu_uniform(seed, it, 2, elem, 0),
                              kr.gpu_uniform(seed, it, 4, elem, 0))
    np.testing.assert_array_equal(kr.gpu_uniform(seed, it ^ (6 << 24), 2, elem, 0),
                                  kr.gpu_uniform(seed, it, 4, elem, 0))


# ---- value conditional ----------------------------------------------------------------


@pytest.fixture(scope="module")
def attrs_kc4():
    cache, _ = make_model(torch.device("cpu"), **vd.MODEL_KW)
    return cache.indexed_attributes


def _value_part(cls):
    """The class's records as the oracle reads them, every one distorted."""
    _, a, recs, _ = cls
    rv = np.full((len(recs), 2), -1, dtype=np.int64)
    rv[:, a] = [x for x, _ in recs]
    part = types.SimpleNamespace(
        rec_values=rv, rec_file=np.array([f for _, f in recs]),
        rec_dist=np.ones((len(recs), 2), dtype=np.uint8))
    return part, list(range(len(recs)))


def _oracle_value_draws(attrs, cls, n, seed):
    _, a, _, collapsed = cls
    part, linked = _value_part(cls)
    rng = np.random.default_rng(seed)
    theta = lambda b, f: float(vd.THETA[b, f])  # noqa: E731
    if collapsed:
        return np.array([ce._update_entity_value_collapsed(rng, a, attrs[a], part, linked,
                                                           theta) for _ in range(n)])
    return np.array([ce._update_entity_value(rng, a, attrs[a], part, linked)
                     for _ in range(n)])


# collapsed classes with _FAST_VALUE off and on; _update_entity_value has one path
ORACLE_CASES = [(k, fast) for k, c in enumerate(vd.CLASSES)
                for fast in ((False, True) if c[3] else (False,))]


@pytest.mark.parametrize("k, fast", ORACLE_CASES)
def test_value_formula_matches_oracle(attrs_kc4, k, fast, monkeypatch):
    cls = vd.CLASSES[k]
    monkeypatch.setattr(ce, "_FAST_VALUE", fast)
    exact, other = vd.class_exact(attrs_kc4, cls)
    draws = _oracle_value_draws(attrs_kc4, cls, 6000, 80 + k)
    _assert_oracle_matches(cls[0], draws, exact, 330 + k)
    # the attribute the class does not observe: phi
    np.testing.assert_allclose(other, attrs_kc4[1 - cls[1]].index.probs, rtol=1e-12)


@pytest.fixture(scope="module")
def long_row_attrs():
    """200 names within two substitutions of one another at threshold 7 of 10:
    similarity rows of 128 entries and more."""
    rng = np.random.default_rng(11)
    pool = set()
    while len(pool) < 200:
        s = list("ABCABCABCA")
        for _ in range(rng.integers(1, 3)):
            s[rng.integers(0, 10)] = "ABCDE"[rng.integers(0, 5)]
        pool.add("".join(s))
    cache, _ = make_model(torch.device("cpu"), threshold=7.0, names=sorted(pool))
    return cache.indexed_attributes


@pytest.mark.parametrize("fast", [False, True], ids=["dict", "fast"])
def test_value_formula_matches_oracle_on_a_long_row(long_row_attrs, fast, monkeypatch):
    """k = 1 where the oracle's vectorised single-record path engages (rows of
    128 entries or more), which the eight-name model never reaches."""
    name = long_row_attrs[1]
    row_lens = np.diff(name.index.sim_index.row_ptr)
    x = int(np.argmax(row_lens))
    assert row_lens[x] >= 128
    monkeypatch.setattr(ce, "_FAST_VALUE", fast)
    cls = ("long row", 1, [(x, 1)], 1)
    exact = kr.value_probs(name, vd.THETA[1], [(x, 1)], 1)
    assert exact.max() < 0.9            # not all on x
    draws = _oracle_value_draws(long_row_attrs, cls, 6000, 95)
    group = kr.heaviest_plus_rest(exact, 20)
    _assert_oracle_matches("long row", draws, exact, 345, group, 21)


def _bound_30000(exact, k):
    """The bound the GPU test puts on class k's own attribute."""
    return kr.calibrated_bound(exact, vd.N_VAL, seed=400 + 2 * k)[1]


def test_value_classes_are_sensitive(attrs_kc4):
    """On the reference alone: a class with two files must tell swapped
    thetas apart, a class with k >= 3 must tell k - 1 apart (whichever record
    is dropped), each by more than twice its calibrated bound. Otherwise a
    file-blind theta index or an off-by-one level would pass the GPU test."""
    swapped = vd.THETA[:, ::-1]
    two_file, deep = 0, 0
    for k, cls in enumerate(vd.CLASSES):
        _, a, recs, collapsed = cls
        obs = vd.observed(recs)
        exact = kr.value_probs(attrs_kc4[a], vd.THETA[a], obs, collapsed)
        bound = _bound_30000(exact, k)
        if collapsed and len({f for _, f in recs}) == 2:
            moved = kr.tv(exact, kr.value_probs(attrs_kc4[a], swapped[a], obs, collapsed))
            print(f"{cls[0]}: swapped thetas move it by {moved:.5f}, bound {bound:.5f}")
            assert moved > 2 * bound, (cls[0], moved, bound)
            two_file += 1
        if len(obs) >= 3 and not (attrs_kc4[a].is_constant and not collapsed):
            for drop in range(len(obs)):
                fewer = obs[:drop] + obs[drop + 1:]
                moved = kr.tv(exact, kr.value_probs(attrs_kc4[a], vd.THETA[a], fewer,
                                                    collapsed))
                print(f"{cls[0]}: without record {drop} it moves by {moved:.5f}, "
                      f"bound {bound:.5f}")
                assert moved > 2 * bound, (cls[0], drop, moved, bound)
            deep += 1
    assert two_file == 4 and deep == 7   # classes 5, 6, 7, 9 and 2, 3, 4, 5, 6, 9, 11


@pytest.mark.parametrize("pairs", [[], [(0, 1, 31)]], ids=["NP0", "NP1"])
def test_index_reference_matches_cpu_inverted_index(pairs):
    """Per partition, _build_inverted_index over the slot values (singles, then
    composites) gives each (slot, value)'s ascending local entity ids: the
    reference's segment of that key, shifted by the partition's offset."""
    rng = np.random.default_rng(70)
    sizes = [40, 25, 60]
    ent_part = np.repeat(np.arange(3), sizes)
    vals = np.stack([rng.integers(0, v, size=125) for v in (12, 31, 400)], 1)
    vmax = 400
    keys, counts, ptr, postings = kr.index_reference(ent_part, vals, pairs, vmax, 3)
    sv = kr.slot_values(vals, pairs)
    T = sv.shape[1]
    assert len(keys) == T * 125 and counts.sum() == T * 125
    seen = 0
    for p in range(3):
        e0 = int(np.sum(sizes[:p]))
        inv = ce._build_inverted_index(sv[ent_part == p])
        for (t, v), local in inv.items():
            key = (p * T + t) * vmax + v
            np.testing.assert_array_equal(postings[ptr[key]:ptr[key + 1]], local + e0)
            seen += len(local)
    assert seen == T * 125  # every posting belongs to a key of the oracle

    # query side: a record equal to an entity finds it in every observed slot
    rv = vals[[3, 50, 110]].copy()
    rv[1, 0] = -1
    qk = kr.query_keys(ent_part[[3, 50, 110]], rv, pairs, vmax)
    assert qk[1, 0] == -1 and (not pairs or qk[1, 3] == -1)
    for i, e in enumerate((3, 50, 110)):
        for t in range(T):
            if qk[i, t] >= 0:
                assert e in postings[ptr[qk[i, t]]:ptr[qk[i, t] + 1]]


def test_classify_reference_on_hand_cases():
    ent_ptr = np.array([0, 600, 605])
    rv = np.array([[1, 2, 3]] * 6)
    rv[5, 0] = -1
    rd = np.array([[1, 1, 1], [0, 1, 1], [0, 0, 1], [0, 1, 1], [1, 1, 1], [0, 0, 1]],
                  dtype=np.uint8)
    part = np.array([0, 0, 0, 0, 1, 0])
    lo = np.zeros((6, 3), dtype=np.int64)
    hi = np.array([[9, 9, 9], [513, 1, 1], [513, 600, 1], [16, 1, 1], [1, 1, 1],
                   [1, 17, 1]], dtype=np.int64)
    # no nd + pool 600 > 512; one nd above; two nd (never heavy), best 513;
    # one nd at the small threshold; no nd + pool 5; missing attr ignored
    want = [2, 2, 0, 1, 0, 0]
    got = kr.classify_modes_reference(rv, rd, part, ent_ptr, lo, hi, 16, 512)
    assert got.tolist() == want
    got0 = kr.classify_modes_reference(rv, rd, part, ent_ptr, lo, hi, 16, 0)
    assert got0.tolist() == [0, 0, 0, 1, 0, 0]
