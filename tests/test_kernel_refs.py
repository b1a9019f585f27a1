"""The references of ``kernel_refs`` against the per-record CPU oracle.

The GPU tests compare kernels with formulas written for the tests; a formula
misread the same way as the kernel would pass there. Here each formula is
held to ``cpu_engine``'s per-record update (a third, independently written
implementation): draws from the oracle, frequencies against the formula's
exact probabilities, under the same calibrated bound the GPU tests use. The
numpy index reference is held to ``_build_inverted_index``. No GPU needed.
"""

import types

import numpy as np
import pytest

import kernel_refs as kr
import test_gpu_dense_seq as ds
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
