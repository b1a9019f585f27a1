"""List mode of the k >= 2 value update (``value_update_lists``).

In list mode ``value_update_kd1_kernel`` classifies every k >= 2 (entity,
attribute) pair once per sweep and appends it to the list of the kernel that
owns it (LDS hash, or union merge / chunked hash); the two wave kernels then
run one wave per listed pair from a static grid. Which kernel handles a pair
is a performance decision, so list mode, the self-selecting kobs mode
(``DBLINK_VALUE_LISTS=0``) and, where the k-tables are cleared and no pair has
k = 1, the explicit pair-list mode must return ``torch.equal`` entity values.
The lists, read back as sets, must equal ``_route_ref``, a numpy transcription
of the predicates of ``value_route`` / ``value_update_pair`` (kernels.hip).

Draws are keyed by the entity's index, so "the same state with the entities
permuted" has other random numbers per entity: what is checked there is that
the permuted state (whose lists fill in another order) again agrees between
the three modes and with the transcription, and that the values that do not
depend on a draw (held values) follow their entities.
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

HASH_LIMIT = (1024 * 3) // 4   # value_is_dense: more entries go to the merge kernel
VAL_DMAX = 16
NC = 64                        # entities per class, as in test_gpu


def _dev(arr, dtype):
    return torch.as_tensor(np.ascontiguousarray(arr)).to(dtype).to(DEV)


# ---- models ----------------------------------------------------------------------


def _ball():
    """test_gpu's 650-name mutation ball: attribute 0 constant (10 years),
    attribute 1 names with sim rows of 262-384 and 650 entries."""
    from test_gpu import _mutation_ball_model

    cache, model = _mutation_ball_model()
    row_lens = [np.ones(cache.indexed_attributes[0].index.num_values, dtype=np.int64),
                np.diff(cache.indexed_attributes[1].index.sim_index.row_ptr)]
    return model, row_lens


@functools.lru_cache(maxsize=None)
def _small_cache():
    """One Levenshtein attribute over 400 names with sim rows of 6-286 entries:
    E * A can be odd, and row lengths add up to 768 and 769 exactly."""
    from dblink_amd.models.records import (Attribute, BetaShapeParameters, RecordsCache,
                                           RecordsTable)
    from dblink_amd.models.similarity import LevenshteinSimilarityFn

    rng = np.random.default_rng(3)
    base = list("ABCABCABCA")
    pool = set()
    while len(pool) < 400:
        s = base.copy()
        for _ in range(rng.integers(1, 4)):
            s[rng.integers(0, 10)] = "ABCDE"[rng.integers(0, 5)]
        pool.add("".join(s))
    rows = [[n] for n in sorted(pool)]
    table = RecordsTable.from_rows([str(i) for i in range(len(rows))],
                                   ["0"] * len(rows), rows)
    attrs = [Attribute("name", LevenshteinSimilarityFn(7.5, 10.0),
                       BetaShapeParameters(0.5, 50.0))]
    return RecordsCache.build(table, attrs, max_cluster_size=10)


@functools.lru_cache(maxsize=None)
def _small():
    from dblink_amd.engine.gpu_engine import GpuModel

    cache = _small_cache()
    row_lens = [np.diff(cache.indexed_attributes[0].index.sim_index.row_ptr)]
    return GpuModel(cache, DEV, 10), row_lens


def _rows_summing(row_lens, target, max_rows=12):
    """Distinct rows whose lengths add up to ``target`` (subset sum)."""
    best = {0: []}
    for i in np.argsort(-row_lens, kind="stable"):
        for s, rows in list(best.items()):
            t = s + int(row_lens[i])
            if t <= target and t not in best and len(rows) < max_rows:
                best[t] = rows + [int(i)]
        if target in best:
            return best[target]
    raise AssertionError(f"no rows add up to {target}")


def test_small_model_rows_reach_both_sides_of_the_hash_limit():
    row_lens = np.diff(_small_cache().indexed_attributes[0].index.sim_index.row_ptr)
    for target in (HASH_LIMIT, HASH_LIMIT + 1):
        rows = _rows_summing(row_lens, target)
        assert len(set(rows)) == len(rows) <= VAL_DMAX
        assert row_lens[rows].sum() == target


# ---- states ----------------------------------------------------------------------


class State:
    """Entities as lists of records ``(values, file, dist)``; values and dist
    have one entry per attribute. Records are stored grouped by entity."""

    def __init__(self, entities, A):
        self.entities, self.A = entities, A
        rv, rd, rf, ptr = [], [], [], [0]
        for recs in entities:
            for values, f, dist in recs:
                rv.append(values)
                rd.append(dist)
                rf.append(f)
            ptr.append(len(rv))
        self.E, self.R = len(entities), len(rv)
        self.rv = np.array(rv, dtype=np.int32).reshape(self.R, A)
        self.rd = np.array(rd, dtype=np.uint8).reshape(self.R, A)
        self.rf = np.array(rf, dtype=np.int32)
        self.ptr = np.array(ptr, dtype=np.int64)
        self.kobs = np.array([[sum(1 for v, _, _ in recs if v[a] >= 0) for a in range(A)]
                              for recs in entities], dtype=np.int32).reshape(-1)

    def permuted(self, perm):
        return State([self.entities[i] for i in perm], self.A)


def _route_ref(st, row_lens, is_const, collapsed, Kc, ktab_max):
    """(hash, merge, kd1) pair sets by the rules of kernels.hip: a pair is
    settled early (non-collapsed: a held value, or a constant attribute) and
    then belongs to the hash kernel; else its distinct (value, file) groups in
    record order (beyond VAL_DMAX: every record its own unit) give the entry
    total; one group with a cached k-table is kd1's; more than 768 entries go
    to the merge kernel."""
    hash_, merge, kd1 = set(), set(), set()
    for e, recs in enumerate(st.entities):
        for a in range(st.A):
            obs = [(v[a], f if collapsed else 0, d[a]) for v, f, d in recs if v[a] >= 0]
            k = len(obs)
            if k < 2:
                continue
            pair = e * st.A + a
            if not collapsed and (is_const[a] or any(not d for _, _, d in obs)):
                hash_.add(pair)
                continue
            groups = list(dict.fromkeys((x, f) for x, f, _ in obs))
            gover = len(groups) > VAL_DMAX
            units = [x for x, _, _ in obs] if gover else [x for x, _ in groups]
            total = sum(int(row_lens[a][x]) for x in units)
            if (ktab_max >= 2 and not is_const[a] and not gover and len(groups) == 1
                    and k <= ktab_max and k <= Kc):
                kd1.add(pair)
            elif total > HASH_LIMIT:
                merge.add(pair)
            else:
                hash_.add(pair)
    return hash_, merge, kd1


def _set_tables(model, on):
    if on:
        assert model.ktab_max >= 2
        C.set_value_ktables(model.ktab_excl, model.ktab_rawsum, model.self_expsim,
                            model.ktab_max, int(model.csr_col.numel()))
    else:
        z = torch.empty(0, dtype=torch.float64)
        C.set_value_ktables(z, z, torch.empty(0, dtype=torch.float32), 0, 0)
    z = torch.empty(0, dtype=torch.float64)
    C.set_value_k2tables(z, z, 0)


def _run(model, st, mode, collapsed=1, grid=2048, F=2):
    """ent_values after one value update, and in list mode the two lists."""
    A, E = st.A, st.E
    theta = _dev(np.tile(np.array([[0.05, 0.2, 0.1][:F]]), (A, 1)) *
                 (1.0 + np.arange(A)[:, None]), torch.float32)
    ev = torch.full((E, A), -3, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    none32 = torch.empty(0, dtype=torch.int32, device=DEV)
    wave_pairs, kobs = empty64, _dev(st.kobs, torch.int32)
    lists, counts = none32, none32
    if mode == "explicit":
        wave_pairs, kobs = torch.arange(E * A, dtype=torch.int64, device=DEV), none32
    elif mode == "lists":
        lists = torch.full((E * A,), -1, dtype=torch.int32, device=DEV)
        counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    else:
        assert mode == "kobs"
    C.value_update_lists(
        _dev(st.rv, torch.int32), _dev(st.rd, torch.uint8), _dev(st.rf, torch.int32),
        _dev(st.ptr, torch.int64), torch.arange(st.R, dtype=torch.int64, device=DEV), ev,
        theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        collapsed, 0, 2718, 3, 0, err, wave_pairs, empty64, empty64,
        model.csr_excl, model.csr_rawsum, model.z1, empty64, kobs,
        lists, counts, grid)
    torch.cuda.synchronize()
    assert int(err.cpu()) == 0
    if mode != "lists":
        return ev.cpu()
    n_hash, n_merge = counts.cpu().tolist()
    host = lists.cpu().numpy()
    hash_l, merge_l = host[:n_hash].tolist(), host[E * A - n_merge:].tolist()
    assert n_hash + n_merge <= E * A
    # each listed pair once, on one list
    assert len(set(hash_l)) == n_hash and len(set(merge_l)) == n_merge
    assert not set(hash_l) & set(merge_l)
    return ev.cpu(), set(hash_l), set(merge_l)


def _assert_modes_agree(model, row_lens, st, collapsed=1, tables=False, explicit=True,
                        grid=2048):
    """List mode == kobs mode (== explicit mode), lists == transcription."""
    _set_tables(model, tables)
    try:
        by_lists, hash_l, merge_l = _run(model, st, "lists", collapsed, grid)
        by_kobs = _run(model, st, "kobs", collapsed)
        assert torch.equal(by_lists, by_kobs)
        if explicit:
            assert not tables and not (st.kobs == 1).any()
            assert torch.equal(by_lists, _run(model, st, "explicit", collapsed))
        is_const = model.attr_const.cpu().numpy().astype(bool)
        ref = _route_ref(st, row_lens, is_const, collapsed, model.Kc,
                         model.ktab_max if tables else 0)
        assert hash_l == ref[0] and merge_l == ref[1]
        assert (by_lists != -3).all()      # every pair was written by someone
        return by_lists, ref
    finally:
        _set_tables(model, False)


def _rec(values, f=0, dist=1):
    return (tuple(values), f, tuple([dist] * len(values)))


def _seven_classes(row_lens_name):
    """The pair classes of test_value_pairlist_and_kobs_paths_agree_bitwise:
    (a) d=1 hash, (b) d=2 hash, (c) two 650-entry rows, (d) three short rows,
    (e) one value in two files, (f) 17 distinct rows (more than VAL_DMAX
    groups, k > Kc), (g) k = 0."""
    order = np.argsort(row_lens_name, kind="stable")
    short = order[row_lens_name[order] < 650]
    long_ = order[row_lens_name[order] == 650]
    assert len(short) >= NC + 17 and len(long_) >= 2
    classes = {
        "a": lambda i: [(short[i], 0)] * 2,
        "b": lambda i: [(short[i], 0), (short[i + 1], 0)],
        "c": lambda i: [(long_[i % len(long_)], 0), (long_[(i + 1) % len(long_)], 0)],
        "d": lambda i: [(short[i + j], 0) for j in range(3)],
        "e": lambda i: [(short[i], 0), (short[i], 1)],
        "f": lambda i: [(short[i + j], 0) for j in range(17)],
        "g": lambda i: [],
    }
    entities, cls_of = [], []
    for name, recs_of in classes.items():
        for i in range(NC):
            entities.append([_rec(((len(entities) + j) % 10, int(x)), f)
                             for j, (x, f) in enumerate(recs_of(i))])
            cls_of.append(name)
    return State(entities, 2), np.array(cls_of)


# ---- tests -----------------------------------------------------------------------


@gpu
@pytest.mark.parametrize("vchunk", ["1", "0"])
def test_seven_classes_agree_in_all_modes(monkeypatch, vchunk):
    model, row_lens = _ball()
    st, cls_of = _seven_classes(row_lens[1])
    monkeypatch.setenv("DBLINK_VCHUNK", vchunk)
    by_lists, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st)
    # not vacuous: name pairs of a, b, e hash, of c, d, f merge; f has more
    # than VAL_DMAX groups and k > Kc; the constant pairs all hash
    name_pair = np.arange(st.E) * 2 + 1
    assert set(name_pair[np.isin(cls_of, ["a", "b", "e"])]) <= hash_ref
    assert set(name_pair[np.isin(cls_of, ["c", "d", "f"])]) == merge_ref
    assert (st.kobs[name_pair[cls_of == "f"]] > max(model.Kc, VAL_DMAX)).all()
    assert (by_lists != 0).float().mean() > 0.5

    # a grid shorter than both lists (2 blocks = 8 waves): the stride serves them
    assert min(len(hash_ref), len(merge_ref)) > 8
    capped, _ = _assert_modes_agree(model, row_lens, st, grid=2, explicit=False)
    assert torch.equal(capped, by_lists)

    # entities permuted: the lists fill in another order
    perm = np.random.default_rng(1).permutation(st.E)
    _assert_modes_agree(model, row_lens, st.permuted(perm))


@gpu
def test_kd1_pairs_are_on_no_list():
    """With the k-tables set, single-group pairs within the tables are kd1's:
    list mode and kobs mode agree and those pairs appear on neither list."""
    model, row_lens = _ball()
    st, cls_of = _seven_classes(row_lens[1])
    _, (hash_ref, merge_ref, kd1_ref) = _assert_modes_agree(
        model, row_lens, st, tables=True, explicit=False)
    name_pair = np.arange(st.E) * 2 + 1
    assert kd1_ref == set(name_pair[cls_of == "a"])
    assert not kd1_ref & (hash_ref | merge_ref)


@gpu
@pytest.mark.parametrize("E", [1, 7, 8, 9])
def test_few_pairs(E):
    model, row_lens = _small()
    order = np.argsort(row_lens[0], kind="stable")
    st = State([[_rec((int(order[i + j]),)) for j in range(2 + i % 2)] for i in range(E)], 1)
    assert st.E * st.A == E and (st.kobs >= 2).all()
    _, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st)
    assert len(hash_ref) + len(merge_ref) == E


@gpu
def test_no_pair_with_two_records():
    """Only k = 0 and k = 1 pairs: both lists stay empty, nothing faults and
    the wave kernels write nothing (kobs mode returns the same values)."""
    model, row_lens = _ball()
    entities = [[_rec((i % 10, i % 600))] if i % 3 else [] for i in range(100)]
    st = State(entities, 2)
    assert (st.kobs < 2).all() and (st.kobs == 1).any() and (st.kobs == 0).any()
    _, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st, explicit=False)
    assert not hash_ref and not merge_ref


@gpu
def test_every_pair_listed_and_more_pairs_than_waves():
    model, row_lens = _small()
    order = np.argsort(row_lens[0], kind="stable")
    st = State([[_rec((int(order[i + j]),)) for j in range(2)] for i in range(40)], 1)
    _, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st, grid=2)
    assert len(hash_ref) + len(merge_ref) == st.E * st.A == 40 > 2 * 4


@gpu
def test_hash_limit_both_sides():
    """Row-length totals of exactly 768 (the last hash pair) and 769 (the
    first merge pair)."""
    model, row_lens = _small()
    at, above = (_rows_summing(row_lens[0], t) for t in (HASH_LIMIT, HASH_LIMIT + 1))
    st = State([[_rec((x,)) for x in at], [_rec((x,)) for x in above]], 1)
    _, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st)
    assert hash_ref == {0} and merge_ref == {1}


@gpu
def test_noncollapsed_held_value_is_written_once():
    """Non-collapsed: a k >= 2 pair with a non-distorted record takes the held
    value. Both wave kernels used to write it; now it is on the hash list
    alone. Pairs without a held value take their usual routes."""
    model, row_lens = _ball()
    order = np.argsort(row_lens[1], kind="stable")
    held, other, long_ = int(order[5]), int(order[9]), int(order[-1])
    assert row_lens[1][long_] == 650
    entities = []
    for i in range(NC):
        # name: first record distorted, second held; year distorted throughout
        entities.append([((i % 10, other), 0, (1, 1)), ((i % 10, held), 0, (1, 0))])
        # all distorted: two long rows -> merge
        entities.append([_rec((i % 10, long_)), _rec((i % 10, int(order[-2])))])
    st = State(entities, 2)
    by_lists, (hash_ref, merge_ref, _) = _assert_modes_agree(model, row_lens, st,
                                                            collapsed=0)
    held_pairs = set((np.arange(0, st.E, 2) * 2 + 1).tolist())
    assert held_pairs <= hash_ref and not held_pairs & merge_ref
    assert len(merge_ref) == NC
    assert (by_lists[0::2, 1] == held).all()
    # held values follow their entities under a permutation
    perm = np.random.default_rng(2).permutation(st.E)
    moved, _ = _assert_modes_agree(model, row_lens, st.permuted(perm), collapsed=0)
    was_held = perm % 2 == 0
    assert (moved[torch.as_tensor(was_held), 1] == held).all()
