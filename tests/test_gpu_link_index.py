"""The inverted-index build of the indexed link phase, op by op, against numpy.

``postings_hist``, ``postings_scatter``, ``cand_ranges``, ``build_keys``,
``build_ekeys_stable`` + ``radix_sort_pairs_i64_i32`` and ``classify_modes``
see only integer tensors, so every comparison is exact. The reference
(``kernel_refs.index_reference``) is the definition: key =
``(part * T + t) * Vmax + v``, ``bincount``, its prefix, and per key the
entities holding it. ``test_kernel_refs`` holds that reference to the CPU
engine's ``_build_inverted_index``.

The second half checks that the constant-attribute pair slots
(``DBLINK_CONST_PAIRS=1``) and the stable-sort route (``DBLINK_FORCE_SORT=1``)
change no draw: the Gumbel keys are (record gid, entity id), so neither the
base a record enumerates nor the order inside a posting range may matter.
"""

import functools

import numpy as np
import pytest

import kernel_refs as kr

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)


def _t(arr, dtype):
    return torch.as_tensor(np.ascontiguousarray(arr)).to(dtype).to(DEV)


# ---- cases -----------------------------------------------------------------------

RANGES3 = (12, 31, 400)   # value ranges of the three attributes
VMAX = 400                # what the engine passes: max(Vmax, composite domain 372)
PAIR = [(0, 1, 31)]       # (a1, a2, V2): composite value v0 * 31 + v1 < 372
NUM_PARTS = 3


def _parts(sizes):
    return np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)


def _random_values(rng, n, ranges):
    return np.stack([rng.integers(0, v, size=n) for v in ranges], 1).astype(np.int32)


def _collide_values(rng, sizes, T):
    """Values for the one-block ``collide`` case: in every partition the
    single-attribute columns cycle through the values whose keys hash into
    the last 8 slots of the 2048-slot table, so more keys are at home there
    than there are slots left and the probe must wrap to slot 0."""
    vals = _random_values(rng, int(np.sum(sizes)), RANGES3)
    e0 = 0
    for p, n in enumerate(sizes):
        for t, vr in enumerate(RANGES3):
            keys = (p * T + t) * VMAX + np.arange(vr)
            hot = np.flatnonzero(kr.pb_hash(keys) >= kr.PB_TBL - 8)
            if hot.size:
                vals[e0:e0 + n, t] = hot[np.arange(n) % hot.size]
        e0 += n
    return vals


@functools.lru_cache(maxsize=None)
def _case(name, NP):
    """(ent_part, ent_values, ranges, pairs, vmax, P) of a named case. A = 3
    with value ranges 12 / 31 / 400 and three unequal partitions, except the
    ``single_*`` cases: the kernels' item count is E * T, and with A = 3 no E
    gives exactly 1, 1024 or 1025 items, so those sizes use one attribute of
    range 400 (T = 1)."""
    rng = np.random.default_rng(len(name) * 131 + NP)
    pairs = PAIR if NP else []
    T = 3 + NP
    if name.startswith("single_"):
        assert NP == 0
        sizes = {"single_1": [1, 0, 0], "single_1024": [400, 399, 225],
                 "single_1025": [400, 399, 226]}[name]
        # distinct values inside each partition: every key of a block differs
        vals = np.concatenate([rng.permutation(400)[:n] for n in sizes])
        return (_parts(sizes), vals.reshape(-1, 1).astype(np.int32), (400,), [],
                VMAX, NUM_PARTS)
    if name == "tiny":          # E = 1: 3 or 4 items
        sizes = [0, 1, 0]
        vals = _random_values(rng, 1, RANGES3)
    elif name == "full_block":  # T = 4: exactly 1024 items; T = 3: 768
        sizes = [100, 90, 66]
        vals = _random_values(rng, 256, RANGES3)
    elif name == "past_block":  # T = 4: 1028 items; T = 3: 771
        sizes = [100, 90, 67]
        vals = _random_values(rng, 257, RANGES3)
    elif name == "popular":     # 5100 / 6800 items: last block partial
        sizes = [1100, 450, 150]
        vals = _random_values(rng, 1700, RANGES3)
        vals[:1100, 0] = 7      # block 0 = items 0..1023 of slot 0: one key
    elif name == "distinct":    # slot 2 is block 2 exactly; 1024 distinct keys
        sizes = [400, 390, 234]
        vals = _random_values(rng, 1024, RANGES3)
        vals[:, 2] = np.concatenate([rng.permutation(400)[:n] for n in sizes])
    elif name == "collide":     # one block holding every slot; 16 partitions
        # (three give too few keys per hash value for any probe to reach the
        # end of the table: 1329 valid keys over 2048 slots)
        sizes = list(range(8, 24))
        vals = _collide_values(rng, sizes, T)
    else:
        raise KeyError(name)
    return _parts(sizes), vals, RANGES3, pairs, VMAX, len(sizes)


CASES = [(n, NP) for n in ("tiny", "full_block", "past_block", "popular",
                           "distinct", "collide") for NP in (0, 1)]
CASES += [(n, 0) for n in ("single_1", "single_1024", "single_1025")]
CASE_IDS = [f"{n}-NP{NP}" for n, NP in CASES]


@functools.lru_cache(maxsize=None)
def _reference(name, NP):
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    return kr.index_reference(ent_part, vals, pairs, vmax, P)


@functools.lru_cache(maxsize=None)
def _records(name, NP, R=301):
    """Records over the same domain: a fifth of the values missing, so pair
    slots with either or both constituents missing occur; values drawn from
    the whole range, so many keys have no entity."""
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    rng = np.random.default_rng(99 + NP)
    rec_part = rng.integers(0, P, size=R).astype(np.int32)
    rv = _random_values(rng, R, ranges)
    rv[rng.random(rv.shape) < 0.2] = -1
    return rec_part, rv


def _pair_tensors(pairs):
    return tuple(_t([p[i] for p in pairs], torch.int32) for i in range(3))


def _block_keys(keys, block):
    return keys[block * kr.PB_THREADS:(block + 1) * kr.PB_THREADS]


# ---- the patterns are what they claim (runs without a GPU) -----------------------


def _check_pattern(name, NP):
    """The named case really has the block content it is there for. Called by
    the counting-pass tests, and for every case by the GPU-free test below."""
    keys = _reference(name, NP)[0]
    T = 3 + NP
    assert 12 * 31 <= VMAX  # the composite domain fits the Vmax that is passed
    if name == "popular":
        assert len(keys) == 1700 * T and len(keys) % kr.PB_THREADS != 0
        assert len(np.unique(_block_keys(keys, 0))) == 1        # one popular key
    elif name == "distinct":
        assert len(np.unique(_block_keys(keys, 2))) == 1024     # table at half load
    elif name == "collide":
        assert len(keys) <= kr.PB_THREADS                       # one block
        uk, home, final = kr.probe_table(keys)
        shared = np.bincount(home, minlength=kr.PB_TBL)
        assert (shared >= 2).any()                              # distinct keys, one hash
        wrapped = final < home                                  # went past slot 2047
        assert wrapped.any() and (home[wrapped] >= kr.PB_TBL - 8).all()
    elif name == "full_block" and NP:
        assert len(keys) == 1024
    elif name == "past_block" and NP:
        assert len(keys) == 1028
    elif name.startswith("single_"):
        n = int(name.split("_")[1])
        assert len(keys) == n and len(np.unique(keys)) == n


@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_index_case_patterns(name, NP):
    _check_pattern(name, NP)


# ---- counting passes -------------------------------------------------------------


@gpu
@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_postings_hist_matches_bincount(name, NP):
    _check_pattern(name, NP)
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    keys, counts_ref, ptr_ref, _ = _reference(name, NP)
    nk = len(counts_ref)
    a1, a2, v2 = _pair_tensors(pairs)
    part_t, vals_t = _t(ent_part, torch.int32), _t(vals, torch.int32)

    counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(part_t, vals_t, a1, a2, v2, vmax, counts)
    np.testing.assert_array_equal(counts.cpu().numpy(), counts_ref)

    # two calls on disjoint halves into one buffer == one call on all: the
    # contract the migration overlap's histogram prebuild relies on
    E = len(ent_part)
    h = E // 2
    both = torch.zeros(nk, dtype=torch.int32, device=DEV)
    for sl in (slice(0, h), slice(h, E)):
        C.postings_hist(part_t[sl].contiguous(), vals_t[sl].contiguous(),
                        a1, a2, v2, vmax, both)
    assert torch.equal(both, counts)


@gpu
@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_postings_scatter_matches_reference_sets(name, NP):
    _check_pattern(name, NP)
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    keys, counts_ref, ptr_ref, post_ref = _reference(name, NP)
    a1, a2, v2 = _pair_tensors(pairs)

    cursor = _t(ptr_ref[:-1], torch.int32)
    postings = torch.full((len(keys),), -7, dtype=torch.int32, device=DEV)
    C.postings_scatter(_t(ent_part, torch.int32), _t(vals, torch.int32),
                       a1, a2, v2, vmax, cursor, postings)
    # every key's segment holds exactly its entities (order inside a key is
    # unspecified); post_ref is ascending inside each key
    got = kr.sort_within_segments(postings.cpu().numpy(), ptr_ref)
    np.testing.assert_array_equal(got, post_ref)
    np.testing.assert_array_equal(cursor.cpu().numpy(), ptr_ref[1:])


@gpu
@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_stable_sort_route_matches_reference_order(name, NP):
    """build_ekeys_stable + the rocprim pair sort, called as the engine calls
    them: entities ascending inside each key, so an exact array compare."""
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    keys, counts_ref, ptr_ref, post_ref = _reference(name, NP)
    a1, a2, v2 = _pair_tensors(pairs)
    E, n, nk = len(ent_part), len(keys), len(counts_ref)

    ekeys = torch.full((n,), -7, dtype=torch.int64, device=DEV)
    C.build_ekeys_stable(_t(ent_part, torch.int32), _t(vals, torch.int32),
                         a1, a2, v2, vmax, ekeys)
    e_of_item = np.arange(n) % E
    np.testing.assert_array_equal(ekeys.cpu().numpy(), keys * E + e_of_item)

    keys_out = torch.empty(n, dtype=torch.int64, device=DEV)
    vals_in = (torch.arange(n, device=DEV, dtype=torch.int64) % E).to(torch.int32)
    postings = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    temp = torch.empty(int(C.radix_sort_pairs_temp_bytes(n)), dtype=torch.uint8,
                       device=DEV)
    end_bit = min(64, int(nk * E).bit_length())
    C.radix_sort_pairs_i64_i32(ekeys, keys_out, vals_in, postings, end_bit, temp)
    np.testing.assert_array_equal(postings.cpu().numpy(), post_ref)
    # segment boundaries are the same prefix
    seg_counts = np.bincount(keys_out.cpu().numpy() // E, minlength=nk)
    np.testing.assert_array_equal(seg_counts, counts_ref)


# ---- candidate ranges ------------------------------------------------------------


def _native_ranges(name, NP):
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    ptr_ref = _reference(name, NP)[2]
    rec_part, rv = _records(name, NP)
    R, T = rv.shape[0], rv.shape[1] + len(pairs)
    a1, a2, v2 = _pair_tensors(pairs)
    lo = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    hi = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    C.cand_ranges(_t(rec_part, torch.int32), _t(rv, torch.int32), a1, a2, v2,
                  _t(ptr_ref, torch.int64), vmax, lo, hi)
    return lo.cpu().numpy(), hi.cpu().numpy()


@gpu
@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_cand_ranges_match_prefix(name, NP):
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    ptr_ref = _reference(name, NP)[2]
    rec_part, rv = _records(name, NP)
    qk = kr.query_keys(rec_part, rv, pairs, vmax)       # -1 = missing slot
    obs = qk >= 0
    A = rv.shape[1]

    # the cases the check is about are present
    assert (~obs[:, :A]).any() and obs[:, :A].any()
    empty = obs & (ptr_ref[np.maximum(qk, 0) + 1] == ptr_ref[np.maximum(qk, 0)])
    assert (empty & (ptr_ref[np.maximum(qk, 0)] > 0)).any()   # no entity, offset > 0
    if NP:
        m1, m2 = rv[:, 0] < 0, rv[:, 1] < 0
        assert (m1 & ~m2).any() and (~m1 & m2).any() and (m1 & m2).any()
        assert obs[:, A].any()

    lo, hi = _native_ranges(name, NP)
    want_lo = np.where(obs, ptr_ref[np.maximum(qk, 0)], 0)
    want_hi = np.where(obs, ptr_ref[np.maximum(qk, 0) + 1], 0)
    np.testing.assert_array_equal(lo, want_lo)
    np.testing.assert_array_equal(hi, want_hi)


@gpu
@pytest.mark.parametrize("name,NP", CASES, ids=CASE_IDS)
def test_build_keys_route_matches_dense_route(name, NP):
    """The fallback for key spaces above 2^28 (build_keys + torch.sort +
    searchsorted, as the engine composes them) gives the keys of the formula,
    the ranges of cand_ranges on every observed slot and, per range, the
    entity set of the reference postings."""
    ent_part, vals, ranges, pairs, vmax, P = _case(name, NP)
    keys, counts_ref, ptr_ref, post_ref = _reference(name, NP)
    rec_part, rv = _records(name, NP)
    E, R, T = len(ent_part), rv.shape[0], rv.shape[1] + len(pairs)
    a1, a2, v2 = _pair_tensors(pairs)

    ekeys = torch.full((T * E,), -7, dtype=torch.int64, device=DEV)
    qkeys = torch.full((R * T,), -7, dtype=torch.int64, device=DEV)
    C.build_keys(_t(ent_part, torch.int32), _t(vals, torch.int32),
                 _t(rec_part, torch.int32), _t(rv, torch.int32), a1, a2, v2,
                 vmax, ekeys, qkeys)
    np.testing.assert_array_equal(ekeys.cpu().numpy(), keys)
    # a missing slot queries value 0 of its (partition, slot)
    sv = kr.slot_values(rv, pairs, missing_to=-1)
    qk_ref = ((rec_part.astype(np.int64)[:, None] * T + np.arange(T)[None, :]) * vmax
              + np.maximum(sv, 0))
    np.testing.assert_array_equal(qkeys.cpu().numpy().reshape(R, T), qk_ref)

    sorted_keys, perm = torch.sort(ekeys)
    post_fb = (perm % E).to(torch.int32).cpu().numpy()
    lo_fb = torch.searchsorted(sorted_keys, qkeys, right=False).view(R, T).cpu().numpy()
    hi_fb = torch.searchsorted(sorted_keys, qkeys, right=True).view(R, T).cpu().numpy()
    lo, hi = _native_ranges(name, NP)
    obs = sv >= 0
    np.testing.assert_array_equal(lo_fb[obs], lo[obs])
    np.testing.assert_array_equal(hi_fb[obs], hi[obs])
    np.testing.assert_array_equal(kr.sort_within_segments(post_fb, ptr_ref), post_ref)


# ---- routing ---------------------------------------------------------------------


def _classify_inputs(NP):
    """600 records with A = 3 over three partitions whose pools are the heavy
    threshold, one above it, and 5; attribute states and range sizes drawn so
    every branch of the rule is met (asserted by the caller)."""
    A, T = 3, 3 + NP
    small, heavy = 16, 512
    rng = np.random.default_rng(4 + NP)
    R = 600
    ent_ptr = np.array([0, heavy, 2 * heavy + 1, 2 * heavy + 6], dtype=np.int64)
    rec_part = rng.integers(0, 3, size=R).astype(np.int32)
    state = rng.integers(0, 3, size=(R, A))       # 0 nd, 1 distorted, 2 missing
    state[:60] = 1                                 # no non-distorted attribute
    state[40:60, 1] = 2
    rv = rng.integers(0, 12, size=(R, A)).astype(np.int32)
    rv[state == 2] = -1
    rd = (state == 1).astype(np.uint8)
    sizes = np.array([0, small - 1, small, small + 1, heavy - 1, heavy, heavy + 1, 4000])
    n = sizes[rng.integers(0, len(sizes), size=(R, T))]
    lo = rng.integers(0, 10000, size=(R, T)).astype(np.int64)
    return rv, rd, rec_part, ent_ptr, lo, lo + n, small, heavy


@gpu
@pytest.mark.parametrize("NP", [0, 1])
@pytest.mark.parametrize("heavy_on", [True, False])
def test_classify_modes_matches_rule(NP, heavy_on):
    rv, rd, rec_part, ent_ptr, lo, hi, small, heavy = _classify_inputs(NP)
    A = rv.shape[1]
    nd = (rv >= 0) & (rd == 0)
    n_single = np.where(nd, (hi - lo)[:, :A], np.iinfo(np.int64).max)
    best = n_single.min(1)
    nd_count = nd.sum(1)
    pool = (ent_ptr[1:] - ent_ptr[:-1])[rec_part]
    # coverage of the rule's edges
    assert {0, 1, 2} <= set(nd_count.tolist())
    assert (rv < 0).any()
    for edge in (small, small + 1):
        assert ((nd_count >= 1) & (best == edge)).any()
    for edge in (heavy, heavy + 1):
        assert ((nd_count == 1) & (best == edge)).any()
        assert ((nd_count == 0) & (pool == edge)).any()

    th = heavy if heavy_on else 0
    want = kr.classify_modes_reference(rv, rd, rec_part, ent_ptr, lo, hi, small, th)
    assert set(want.tolist()) == ({0, 1, 2} if heavy_on else {0, 1})
    mode = torch.full((len(rv),), 9, dtype=torch.uint8, device=DEV)
    C.classify_modes(_t(rv, torch.int32), _t(rd, torch.uint8),
                     _t(rec_part, torch.int32), _t(ent_ptr, torch.int64),
                     _t(lo, torch.int64), _t(hi, torch.int64), NP, small, th, mode)
    np.testing.assert_array_equal(mode.cpu().numpy(), want)


# ---- pair slots and the sort route change no draw ----------------------------------


def _pair_slot_inputs(cache, R=512, E=1500):
    """Entities and records over the bench schema (by, bm, bd constant; two
    Levenshtein names) in two partitions. Records copy an entity of their own
    partition, then:
      kind 0  constants held, both names distorted      (4 in 10)
      kind 1  everything held                           (1 in 10)
      kind 2  'by' distorted, names distorted           (2 in 10)
      kind 3  'bm' missing, names distorted             (2 in 10)
      kind 4  every attribute distorted                 (1 in 10)
    Distorted names take a random other value, so the od log-weight is real."""
    rng = np.random.default_rng(21)
    n_vals = [ia.index.num_values for ia in cache.indexed_attributes]
    ent_values = _random_values(rng, E, n_vals)
    ent_part = _parts([900, 600])
    src = rng.integers(0, E, size=R)
    rv = ent_values[src].copy()
    rd = np.zeros_like(rv, dtype=np.uint8)
    kind = np.array([0, 0, 0, 0, 1, 2, 2, 3, 3, 4])[np.arange(R) % 10]
    names = kind != 1
    for a in (3, 4):
        rd[names, a] = 1
        rv[names, a] = rng.integers(0, n_vals[a], size=names.sum())
    k2, k3, k4 = kind == 2, kind == 3, kind == 4
    rd[k2, 0] = 1
    rv[k2, 0] = rng.integers(0, n_vals[0], size=k2.sum())
    rv[k3, 1] = -1
    rd[k4, :3] = 1
    return ent_part, ent_values, ent_part[src].copy(), rv, rd, kind, n_vals


def _const_pairs(n_vals):
    """The engine's DBLINK_CONST_PAIRS=1 slots for constants 0, 1, 2."""
    return [(a1, a2, n_vals[a2]) for a1, a2 in ((0, 1), (0, 2), (1, 2))]


@gpu
def test_link_update_pair_slots_change_no_draw():
    """512 records through link_update over an index built by the native ops,
    once with the three constant-pair slots and once without; same seed and
    iteration. Outputs must be torch.equal."""
    from test_gpu_sweep_glue import _data
    from dblink_amd.engine.gpu_engine import GpuModel

    cache = _data(2000)[0]
    model = GpuModel(cache, DEV, 1)
    ent_part, ent_values, rec_part, rv, rd, kind, n_vals = _pair_slot_inputs(cache)
    E, R, A = len(ent_part), len(rv), rv.shape[1]
    pairs3 = _const_pairs(n_vals)
    assert max(n_vals[a1] * v2 for a1, _, v2 in pairs3) <= 65536  # engine's cap
    ent_ptr = np.array([0, 900, E], dtype=np.int64)

    # not vacuous: at least a quarter of the records enumerate a pair base
    vmax3 = max(max(n_vals), max(n_vals[a1] * v2 for a1, _, v2 in pairs3))
    ptr3 = kr.index_reference(ent_part, ent_values, pairs3, vmax3, 2)[2]
    qk = kr.query_keys(rec_part, rv, pairs3, vmax3)
    size = np.where(qk >= 0, ptr3[np.maximum(qk, 0) + 1] - ptr3[np.maximum(qk, 0)],
                    np.iinfo(np.int64).max)
    nd = (rv >= 0) & (rd == 0)
    big = np.iinfo(np.int64).max
    single = np.where(nd, size[:, :A], big).min(1)
    pair_ok = np.stack([nd[:, a1] & nd[:, a2] for a1, a2, _ in pairs3], 1)
    pair = np.where(pair_ok, size[:, A:], big).min(1)
    assert (pair < single).sum() >= R // 4, (pair < single).sum()
    assert set(kind.tolist()) == {0, 1, 2, 3, 4}
    assert (nd.sum(1) == 0).any()

    tensors = dict(
        part=_t(ent_part, torch.int32), vals=_t(ent_values, torch.int32),
        rpart=_t(rec_part, torch.int32), rv=_t(rv, torch.int32),
        rd=_t(rd, torch.uint8), gid=_t(np.arange(R) + 1000, torch.int64),
        ent_ptr=_t(ent_ptr, torch.int64),
        rec_ent_in=torch.zeros(R, dtype=torch.int64, device=DEV))

    def run(pairs):
        t = tensors
        T = A + len(pairs)
        vmax = max([max(n_vals)] + [n_vals[a1] * v2 for a1, _, v2 in pairs])
        nk = 2 * T * vmax
        a1, a2, v2 = _pair_tensors(pairs)
        counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
        C.postings_hist(t["part"], t["vals"], a1, a2, v2, vmax, counts)
        ptr = torch.zeros(nk + 1, dtype=torch.int64, device=DEV)
        torch.cumsum(counts, 0, dtype=torch.int64, out=ptr[1:])
        cursor = ptr[:-1].to(torch.int32)
        postings = torch.empty(T * E, dtype=torch.int32, device=DEV)
        C.postings_scatter(t["part"], t["vals"], a1, a2, v2, vmax, cursor, postings)
        lo = torch.empty((R, T), dtype=torch.int64, device=DEV)
        hi = torch.empty((R, T), dtype=torch.int64, device=DEV)
        C.cand_ranges(t["rpart"], t["rv"], a1, a2, v2, ptr, vmax, lo, hi)
        out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        C.link_update(t["rv"], t["rd"], t["gid"], t["rpart"], lo, hi, postings,
                      t["vals"], t["ent_ptr"], model.log_norm, model.voff,
                      model.csr_row_ptr, model.csr_col, model.csr_sim,
                      model.attr_const, 9001, 13, out, t["rec_ent_in"], err,
                      torch.empty(0, dtype=torch.uint8, device=DEV),
                      torch.empty(0, dtype=torch.int64, device=DEV), a1, a2)
        assert int(err.cpu()) == 0
        return out

    with_pairs = run(pairs3)
    without = run([])
    assert torch.equal(with_pairs, without)
    sel = with_pairs.cpu().numpy()
    # every draw is a legal candidate of the record's own partition
    assert ((sel >= ent_ptr[rec_part]) & (sel < ent_ptr[rec_part + 1])).all()
    assert ((ent_values[sel] == rv) | ~nd).all()


def _chain(monkeypatch, graphs, env=None):
    from test_gpu_sweep_glue import _run_chain

    for k in ("DBLINK_CONST_PAIRS", "DBLINK_FORCE_SORT"):
        monkeypatch.delenv(k, raising=False)
    if env:
        monkeypatch.setenv(env, "1")
    return _run_chain(monkeypatch, True, graphs, "PCG-I", levels=2, n=2000,
                      sweeps=20)


@gpu
def test_chain_equal_with_const_pairs(monkeypatch):
    from test_gpu_sweep_glue import _assert_chains_equal

    plain = _chain(monkeypatch, True)
    paired = _chain(monkeypatch, True, "DBLINK_CONST_PAIRS")
    assert plain[0]._num_pairs == 0 and paired[0]._num_pairs == 3
    _assert_chains_equal(plain, paired)


@gpu
def test_chain_equal_on_stable_sort_route(monkeypatch):
    """Graphs off: the engine never replays the sort route from a graph (heavy
    routing switches graphs off)."""
    from test_gpu_sweep_glue import _assert_chains_equal

    plain = _chain(monkeypatch, False)
    sorted_route = _chain(monkeypatch, False, "DBLINK_FORCE_SORT")
    _assert_chains_equal(plain, sorted_route)
