"""The split path of the indexed link update (``link_update_split``).

Records whose base candidate list is longer than the split length S leave the
wave-per-record kernel for a device-side list, and ``link_update_split_kernel``
gives each listed record a whole block. Routing is a performance decision, so
the draws must not move: split on, split off and split on with the sim rows
read from global memory (``DBLINK_SIMH=0``) must be ``torch.equal``, and all
of them must agree with the thread kernel (``mode_mask`` all ones), which
walks the same lists serially.

The state is built by hand over the bench schema (by, bm, bd constant; two
Levenshtein names): partitions of S-1, S, S+1, 2S+1, 5 and 2500 entities, in
each of them records without any non-distorted attribute and with 0, 1 and 2
observed distorted names (the whole partition is their base list), and in the
big one records whose base is a posting list longer than S and one record for
which no candidate survives the equality check.

An exact f32 tie between two candidates cannot be forced by a cheap test, so
the tie order of the split kernel (the comment above ``link_split_better`` in
``kernels.hip``) is checked by reading, not here.

The last tests run whole chains with ``DBLINK_LINK_SPLIT`` and
``DBLINK_VALUE_LISTS`` both on and both off.
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

S = 256                                   # the engine's default split length
SIZES = [S - 1, S, S + 1, 2 * S + 1, 5, 2500]
BIG = len(SIZES) - 1
SPLIT_PARTS = (2, 3, BIG)                 # partitions longer than S
GRID = 2                                  # fewer blocks than listed records


def _t(arr, dtype):
    return torch.as_tensor(np.ascontiguousarray(arr)).to(dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _state():
    from test_gpu_sweep_glue import _data

    cache = _data(2000)[0]
    n_vals = [ia.index.num_values for ia in cache.indexed_attributes]
    assert len(n_vals) == 5 and n_vals[1] >= 3 and n_vals[2] >= 6
    rng = np.random.default_rng(5)
    ent_part = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int32)
    E = len(ent_part)
    ent_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    ent_values = np.stack([rng.integers(0, v, size=E) for v in n_vals], 1).astype(np.int32)
    # big partition: bm takes three values (posting lists of ~833 entities);
    # bd is 5 exactly where bm is 1, so the lists (bm = 0) and (bd = 5) are
    # both long and disjoint
    big = np.arange(ent_ptr[BIG], ent_ptr[BIG + 1])
    ent_values[big, 1] = np.arange(len(big)) % 3
    ent_values[big, 2] = np.where(ent_values[big, 1] == 1, 5,
                                  rng.integers(0, 5, size=len(big)))

    rows = []  # (partition, values, dist, kind)

    def add(p, kind):
        src = int(rng.integers(ent_ptr[p], ent_ptr[p + 1]))
        v = ent_values[src].copy()
        d = np.zeros(5, dtype=np.uint8)
        if kind in ("z0", "z1", "z2"):     # nothing held: the whole partition
            d[:] = 1
            v[3:] = rng.integers(0, [n_vals[3], n_vals[4]])
            if kind == "z0":
                v[3:] = -1                 # no observed name: pure Gumbel draw
            elif kind == "z1":
                v[4] = -1
        elif kind == "post":               # only bm held: a posting base > S
            d[[0, 2, 3, 4]] = 1
            v[3:] = rng.integers(0, [n_vals[3], n_vals[4]])
        elif kind == "none":               # bm = 0 and bd = 5 held: disjoint
            d[[0, 3, 4]] = 1
            v[1], v[2] = 0, 5
        elif kind == "two":                # by and bm held: a shorter base
            d[[2, 3, 4]] = 1
        else:
            assert kind == "held"          # everything held: a short name list
        rows.append((p, v, d, kind))

    for p in range(len(SIZES)):
        for kind in ("z0", "z1", "z2", "z0", "z1", "z2", "held", "held", "held"):
            add(p, kind)
    for _ in range(6):
        add(BIG, "post")
    for _ in range(4):
        add(BIG, "two")
    add(BIG, "none")
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rec_part = np.array([r[0] for r in rows], dtype=np.int32)
    rv = np.stack([r[1] for r in rows]).astype(np.int32)
    rd = np.stack([r[2] for r in rows]).astype(np.uint8)
    kind = np.array([r[3] for r in rows])
    return cache, n_vals, ent_part, ent_ptr, ent_values, rec_part, rv, rd, kind


def _base_lengths(state):
    """Base-list length per record by the rule of ``link_select_base``."""
    _, n_vals, ent_part, ent_ptr, ent_values, rec_part, rv, rd, _ = state
    vmax = max(n_vals)
    ptr = kr.index_reference(ent_part, ent_values, [], vmax, len(SIZES))[2]
    qk = kr.query_keys(rec_part, rv, [], vmax)
    size = ptr[np.maximum(qk, 0) + 1] - ptr[np.maximum(qk, 0)]
    nd = (rv >= 0) & (rd == 0)
    n = np.where(nd, size, np.iinfo(np.int64).max).min(1)
    pool = ent_ptr[rec_part.astype(np.int64) + 1] - ent_ptr[rec_part]
    return np.where(nd.any(1), n, pool), nd


def _precheck(state):
    """The cases reach the paths they are there for. Returns the split mask."""
    rec_part, kind = state[5], state[8]
    n, nd = _base_lengths(state)
    split = n > S
    R = len(rec_part)
    assert R % 4 != 0
    whole = np.isin(kind, ["z0", "z1", "z2"])
    assert not nd[whole].any()
    for p, size in enumerate(SIZES):       # S-1 and S stay, S+1 and up leave
        assert (n[whole & (rec_part == p)] == size).all()
        assert split[whole & (rec_part == p)].all() == (size > S)
        assert (whole & (rec_part == p)).sum() == 6
    assert not split[whole & np.isin(rec_part, [0, 1, 4])].any()
    assert split[kind == "post"].all() and (kind == "post").sum() == 6
    assert split[kind == "none"].all() and (kind == "none").sum() == 1
    assert not split[kind == "held"].any()
    # both base kinds among the listed records, and more of them than blocks
    assert split.sum() == 6 * len(SPLIT_PARTS) + 6 + 1 + (split & (kind == "two")).sum()
    assert (split & nd.any(1)).sum() >= 7 and (split & ~nd.any(1)).sum() == 18
    assert split.sum() > GRID
    for k in ("z0", "z1", "z2"):           # 0, 1 and 2 observed distorted names
        assert (split & (kind == k)).sum() == 6
    return split


def test_split_cases_reach_their_paths():
    _precheck(_state())


def _wave_argmax_lane(scores):
    """Transcription of ``wave_argmax`` (common.h): the lane whose value lane
    0 holds after the shfl_down tree; a lane keeps its own value unless the
    other one is strictly larger."""
    s, lane = list(scores), list(range(64))
    off = 32
    while off:
        ns, nl = s[:], lane[:]
        for i in range(64 - off):          # past the wave end a lane reads itself
            if s[i + off] > s[i]:
                ns[i], nl[i] = s[i + off], lane[i + off]
        s, lane, off = ns, nl, off // 2
    return lane[0]


def test_tie_order_of_the_shuffle_tree():
    """The order ``link_split_better`` applies among equal scores (lower
    bit-reversed lane first) is the one ``wave_argmax``'s tree produces, here
    on transcriptions of both; the kernels themselves are compared by reading
    (no cheap test forces an f32 tie)."""
    rng = np.random.default_rng(0)
    brev6 = lambda x: int(format(x, "06b")[::-1], 2)
    for _ in range(2000):
        scores = rng.integers(0, 3, size=64).tolist()
        top = rng.choice(64, size=rng.integers(1, 7), replace=False).tolist()
        for i in top:
            scores[i] = 5
        assert _wave_argmax_lane(scores) == min(top, key=brev6)


def _run(state, model, split_len, mask_all_ones=False, grid=GRID):
    _, n_vals, ent_part, ent_ptr, ent_values, rec_part, rv, rd, _ = state
    E, R, A = len(ent_part), len(rv), 5
    vmax, P = max(n_vals), len(SIZES)
    nk = P * A * vmax
    none32 = torch.empty(0, dtype=torch.int32, device=DEV)
    part_t, vals_t = _t(ent_part, torch.int32), _t(ent_values, torch.int32)
    rpart_t, rv_t = _t(rec_part, torch.int32), _t(rv, torch.int32)
    counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(part_t, vals_t, none32, none32, none32, vmax, counts)
    ptr = torch.zeros(nk + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, dtype=torch.int64, out=ptr[1:])
    cursor = ptr[:-1].to(torch.int32)
    postings = torch.empty(A * E, dtype=torch.int32, device=DEV)
    C.postings_scatter(part_t, vals_t, none32, none32, none32, vmax, cursor, postings)
    lo = torch.empty((R, A), dtype=torch.int64, device=DEV)
    hi = torch.empty((R, A), dtype=torch.int64, device=DEV)
    C.cand_ranges(rpart_t, rv_t, none32, none32, none32, ptr, vmax, lo, hi)
    out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    # every record starts on the first entity of its partition
    rec_ent_in = _t(ent_ptr[rec_part], torch.int64)
    mask = (torch.ones(R, dtype=torch.uint8, device=DEV) if mask_all_ones
            else torch.empty(0, dtype=torch.uint8, device=DEV))
    split_list = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    split_count = torch.zeros(1, dtype=torch.int32, device=DEV)
    C.link_update_split(rv_t, _t(rd, torch.uint8), _t(np.arange(R) + 1000, torch.int64),
                        rpart_t, lo, hi, postings, vals_t, _t(ent_ptr, torch.int64),
                        model.log_norm, model.voff, model.csr_row_ptr, model.csr_col,
                        model.csr_sim, model.attr_const, 9001, 13, out, rec_ent_in, err,
                        mask, torch.empty(0, dtype=torch.int64, device=DEV),
                        none32, none32, split_list, split_count, split_len, grid)
    n_listed = int(split_count.cpu())
    listed = set(split_list[:n_listed].cpu().tolist())
    assert len(listed) == n_listed
    return out, int(err.cpu()), listed


@gpu
def test_split_path_changes_no_draw(monkeypatch):
    from dblink_amd.engine.gpu_engine import GpuModel

    state = _state()
    split = _precheck(state)
    model = GpuModel(state[0], DEV, 1)
    ent_ptr, ent_values, rec_part, rv, rd, kind = state[3:]
    monkeypatch.delenv("DBLINK_SIMH", raising=False)

    on, err_on, listed = _run(state, model, S)
    off, err_off, listed_off = _run(state, model, 0)
    wide, err_wide, _ = _run(state, model, S, grid=64)   # a block per record
    thread, err_thread, listed_thread = _run(state, model, S, mask_all_ones=True)
    monkeypatch.setenv("DBLINK_SIMH", "0")  # re-read per launch; restored on exit
    on_global, err_global, _ = _run(state, model, S)

    # the list is the records the rule names, each once; the other paths list none
    assert listed == set(np.flatnonzero(split).tolist())
    assert listed_off == set() and listed_thread == set()

    assert torch.equal(on, off)
    assert torch.equal(on, wide)
    assert torch.equal(on, on_global)
    # the one record without a surviving candidate keeps its link and is counted
    none = np.flatnonzero(kind == "none")
    assert err_on == err_off == err_wide == err_global == 1
    sel = on.cpu().numpy()
    assert sel[none[0]] == ent_ptr[rec_part[none[0]]]
    others = torch.as_tensor(np.flatnonzero(kind != "none"), device=DEV)
    assert torch.equal(on[others], thread[others])
    assert err_thread == 1

    # every other draw is a legal candidate of the record's own partition
    ok = kind != "none"
    nd = (rv >= 0) & (rd == 0)
    assert ((sel >= ent_ptr[rec_part]) & (sel < ent_ptr[rec_part.astype(np.int64) + 1])).all()
    assert ((ent_values[sel] == rv) | ~nd)[ok].all()
    # and the draws of one partition-sized list are not all one entity
    assert len(set(sel[split & ok].tolist())) > 10


# ---- whole chains ----------------------------------------------------------------


def _run_chain(monkeypatch, on, graphs, sampler):
    """2000 records, 4 partitions, 40 sweeps with both routing switches of the
    link tail and the value lists on or off."""
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner
    from test_gpu_sweep_glue import _data

    for k in ("DBLINK_LINK_SPLIT", "DBLINK_VALUE_LISTS"):
        monkeypatch.setenv(k, "1" if on else "0")
    # 40 sweeps from the initial state stay early in the chain, where base
    # lists are short (about 60 records a sweep above 8 entries, none above
    # 64, counted on the CPU engine): a split length of 8 and 16 blocks put
    # records on the split path every sweep, more of them than blocks
    monkeypatch.setenv("DBLINK_LINK_SPLIT_LEN", "8")
    monkeypatch.setenv("DBLINK_LINK_SPLIT_GRID", "16")
    monkeypatch.delenv("DBLINK_FUSED_GLUE", raising=False)
    monkeypatch.setenv("DBLINK_GRAPHS", "1" if graphs else "0")
    n = 2000
    cache, rec_values, rec_files = _data(n)
    partitioner = KDTreePartitioner(2, [3, 4])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=7)
    engine = GpuEngine(cache, partitioner, device=DEV)
    assert (engine._split_len > 0) == on and engine._vlists == on
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(sampler)
    series, listed, vlisted = [], 0, 0
    for _ in range(40):
        engine.step(state, flags)
        series.append((state.summary.log_likelihood, state.summary.num_isolates,
                       state.summary.agg_distortions.copy()))
        listed += int(engine._split_cnt.cpu())
        vlisted += int(engine._vlist_cnt.sum().cpu())
    if graphs:
        assert len(engine._graphs) == 2
    engine.sync_state(state)
    return state, series, int(engine._err.cpu()), listed, vlisted


@gpu
@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("sampler", ["PCG-I", "Gibbs"])
def test_chain_equal_with_and_without_split_and_lists(monkeypatch, sampler, graphs):
    sa, ser_a, err_a, listed_a, vlisted_a = _run_chain(monkeypatch, True, graphs, sampler)
    sb, ser_b, err_b, listed_b, vlisted_b = _run_chain(monkeypatch, False, graphs, sampler)
    # the split path served records and the value lists held pairs
    assert listed_a > 40 * 16 and listed_b == 0
    assert vlisted_a > 0 and vlisted_b == 0
    for f in ("rec_ent", "ent_values", "ent_part", "rec_dist"):
        assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
    for k, (a, b) in enumerate(zip(ser_a, ser_b)):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), k
    assert err_a == err_b == 0
