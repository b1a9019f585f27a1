"""The co-launched sweep kernels against the launches they replace.

``kernels.hip`` routes whole blocks of independent kernels by block index:
``sweep_begin`` (posting histogram + counter fill + staging copy),
``postings_scatter_ranges_split`` (scatter + ranges + the link split list),
``link_update_merged`` (split and wave blocks), the re-sort scatter's scan
prologue (``DBLINK_RESORT_SCAN``) and ``sweep_tail`` (re-sort + summary in
three launches). Every output is an integer array or a sum taken in a fixed order,
so each comparison is ``torch.equal`` against the launches replaced; the chain
tests run whole engines with each new switch off in turn.

The link state is ``test_gpu_link_split``'s generator run nine times over
(about 600 records). That file has no precheck that f32 ties occur (it says an
exact tie cannot be forced cheaply); the tie order is held here by comparing
with the wave-only ``link_update``, whose order is the specification.
"""

import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_link_split as ls  # noqa: E402
from test_gpu_sweep_glue import (_assert_chains_equal, _data, _flat_tree,  # noqa: E402
                                 _i32, _i64)
from test_gpu_sweep_launches import _index_case  # noqa: E402

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)


def _u8(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.uint8).to(DEV)


# ---- sweep_begin -------------------------------------------------------------------


@gpu
def test_sweep_begin_matches_hist_fill_and_copy():
    rng = np.random.default_rng(3)
    E, P, A = 1500, 3, 3
    V = [40, 12, 28]
    ent_values = _i32(np.stack([rng.integers(0, v, size=E) for v in V], axis=1))
    ent_part = _i32(np.sort(rng.integers(0, P, size=E)))
    a1, a2, v2 = _i32([0]), _i32([1]), _i32([V[1]])
    vmax = V[0] * V[1]
    nk = P * (A + 1) * vmax
    ref = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(ent_part, ent_values, a1, a2, v2, vmax, ref)
    assert int(ref.sum()) == E * (A + 1)

    # 4099 words: more than one zeroing block and a ragged last thread
    words = rng.integers(1, 1 << 30, size=(16 + 4 * A * 2) // 4)
    pin = torch.zeros(16 + 4 * A * 2, dtype=torch.uint8, pin_memory=True)
    pin.view(torch.int32).copy_(torch.as_tensor(words, dtype=torch.int32))
    for n_blk, offset in [(4099, 0), (4099, 1), (3, 0)]:
        counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
        stage = torch.full((pin.numel(),), 0xAB, dtype=torch.uint8, device=DEV)
        for _ in range(2):  # nothing accumulates but the histogram itself
            counts.zero_()
            blk = torch.full((n_blk + offset,), -7, dtype=torch.int32, device=DEV)[offset:]
            C.sweep_begin(ent_part, ent_values, a1, a2, v2, vmax, counts, blk, pin, stage)
            assert torch.equal(counts, ref)
            assert not blk.any()
            assert torch.equal(stage.cpu(), pin)


# ---- ranges + split list ----------------------------------------------------------


def _base_len(c, lo, hi, rec_dist, ent_ptr):
    """Base-list length per record by the rule of ``link_select_base``."""
    rv = c["rec_values"].cpu().numpy()
    A = rv.shape[1]
    size = (hi - lo).cpu().numpy()
    nd = (rv >= 0) & (rec_dist == 0)
    big = np.iinfo(np.int64).max
    n = np.where(nd, size[:, :A], big).min(1)
    a1, a2 = c["a1"].cpu().numpy(), c["a2"].cpu().numpy()
    for t in range(len(a1)):
        both = nd[:, a1[t]] & nd[:, a2[t]]
        n = np.minimum(n, np.where(both, size[:, A + t], big))
    part = c["rec_part"].cpu().numpy().astype(np.int64)
    pool = ent_ptr[part + 1] - ent_ptr[part]
    return np.where(nd.any(1), n, pool), nd


@gpu
@pytest.mark.parametrize("name", ["plain", "pair_and_missing", "ragged",
                                  "single_record", "fewer_records", "more_records"])
def test_ranges_and_split_list(name):
    c = _index_case(name)
    E, R, T, nk = c["ent_values"].shape[0], c["rec_values"].shape[0], c["T"], c["nk"]
    A, P = 5, 4
    pair = (c["a1"], c["a2"], c["v2"], c["vmax"])
    rng = np.random.default_rng(R)
    rec_dist = (rng.random((R, A)) < 0.5).astype(np.uint8)
    rec_dist[::7] = 1  # no non-distorted attribute: the partition is the base
    attr_const = _u8([1, 1, 1, 0, 0])
    ent_ptr = np.searchsorted(c["ent_part"].cpu().numpy(), np.arange(P + 1)).astype(np.int64)

    counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(c["ent_part"], c["ent_values"], *pair, counts)
    ptr = torch.empty(nk + 1, dtype=torch.int64, device=DEV)
    cursor = torch.empty(nk, dtype=torch.int32, device=DEV)
    C.scan_excl(counts, ptr, cursor)
    lo_ref = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    hi_ref = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    C.cand_ranges(c["rec_part"], c["rec_values"], *pair[:3], ptr, c["vmax"],
                  lo_ref, hi_ref)
    post_ref = torch.full((E * T,), -7, dtype=torch.int32, device=DEV)
    C.postings_scatter(c["ent_part"], c["ent_values"], *pair, cursor.clone(), post_ref)
    n, nd = _base_len(c, lo_ref, hi_ref, rec_dist, ent_ptr)
    assert (~nd.any(1)).any()
    if name == "pair_and_missing":
        assert (c["rec_values"].cpu().numpy() < 0).any()

    huge = int(n.max())
    # the intended list sizes: every nonempty base, some of them, none
    assert (n > 0).sum() > 0 and (n > huge).sum() == 0
    if R > 1:
        assert 0 < (n > 8).sum() < (n > 0).sum() <= R
    for split_len, want in [(0, n > 0), (8, n > 8), (huge, n > huge)]:
        post = torch.full((E * T,), -7, dtype=torch.int32, device=DEV)
        lo = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
        hi = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
        cur = cursor.clone()
        lst = torch.full((R,), -1, dtype=torch.int32, device=DEV)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
        C.postings_scatter_ranges_split(
            c["ent_part"], c["ent_values"], c["rec_part"], c["rec_values"], *pair,
            cur, ptr, post, lo, hi, _u8(rec_dist), attr_const, _i64(ent_ptr), lst,
            cnt, split_len)
        assert torch.equal(lo, lo_ref)
        assert torch.equal(hi, hi_ref)
        assert torch.equal(cur.to(torch.int64), ptr[1:])
        seg = torch.repeat_interleave(torch.arange(nk, device=DEV), (ptr[1:] - ptr[:-1]))
        key_of = seg.to(torch.int64) * E
        assert torch.equal(torch.sort(key_of + post)[0], torch.sort(key_of + post_ref)[0])
        k = int(cnt.cpu())
        listed = np.sort(lst[:k].cpu().numpy())
        assert np.array_equal(listed, np.flatnonzero(want))
        assert (lst[k:] == -1).all()


# ---- link in one launch ------------------------------------------------------------

REPS = 9


def _link_state():
    """test_gpu_link_split's state with its records repeated REPS times (own
    gids, so own draws): partition-sized and long posting base lists."""
    st = ls._state()
    ls._precheck(st)
    cache, n_vals, ent_part, ent_ptr, ent_values, rec_part, rv, rd, kind = st
    return (cache, n_vals, ent_part, ent_ptr, ent_values, np.tile(rec_part, REPS),
            np.tile(rv, (REPS, 1)), np.tile(rd, (REPS, 1)), np.tile(kind, REPS))


def _link_run(state, model, split_len, op, grid=2, force_empty=False):
    _, n_vals, ent_part, ent_ptr, ent_values, rec_part, rv, rd, _ = state
    E, R, A = len(ent_part), len(rv), 5
    vmax, P = max(n_vals), len(ls.SIZES)
    nk = P * A * vmax
    none32 = torch.empty(0, dtype=torch.int32, device=DEV)
    t = ls._t
    part_t, vals_t = t(ent_part, torch.int32), t(ent_values, torch.int32)
    rpart_t, rv_t, rd_t = t(rec_part, torch.int32), t(rv, torch.int32), t(rd, torch.uint8)
    ent_ptr_t = t(ent_ptr, torch.int64)
    counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(part_t, vals_t, none32, none32, none32, vmax, counts)
    ptr = torch.empty(nk + 1, dtype=torch.int64, device=DEV)
    cursor = torch.empty(nk, dtype=torch.int32, device=DEV)
    C.scan_excl(counts, ptr, cursor)
    postings = torch.empty(A * E, dtype=torch.int32, device=DEV)
    lo = torch.empty((R, A), dtype=torch.int64, device=DEV)
    hi = torch.empty((R, A), dtype=torch.int64, device=DEV)
    lst = torch.full((R,), -1, dtype=torch.int32, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    rec_ent_in = t(ent_ptr[rec_part], torch.int64)
    gid = t(np.arange(R) + 1000, torch.int64)
    ctrl = torch.empty(0, dtype=torch.int64, device=DEV)
    link = (rv_t, rd_t, gid, rpart_t, lo, hi, postings, vals_t, ent_ptr_t,
            model.log_norm, model.voff, model.csr_row_ptr, model.csr_col,
            model.csr_sim, model.attr_const, 9001, 13, out, rec_ent_in, err)
    if op == "merged":
        C.postings_scatter_ranges_split(
            part_t, vals_t, rpart_t, rv_t, none32, none32, none32, vmax, cursor, ptr,
            postings, lo, hi, rd_t, model.attr_const, ent_ptr_t, lst, cnt, split_len)
        C.link_update_merged(*link, ctrl, none32, none32, lst, cnt, split_len, grid)
    else:
        C.postings_scatter_ranges(part_t, vals_t, rpart_t, rv_t, none32, none32,
                                  none32, vmax, cursor, ptr, postings, lo, hi)
        mask = torch.empty(0, dtype=torch.uint8, device=DEV)
        if op == "split":
            C.link_update_split(*link, mask, ctrl, none32, none32, lst, cnt,
                                split_len, grid)
        else:
            C.link_update(*link, mask, ctrl, none32, none32)
    k = int(cnt.cpu())
    return out, int(err.cpu()), set(lst[:k].cpu().tolist())


@gpu
@pytest.mark.parametrize("split_len", [4, 64])
def test_link_in_one_launch_changes_no_draw(monkeypatch, split_len):
    from dblink_amd.engine.gpu_engine import GpuModel

    monkeypatch.delenv("DBLINK_SIMH", raising=False)
    state = _link_state()
    R = len(state[5])
    assert 550 < R < 650 and R % 16 != 0
    model = GpuModel(state[0], DEV, 1)
    merged, err_m, listed_m = _link_run(state, model, split_len, "merged")
    split, err_s, listed_s = _link_run(state, model, split_len, "split")
    wave, err_w, _ = _link_run(state, model, 0, "wave")
    assert listed_m == listed_s and len(listed_m) > 2  # the stride serves the list
    assert torch.equal(merged, split)
    assert torch.equal(merged, wave)
    assert err_m == err_s == err_w == REPS  # the "none" records, each counted once


@gpu
def test_link_in_one_launch_with_an_empty_list():
    from dblink_amd.engine.gpu_engine import GpuModel

    state = _link_state()
    model = GpuModel(state[0], DEV, 1)
    merged, err_m, listed = _link_run(state, model, 1 << 20, "merged")
    wave, err_w, _ = _link_run(state, model, 0, "wave")
    assert listed == set()
    assert torch.equal(merged, wave) and err_m == err_w


# ---- re-sort prologue and tail op --------------------------------------------------


def _tail(E, P, R, merged, A=3, F=2):
    """All outputs of the sweep tail: partition_resort + summary_counts, or
    sweep_tail."""
    rng = np.random.default_rng(E + P)
    ent_values = _i32(rng.integers(0, 256, size=(E, A)))
    rec_ent = _i64(rng.integers(0, E, size=R))
    tree = _flat_tree(P, A)
    rec_dist = _u8(rng.random((R, A)) < 0.4)
    rec_file = _i32(rng.integers(0, F, size=R))
    cnt = np.bincount(rec_ent.cpu().numpy(), minlength=E)
    assert (cnt == 0).any() or E == 1
    ent_rec_ptr = _i64(np.concatenate([[0], np.cumsum(cnt)]))
    loglik = torch.as_tensor(rng.normal(size=256) * 1e3, dtype=torch.float64).to(DEV)
    err = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    n_counts = 1 + A * F + A + 1
    nh = C.resort_hist_size(E, P)
    o = types.SimpleNamespace(
        part=torch.full((E,), -7, dtype=torch.int32, device=DEV),
        tile_base=torch.full((nh + 1,), -7, dtype=torch.int64, device=DEV),
        ent_part=torch.full((E,), -7, dtype=torch.int32, device=DEV),
        ent_values=torch.full((E, A), -7, dtype=torch.int32, device=DEV),
        rec_ent=torch.full((R,), -7, dtype=torch.int64, device=DEV),
        rec_part=torch.full((R,), -7, dtype=torch.int32, device=DEV),
        ent_ptr=torch.full((P + 1,), -7, dtype=torch.int64, device=DEV),
        counts=torch.zeros(n_counts, dtype=torch.int64, device=DEV),
        packed=torch.full((2 + n_counts,), -7.0, dtype=torch.float64, device=DEV))
    resort = (ent_values, o.part, rec_ent, tree["kind"], tree["attr"], tree["a"],
              tree["b"], tree["rset"], P, torch.empty(nh, dtype=torch.int32, device=DEV),
              o.tile_base, torch.empty(E, dtype=torch.int32, device=DEV), o.ent_part,
              o.ent_values, o.rec_ent, o.rec_part, o.ent_ptr)
    if merged:
        C.sweep_tail(*resort, rec_dist, rec_file, ent_rec_ptr, o.counts, loglik,
                     o.packed, err)
    else:
        C.partition_resort(*resort)
        C.summary_counts(rec_dist, rec_file, ent_rec_ptr, E, o.counts, loglik,
                         o.packed, err)
    return o, nh


@gpu
@pytest.mark.parametrize("E,P,nh_want", [(2500, 1, 3), (2500, 4, 12), (1, 1, 1),
                                         (20000, 256, 5120)])
def test_resort_prologue_and_sweep_tail(monkeypatch, E, P, nh_want):
    R = 3000
    monkeypatch.setenv("DBLINK_RESORT_SCAN", "0")  # re-read per launch
    ref, nh = _tail(E, P, R, merged=False)
    assert nh == nh_want  # 5120 counters: above the prologue's 4096, the scan stays
    assert float(ref.packed[-1]) == 5.0 and int(ref.counts[1:1 + 6].sum()) > 0
    monkeypatch.setenv("DBLINK_RESORT_SCAN", "1")
    for merged in (False, True):
        new, _ = _tail(E, P, R, merged=merged)
        for f in vars(ref):
            assert torch.equal(getattr(new, f), getattr(ref, f)), (f, merged)
    monkeypatch.setenv("DBLINK_RESORT_SCAN", "0")
    new, _ = _tail(E, P, R, merged=True)
    for f in vars(ref):
        assert torch.equal(getattr(new, f), getattr(ref, f)), f


# ---- whole chains: each new switch off in turn -------------------------------------

SWITCHES = ["DBLINK_BEGIN_MERGE", "DBLINK_LINK_MERGE", "DBLINK_RESORT_SCAN",
            "DBLINK_TAIL_MERGE"]
_CHAINS = {}


def _chain(monkeypatch, off, graphs, sampler):
    """30 sweeps of 500 records in 4 partitions with switch `off` (or none)
    turned off; the all-on run of a (sampler, graphs) pair is computed once."""
    key = (off, graphs, sampler)
    if key in _CHAINS:
        return _CHAINS[key]
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    for s in SWITCHES:
        monkeypatch.setenv(s, "0" if s == off else "1")
    for s in ("DBLINK_FUSED_GLUE", "DBLINK_INDEX_MERGE", "DBLINK_VALUE_MERGE"):
        monkeypatch.setenv(s, "1")
    # early in a chain base lists are short: a split length of 4 puts records
    # on the split path every sweep (see test_gpu_link_split)
    monkeypatch.setenv("DBLINK_LINK_SPLIT_LEN", "4")
    monkeypatch.setenv("DBLINK_LINK_SPLIT_GRID", "16")
    monkeypatch.setenv("DBLINK_GRAPHS", "1" if graphs else "0")
    n = 500
    cache, rec_values, rec_files = _data(n)
    partitioner = KDTreePartitioner(2, [3, 4])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=7)
    engine = GpuEngine(cache, partitioner, device=DEV)
    assert (engine._begin_merge, engine._link_merge, engine._tail_merge) == tuple(
        s != off for s in SWITCHES if s != "DBLINK_RESORT_SCAN")
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(sampler)
    series, listed = [], 0
    for _ in range(30):
        engine.step(state, flags)
        series.append((state.summary.num_isolates,
                       state.summary.agg_distortions.copy()))
        listed += int(engine._split_cnt.cpu())
    if graphs:
        assert len(engine._graphs) == 2
    if sampler != "PCG-II":
        assert listed > 0  # the split path served records
    engine.sync_state(state)
    _CHAINS[key] = (engine, state, series)
    return _CHAINS[key]


@gpu
@pytest.mark.parametrize("off", SWITCHES)
@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("sampler", ["PCG-I", "Gibbs", "PCG-II"])
def test_chain_equal_with_each_new_switch_off(monkeypatch, sampler, graphs, off):
    full = _chain(monkeypatch, None, graphs, sampler)
    arm = _chain(monkeypatch, off, graphs, sampler)
    _assert_chains_equal(full, arm)
    sa, sb = full[1], arm[1]
    assert np.array_equal(sa.dist_probs.probs, sb.dist_probs.probs)
    assert sa.summary.log_likelihood == sb.summary.log_likelihood
