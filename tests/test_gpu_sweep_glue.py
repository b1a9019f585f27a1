"""The sweep's native integer glue against the torch expressions it replaces.

Three ops of ``kernels.hip`` ("Sweep glue") stand in for torch sorts,
searchsorted, scatter_add and gathers between the sampling kernels:
``ent_csr_build`` (entity -> records CSR + kobs + link store),
``partition_resort`` (KD descent + stable re-sort by partition id + record
remap + next partition offsets) and ``scan_excl`` (index prefix + cursor).
All outputs are integers, so every comparison is ``torch.equal`` against the
torch expression on the same device tensors; the chain tests then run whole
engines with ``DBLINK_FUSED_GLUE=1`` and ``=0`` side by side.
"""

import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)


def _i64(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int64).to(DEV)


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(DEV)


# ---- entity -> records CSR ---------------------------------------------------


def _csr_torch(rec_ent, rec_values, E):
    """The expressions of the DBLINK_FUSED_GLUE=0 sweep."""
    R, A = rec_values.shape
    sorted_re, order = torch.sort(rec_ent, stable=True)
    ptr = torch.searchsorted(
        sorted_re, torch.arange(E + 1, device=DEV, dtype=torch.int64))
    obs = rec_values >= 0
    kobs = torch.zeros(E * A, dtype=torch.int32, device=DEV)
    pair_idx = (rec_ent.view(R, 1) * A
                + torch.arange(A, device=DEV, dtype=torch.int64).view(1, A))
    kobs.scatter_add_(0, pair_idx.reshape(-1), obs.reshape(-1).to(torch.int32))
    return ptr, order, kobs


def _csr_case(name):
    rng = np.random.default_rng(11)
    A = 5
    if name == "random":
        # links only into the first two thirds of the entities
        R, E = 3000, 2000
        ent = rng.integers(0, 2 * E // 3, size=R)
    elif name == "one_entity":
        R, E = 3000, 2000
        ent = np.full(R, 1234)
    elif name == "identity":
        R = E = 2000
        ent = np.arange(R)
    elif name == "single_record":
        R, E = 1, 2000
        ent = np.array([1999])
    elif name == "single_entity":
        R, E = 100, 1
        ent = np.zeros(R)
    elif name == "past_a_block":
        R, E = 1025, 700
        ent = rng.integers(0, E, size=R)
    elif name == "segment_lengths":
        # around the one-thread / whole-block threshold of the order pass (32)
        lens = [1, 2, 31, 32, 33, 64, 65, 300, 0, 7]
        E = len(lens)
        ent = rng.permutation(np.repeat(np.arange(E), lens))
        R = ent.size
    vals = rng.integers(0, 50, size=(R, A))
    vals[rng.random((R, A)) < 0.2] = -1  # missing
    return _i64(ent), _i32(vals), E


CSR_CASES = ["random", "one_entity", "identity", "single_record", "single_entity",
             "past_a_block", "segment_lengths"]


@gpu
@pytest.mark.parametrize("name", CSR_CASES)
def test_ent_csr_build_matches_torch(name):
    rec_ent_new, rec_values, E = _csr_case(name)
    R, A = rec_values.shape
    ptr_ref, idx_ref, kobs_ref = _csr_torch(rec_ent_new, rec_values, E)

    cnt = torch.zeros(E, dtype=torch.int32, device=DEV)
    kobs = torch.zeros(E * A, dtype=torch.int32, device=DEV)
    stored = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    ptr = torch.full((E + 1,), -7, dtype=torch.int64, device=DEV)
    idx = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    C.ent_csr_build(rec_ent_new, rec_values, stored, cnt, kobs, ptr, idx)

    assert torch.equal(ptr, ptr_ref)
    assert torch.equal(idx, idx_ref)
    assert torch.equal(kobs, kobs_ref)
    assert torch.equal(stored, rec_ent_new)
    assert not cnt.any()  # the scatter pass counts the histogram back to zero


# ---- index prefix --------------------------------------------------------------


@gpu
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 4096, 4097, 7880, 40001, 1 << 17,
                               (1 << 17) + 5])
def test_scan_excl_matches_cumsum(n, offset):
    """One block up to 2^17 counters (4096 per tile), cumsum above; 16-byte
    accesses on aligned buffers (offset 0), element-wise ones otherwise."""
    rng = np.random.default_rng(n)
    counts = _i32(rng.integers(0, 9, size=n + offset))[offset:]
    ptr_ref = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    torch.cumsum(counts, 0, dtype=torch.int64, out=ptr_ref[1:])
    cur_ref = torch.empty(n, dtype=torch.int32, device=DEV)
    cur_ref.copy_(ptr_ref[:-1])

    ptr = torch.full((n + 1 + offset,), -7, dtype=torch.int64, device=DEV)[offset:]
    cur = torch.full((n + offset,), -7, dtype=torch.int32, device=DEV)[offset:]
    C.scan_excl(counts, ptr, cur)
    assert torch.equal(ptr, ptr_ref)
    assert torch.equal(cur, cur_ref)

    ptr.fill_(-7)
    C.scan_excl(counts, ptr, cur[:0])  # cursor is optional
    assert torch.equal(ptr, ptr_ref)


# ---- KD descent + partition re-sort -------------------------------------------


def _flat_tree(P, A, vmax=256):
    """Heap-layout KD tree of range splits (kind 1: right iff v > a) with
    2^ceil(log2 P) leaves numbered min(leaf, P - 1): any P, not only powers
    of two. Splits bisect each attribute's remaining value range in turn."""
    depth = int(np.ceil(np.log2(P))) if P > 1 else 0
    n = 2 ** (depth + 1) - 1
    kind = np.zeros(n, np.int32)
    attr = np.full(n, -1, np.int32)
    a = np.zeros(n, np.int32)
    b = np.zeros(n, np.int32)

    def fill(nid, level, ranges):
        if level == depth:
            a[nid] = min(nid - (2 ** depth - 1), P - 1)
            return
        at = level % A
        lo, hi = ranges[at]
        mid = (lo + hi) // 2
        kind[nid], attr[nid], a[nid] = 1, at, mid - 1
        left, right = dict(ranges), dict(ranges)
        left[at], right[at] = (lo, mid), (mid, hi)
        fill(2 * nid + 1, level + 1, left)
        fill(2 * nid + 2, level + 1, right)

    fill(0, 0, {i: (0, vmax) for i in range(A)})
    return {"kind": _i32(kind), "attr": _i32(attr), "a": _i32(a), "b": _i32(b),
            "rset": torch.zeros(1, dtype=torch.int32, device=DEV)}


def _resort_torch(ent_values, rec_ent, tree, P):
    """kd_descent + the engine's present _sort_into + searchsorted."""
    from dblink_amd.engine.gpu_engine import GpuEngine

    E, A = ent_values.shape
    part = torch.empty(E, dtype=torch.int32, device=DEV)
    C.kd_descent(ent_values, tree["kind"], tree["attr"], tree["a"], tree["b"],
                 tree["rset"], part)
    gs = types.SimpleNamespace(E=E, ent_part=part, ent_values=ent_values,
                               rec_ent=rec_ent)
    out = types.SimpleNamespace(
        ent_part=torch.empty_like(part), ent_values=torch.empty_like(ent_values),
        rec_ent=torch.empty_like(rec_ent),
        rec_part=torch.empty(rec_ent.numel(), dtype=torch.int32, device=DEV))
    eng = types.SimpleNamespace(model=types.SimpleNamespace(A=A), device=DEV)
    GpuEngine._sort_into(eng, gs, out)
    ent_ptr = torch.searchsorted(
        out.ent_part.to(torch.int64).contiguous(),
        torch.arange(P + 1, device=DEV, dtype=torch.int64))
    return part, out, ent_ptr


def _resort_native(ent_values, rec_ent, tree, P):
    E, A = ent_values.shape
    R = rec_ent.numel()
    nh = C.resort_hist_size(E, P)
    part = torch.full((E,), -7, dtype=torch.int32, device=DEV)
    out = types.SimpleNamespace(
        ent_part=torch.full((E,), -7, dtype=torch.int32, device=DEV),
        ent_values=torch.full((E, A), -7, dtype=torch.int32, device=DEV),
        rec_ent=torch.full((R,), -7, dtype=torch.int64, device=DEV),
        rec_part=torch.full((R,), -7, dtype=torch.int32, device=DEV))
    ent_ptr = torch.full((P + 1,), -7, dtype=torch.int64, device=DEV)
    C.partition_resort(
        ent_values, part, rec_ent, tree["kind"], tree["attr"], tree["a"],
        tree["b"], tree["rset"], P,
        torch.empty(nh, dtype=torch.int32, device=DEV),
        torch.empty(nh + 1, dtype=torch.int64, device=DEV),
        torch.empty(E, dtype=torch.int32, device=DEV),
        out.ent_part, out.ent_values, out.rec_ent, out.rec_part, ent_ptr)
    return part, out, ent_ptr


def _resort_inputs(E, A, variant):
    rng = np.random.default_rng(E + 17)
    if variant == "spread":
        vals = rng.integers(0, 256, size=(E, A))
    elif variant == "empty_partitions":  # only the low quarter of each range
        vals = rng.integers(0, 64, size=(E, A))
    elif variant == "one_partition":
        vals = np.tile(rng.integers(0, 256, size=(1, A)), (E, 1))
    R = E + E // 2 + 1
    return _i32(vals), _i64(rng.integers(0, E, size=R))


def _assert_resort_equal(ent_values, rec_ent, tree, P):
    part_ref, out_ref, ptr_ref = _resort_torch(ent_values, rec_ent, tree, P)
    part, out, ptr = _resort_native(ent_values, rec_ent, tree, P)
    assert torch.equal(part, part_ref)
    assert torch.equal(out.ent_part, out_ref.ent_part)
    assert torch.equal(out.ent_values, out_ref.ent_values)
    assert torch.equal(out.rec_ent, out_ref.rec_ent)
    assert torch.equal(out.rec_part, out_ref.rec_part)
    assert torch.equal(ptr, ptr_ref)


@gpu
@pytest.mark.parametrize("P", [1, 4, 64, 256])
@pytest.mark.parametrize("variant", ["spread", "empty_partitions", "one_partition"])
def test_partition_resort_matches_torch(P, variant):
    assert C.resort_max_parts() == 256
    A = 3
    ent_values, rec_ent = _resort_inputs(5000, A, variant)
    _assert_resort_equal(ent_values, rec_ent, _flat_tree(P, A), P)


@gpu
@pytest.mark.parametrize("E", [1, 1025])
def test_partition_resort_small_and_past_a_tile(E):
    A = 3
    ent_values, rec_ent = _resort_inputs(E, A, "spread")
    _assert_resort_equal(ent_values, rec_ent, _flat_tree(4, A), 4)


@gpu
def test_partition_resort_refuses_above_cap():
    """One past the LDS cap the op raises; the engine keeps the torch path
    there (test_chain_above_resort_cap runs it)."""
    P = C.resort_max_parts() + 1
    A = 3
    ent_values, rec_ent = _resort_inputs(5000, A, "spread")
    tree = _flat_tree(P, A)
    # the torch path itself is fine at this P
    _, out_ref, ptr_ref = _resort_torch(ent_values, rec_ent, tree, P)
    assert int(ptr_ref[-1]) == 5000
    with pytest.raises(RuntimeError, match="partitions"):
        _resort_native(ent_values, rec_ent, tree, P)


# ---- whole chains: fused glue on / off -----------------------------------------


def _bench_module():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench

    return bench


_DATA = {}


def _data(n):
    if n not in _DATA:
        _DATA[n] = _bench_module().build_cache_and_records(n, seed=7)
    return _DATA[n]


def _run_chain(monkeypatch, fused, graphs, sampler, levels, n, sweeps):
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    monkeypatch.setenv("DBLINK_FUSED_GLUE", "1" if fused else "0")
    monkeypatch.setenv("DBLINK_GRAPHS", "1" if graphs else "0")
    cache, rec_values, rec_files = _data(n)
    partitioner = KDTreePartitioner(levels, [3, 4])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=7)
    engine = GpuEngine(cache, partitioner, device=DEV)
    assert engine._fused == fused
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(sampler)
    series = []
    for _ in range(sweeps):
        engine.step(state, flags)
        series.append((state.summary.num_isolates,
                       state.summary.agg_distortions.copy()))
    if graphs:  # both directions were captured and replayed
        assert len(engine._graphs) == 2
    engine.sync_state(state)
    return engine, state, series


def _assert_chains_equal(a, b):
    (_, sa, ser_a), (_, sb, ser_b) = a, b
    for f in ("rec_ent", "ent_values", "ent_part", "rec_dist"):
        assert np.array_equal(getattr(sa, f), getattr(sb, f)), f
    for k, ((iso_a, agg_a), (iso_b, agg_b)) in enumerate(zip(ser_a, ser_b)):
        assert iso_a == iso_b, k
        assert np.array_equal(agg_a, agg_b), k


@gpu
@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("sampler", ["PCG-I", "Gibbs", "PCG-II"])
def test_chain_equal_fused_and_torch_glue(monkeypatch, sampler, graphs):
    """2000 records, 4 partitions, 40 sweeps from deterministic_init: past the
    capture point of both graph directions (sweeps 3 and 4)."""
    runs = [_run_chain(monkeypatch, fused, graphs, sampler, levels=2, n=2000,
                       sweeps=40) for fused in (True, False)]
    assert runs[0][0]._resort_fused_ok() and not runs[1][0]._resort_fused_ok()
    _assert_chains_equal(*runs)


@gpu
def test_chain_above_resort_cap(monkeypatch):
    """512 partitions: above the re-sort cap the fused engine keeps the torch
    re-sort (and still uses the native CSR and prefix); results unchanged."""
    runs = [_run_chain(monkeypatch, fused, True, "PCG-I", levels=9, n=2000,
                       sweeps=8) for fused in (True, False)]
    assert runs[0][0].num_partitions > C.resort_max_parts()
    assert not runs[0][0]._resort_fused_ok()
    _assert_chains_equal(*runs)


# ---- error count in the packed summary -----------------------------------------


@gpu
def test_summary_counts_packs_error_count():
    A, F, E, R = 2, 1, 4, 6
    n_counts = 1 + A * F + A + 1
    ptr = _i64([0, 2, 2, 5, 6])
    args = (torch.zeros((R, A), dtype=torch.uint8, device=DEV),
            torch.zeros(R, dtype=torch.int32, device=DEV), ptr, E)
    loglik = torch.zeros(256, dtype=torch.float64, device=DEV)
    for err in (0, 3):
        packed = torch.full((1 + n_counts + 1,), -7.0, dtype=torch.float64, device=DEV)
        C.summary_counts(*args, torch.zeros(n_counts, dtype=torch.int64, device=DEV),
                         loglik, packed, _i32([err]))
        host = packed.cpu().numpy()
        assert host[-1] == err
        assert host[1] == 1  # one entity without records
    # without an error tensor the buffer keeps its old size
    packed = torch.zeros(1 + n_counts, dtype=torch.float64, device=DEV)
    C.summary_counts(*args, torch.zeros(n_counts, dtype=torch.int64, device=DEV),
                     loglik, packed, torch.empty(0, dtype=torch.int32, device=DEV))
    assert packed[1] == 1


@gpu
def test_read_summary_raises_on_error_count(monkeypatch):
    """The engine learns of empty candidate sets from the packed buffer alone:
    a count left in the link kernels' error word raises at the next summary."""
    engine, state, _ = _run_chain(monkeypatch, True, False, "PCG-I", levels=2,
                                  n=2000, sweeps=1)
    engine._err.fill_(2)
    with pytest.raises(RuntimeError, match="2 empty candidate sets"):
        engine.initial_summary(state)
