"""The merged launches of the sweep glue against the launches they replace.

``kernels.hip`` lets the index scan zero its own counters
(``scan_excl(..., clear=True)``), computes the candidate ranges in the
posting scatter's launch (``postings_scatter_ranges``) and covers the three
thread-per-pair value classes with one kernel (``value_update_merged``). Every
output is an integer array, so each comparison is ``torch.equal`` against the
launches replaced; the chain tests run whole engines with each switch off in
turn.
"""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_sweep_glue import _assert_chains_equal, _data  # noqa: E402

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).to(DEV)


# ---- scan with clear -------------------------------------------------------------


@gpu
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 4096, 4097, 7880, 1 << 17, (1 << 17) + 5])
def test_scan_excl_clear(n, offset):
    rng = np.random.default_rng(n)
    counts = _i32(rng.integers(0, 9, size=n + offset))[offset:]
    ptr_ref = torch.full((n + 1 + offset,), -7, dtype=torch.int64, device=DEV)[offset:]
    cur_ref = torch.full((n + offset,), -7, dtype=torch.int32, device=DEV)[offset:]
    C.scan_excl(counts, ptr_ref, cur_ref)  # the three-argument call still works
    assert counts.any()

    ptr = torch.full((n + 1 + offset,), -7, dtype=torch.int64, device=DEV)[offset:]
    cur = torch.full((n + offset,), -7, dtype=torch.int32, device=DEV)[offset:]
    C.scan_excl(counts, ptr, cur, True)
    assert torch.equal(ptr, ptr_ref)
    assert torch.equal(cur, cur_ref)
    assert not counts.any()

    C.scan_excl(counts, ptr, cur[:0], clear=True)  # scan of the cleared buffer
    assert not ptr.any()


# ---- posting scatter + candidate ranges ---------------------------------------


def _index_case(name):
    rng = np.random.default_rng(31)
    A, P = 5, 4
    pairs = []
    missing = False
    if name == "plain":
        E, R = 2000, 3000
    elif name == "pair_and_missing":
        E, R = 2000, 3000
        pairs, missing = [(0, 1)], True
    elif name == "ragged":  # E * T = 5195 and R * T = 6495: no multiple of 1024
        E, R = 1039, 1299
    elif name == "single_record":
        E, R = 2000, 1
    elif name == "fewer_records":
        E, R = 3000, 500
    elif name == "more_records":
        E, R = 500, 3000
    V = [40, 12, 28, 90, 70]
    ent_values = np.stack([rng.integers(0, v, size=E) for v in V], axis=1)
    rec_values = np.stack([rng.integers(0, v, size=R) for v in V], axis=1)
    if missing:
        rec_values[rng.random((R, A)) < 0.2] = -1
    a1 = _i32([p[0] for p in pairs])
    a2 = _i32([p[1] for p in pairs])
    v2 = _i32([V[p[1]] for p in pairs])
    vmax = max(V + [V[p[0]] * V[p[1]] for p in pairs])
    return dict(
        ent_part=_i32(np.sort(rng.integers(0, P, size=E))), ent_values=_i32(ent_values),
        rec_part=_i32(rng.integers(0, P, size=R)), rec_values=_i32(rec_values),
        a1=a1, a2=a2, v2=v2, vmax=vmax, nk=P * (A + len(pairs)) * vmax,
        T=A + len(pairs))


@gpu
@pytest.mark.parametrize("name", ["plain", "pair_and_missing", "ragged",
                                  "single_record", "fewer_records", "more_records"])
def test_postings_scatter_ranges_matches_the_pair(name):
    c = _index_case(name)
    E, R, T, nk = c["ent_values"].shape[0], c["rec_values"].shape[0], c["T"], c["nk"]
    pair = (c["a1"], c["a2"], c["v2"], c["vmax"])
    counts = torch.zeros(nk, dtype=torch.int32, device=DEV)
    C.postings_hist(c["ent_part"], c["ent_values"], *pair, counts)
    ptr = torch.empty(nk + 1, dtype=torch.int64, device=DEV)
    cursor = torch.empty(nk, dtype=torch.int32, device=DEV)
    C.scan_excl(counts, ptr, cursor)

    post_ref = torch.full((E * T,), -7, dtype=torch.int32, device=DEV)
    C.postings_scatter(c["ent_part"], c["ent_values"], *pair, cursor.clone(), post_ref)
    lo_ref = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    hi_ref = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    C.cand_ranges(c["rec_part"], c["rec_values"], *pair[:3], ptr, c["vmax"],
                  lo_ref, hi_ref)

    post = torch.full((E * T,), -7, dtype=torch.int32, device=DEV)
    lo = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    hi = torch.full((R, T), -7, dtype=torch.int64, device=DEV)
    ptr_before = ptr.clone()
    cur = cursor.clone()
    C.postings_scatter_ranges(c["ent_part"], c["ent_values"], c["rec_part"],
                              c["rec_values"], *pair, cur, ptr, post, lo, hi)
    assert torch.equal(lo, lo_ref)
    assert torch.equal(hi, hi_ref)
    assert torch.equal(ptr, ptr_before)  # the prefix is untouched
    assert torch.equal(cur.to(torch.int64), ptr[1:])  # every cursor ran to its end
    # order within a key is arbitrary: compare each key's postings as a set
    seg = torch.repeat_interleave(
        torch.arange(nk, device=DEV), (ptr[1:] - ptr[:-1]))
    key_of = seg.to(torch.int64) * E
    assert torch.equal(torch.sort(key_of + post)[0], torch.sort(key_of + post_ref)[0])


# ---- whole chains: each switch off in turn -------------------------------------

SWITCHES = ["DBLINK_INDEX_MERGE", "DBLINK_VALUE_MERGE"]
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
    monkeypatch.setenv("DBLINK_FUSED_GLUE", "1")
    monkeypatch.setenv("DBLINK_GRAPHS", "1" if graphs else "0")
    n = 500
    cache, rec_values, rec_files = _data(n)
    partitioner = KDTreePartitioner(2, [3, 4])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=7)
    engine = GpuEngine(cache, partitioner, device=DEV)
    assert (engine._index_merge, engine._value_merge) == tuple(
        s != off for s in SWITCHES)
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(sampler)
    series = []
    for _ in range(30):
        engine.step(state, flags)
        series.append((state.summary.num_isolates,
                       state.summary.agg_distortions.copy()))
    if graphs:
        assert len(engine._graphs) == 2
    engine.sync_state(state)
    _CHAINS[key] = (engine, state, series)
    return _CHAINS[key]


@gpu
@pytest.mark.parametrize("off", SWITCHES)
@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("sampler", ["PCG-I", "Gibbs", "PCG-II"])
def test_chain_equal_with_each_switch_off(monkeypatch, sampler, graphs, off):
    full = _chain(monkeypatch, None, graphs, sampler)
    arm = _chain(monkeypatch, off, graphs, sampler)
    _assert_chains_equal(full, arm)
    sa, sb = full[1], arm[1]
    assert np.array_equal(sa.dist_probs.probs, sb.dist_probs.probs)
    assert sa.summary.log_likelihood == sb.summary.log_likelihood
