"""GPU kernel tests (run on MI355X via gpurun).

Numerics strategy: the Gibbs kernels SAMPLE from discrete distributions, so
parity with the CPU fp64 reference is checked distributionally — many
independent replicas of one configuration in a single launch (each replica
draws with its own Philox counters), empirical frequencies compared against
exact fp64 probabilities computed in numpy. Deterministic kernels
(kd_descent, summary_loglik, sim_pairs_gpu) are checked exactly / to fp32
tolerance.
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


def _dev(arr, dtype):
    return torch.as_tensor(np.ascontiguousarray(arr)).to(dtype).to(DEV)


def make_model(device, values_weights=None, threshold=5.0, max_sim=10.0, Kc=10,
               priors=(0.5, 50.0), names=None):
    """Small two-attribute model (1 const, 1 Levenshtein) on the GPU."""
    from dblink_amd.engine.gpu_engine import GpuModel
    from dblink_amd.models.attribute_index import _python_sim_pairs
    from dblink_amd.models.records import Attribute, BetaShapeParameters, RecordsCache, RecordsTable
    from dblink_amd.models.similarity import ConstantSimilarityFn, LevenshteinSimilarityFn

    rng = np.random.default_rng(0)
    if names is None:
        names = ["ANNA", "ANNE", "ANNAH", "BOB", "BORB", "CLAIRE", "CLAIR", "DAVE"]
    years = [str(y) for y in range(1950, 1960)]
    rows = []
    for i in range(max(400, len(names))):
        # every supplied name appears at least once so the full vocab builds
        nm = names[i] if i < len(names) else str(rng.choice(names))
        rows.append([str(rng.choice(years)), nm])
    n_rows = len(rows)
    table = RecordsTable.from_rows([str(i) for i in range(n_rows)],
                                   ["0"] * n_rows, rows)
    prior = BetaShapeParameters(*priors)
    attrs = [
        Attribute("year", ConstantSimilarityFn(), prior),
        Attribute("name", LevenshteinSimilarityFn(threshold, max_sim), prior),
    ]
    cache = RecordsCache.build(table, attrs, max_cluster_size=Kc,
                               pair_sweep=_python_sim_pairs)
    model = GpuModel(cache, device, Kc)
    return cache, model


def tv_distance(emp, exact):
    return 0.5 * np.abs(emp - exact).sum()


@gpu
def test_sim_pairs_gpu_matches_cpu():
    from dblink_amd.models.attribute_index import _python_sim_pairs
    from dblink_amd.models.similarity import LevenshteinSimilarityFn

    fn = LevenshteinSimilarityFn(5.0, 10.0)
    values = sorted({
        "Australian Capital Territory", "New South Wales", "Northern Territory",
        "Queensland", "South Australia", "Tasmania", "Victoria", "Western Australia",
        "ANNA", "ANNE", "ANNAH", "BOB", "BORB", "",
    })
    ref = _python_sim_pairs(values, fn)
    enc = [v.encode() for v in values]
    lens = np.array([len(e) for e in enc], dtype=np.int32)
    buf = np.zeros((len(enc), 64), dtype=np.uint8)
    for i, e in enumerate(enc):
        buf[i, : len(e)] = np.frombuffer(e, dtype=np.uint8)
    row_ptr, col, expsim = C.sim_pairs_gpu(_dev(buf, torch.uint8), _dev(lens, torch.int32),
                                           5.0, 10.0)
    row_ptr = row_ptr.cpu().numpy()
    np.testing.assert_array_equal(row_ptr, ref.row_ptr)
    # rows may be filled in any order -> compare as sets per row
    col = col.cpu().numpy()
    expsim = expsim.cpu().numpy()
    for v in range(len(values)):
        lo, hi = row_ptr[v], row_ptr[v + 1]
        got = dict(zip(col[lo:hi].tolist(), expsim[lo:hi].tolist()))
        want = dict(zip(ref.col[ref.row_ptr[v]:ref.row_ptr[v+1]].tolist(),
                        ref.expsim[ref.row_ptr[v]:ref.row_ptr[v+1]].tolist()))
        assert set(got) == set(want)
        for k in want:
            assert got[k] == pytest.approx(want[k], rel=1e-5)


@gpu
def test_kd_descent_matches_cpu():
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    rng = np.random.default_rng(2)
    vals = rng.integers(0, 25, size=(4000, 3)).astype(np.int32)
    p = KDTreePartitioner(3, [0, 1, 2]).fit(vals)
    flat = p.as_flat()
    out = torch.empty(4000, dtype=torch.int32, device=DEV)
    rset = flat["rset"] if flat["rset"].size else np.zeros(1, np.int32)
    C.kd_descent(_dev(vals, torch.int32), _dev(flat["kind"], torch.int32),
                 _dev(flat["attr"], torch.int32), _dev(flat["a"], torch.int32),
                 _dev(flat["b"], torch.int32), _dev(rset, torch.int32), out)
    np.testing.assert_array_equal(out.cpu().numpy(), p.get_partition_ids(vals))


@gpu
def test_distortion_kernel_distribution():
    """Empirical distortion rates vs exact Bernoulli probabilities
    (GibbsUpdates.scala:324-359)."""
    cache, model = make_model(DEV)
    a_name = 1  # Levenshtein attribute
    ia = cache.indexed_attributes[a_name]
    N = 40000
    theta = np.array([[0.05], [0.12]])
    model.theta.copy_(torch.from_numpy(theta).float())

    # three cases per record: missing(attr0), agree(attr1), disagree via values
    x_name = 2  # some value id
    rec_values = np.tile(np.array([[-1, x_name]], dtype=np.int32), (N, 1))
    ent_values = np.tile(np.array([[0, x_name]], dtype=np.int32), (N, 1))
    rec_ent = np.arange(N, dtype=np.int64)
    rec_dist = np.zeros((N, 2), dtype=np.uint8)
    C.distortion_update(
        _dev(rec_values, torch.int32), (d := _dev(rec_dist, torch.uint8)),
        _dev(np.zeros(N, np.int32), torch.int32),
        _dev(np.arange(N, dtype=np.int64), torch.int64),
        _dev(rec_ent, torch.int64), _dev(ent_values, torch.int32),
        model.theta, model.phi, model.norm_lin, model.self_expsim, model.voff,
        model.attr_const, 1234, 7, torch.empty(0, dtype=torch.int64, device=DEV),
        model.log_phi, model.log_norm, model.csr_row_ptr, model.csr_col,
        model.csr_sim, torch.empty(0, dtype=torch.float64, device=DEV),
    )
    z = d.cpu().numpy()
    # attr 0 missing: P(z=1) = theta
    assert z[:, 0].mean() == pytest.approx(0.05, abs=0.01)
    # attr 1 agree: p = pr1/(pr0+pr1)
    px = ia.index.probability_of(x_name)
    pr1 = 0.12 * px * ia.index.sim_norms[x_name] * ia.index.exp_sim_of(x_name, x_name)
    pr0 = 1 - 0.12
    assert z[:, 1].mean() == pytest.approx(pr1 / (pr0 + pr1), abs=0.01)

    # disagree: always distorted
    ent_values[:, 1] = x_name + 1
    C.distortion_update(
        _dev(rec_values, torch.int32), (d := _dev(rec_dist, torch.uint8)),
        _dev(np.zeros(N, np.int32), torch.int32),
        _dev(np.arange(N, dtype=np.int64), torch.int64),
        _dev(rec_ent, torch.int64), _dev(ent_values, torch.int32),
        model.theta, model.phi, model.norm_lin, model.self_expsim, model.voff,
        model.attr_const, 99, 3, torch.empty(0, dtype=torch.int64, device=DEV),
        model.log_phi, model.log_norm, model.csr_row_ptr, model.csr_col,
        model.csr_sim, torch.empty(0, dtype=torch.float64, device=DEV),
    )
    assert d.cpu().numpy()[:, 1].min() == 1


@gpu
def test_link_kernel_distribution():
    """PCG-I link update: N identical records in one partition, empirical
    entity-selection frequencies vs exact weights (GibbsUpdates.scala:398-430)."""
    cache, model = make_model(DEV)
    ia = cache.indexed_attributes[1]
    idx = ia.index
    E = 12
    # entities: attr0 value all = 3 (so nd-attr0 matches everyone); attr1 varied
    ent_vals = np.zeros((E, 2), dtype=np.int32)
    ent_vals[:, 0] = 3
    ent_vals[:, 1] = (np.arange(E) % idx.num_values).astype(np.int32)
    x = 0  # record's name value
    N = 30000
    rec_values = np.tile(np.array([[3, x]], dtype=np.int32), (N, 1))
    rec_dist = np.tile(np.array([[0, 1]], dtype=np.uint8), (N, 1))  # name distorted

    # exact weights over candidates = all entities (single nd set = everyone)
    w = np.array([
        idx.sim_norms[y] * idx.exp_sim_of(x, int(y)) * idx.probability_of(x)
        for y in ent_vals[:, 1]
    ])
    exact = w / w.sum()

    # postings: key layout (part*A + a)*Vmax + v, a-major flatten like the engine
    A, Vmax = 2, model.Vmax
    keys = ((0 * A + np.repeat([0, 1], E)) * Vmax
            + ent_vals.T.reshape(-1)).astype(np.int64)
    order = np.argsort(keys, kind="stable")
    sorted_keys = keys[order]
    postings = (order % E).astype(np.int32)
    qk = np.array([(0 * A + 0) * Vmax + 3, (0 * A + 1) * Vmax + x], dtype=np.int64)
    lo = np.searchsorted(sorted_keys, qk, "left")
    hi = np.searchsorted(sorted_keys, qk, "right")
    cand_lo = np.tile(lo, (N, 1)).astype(np.int64)
    cand_hi = np.tile(hi, (N, 1)).astype(np.int64)

    out = torch.empty(N, dtype=torch.int64, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    C.link_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.arange(N, dtype=np.int64), torch.int64),
        _dev(np.zeros(N, np.int32), torch.int32),
        _dev(cand_lo, torch.int64), _dev(cand_hi, torch.int64),
        _dev(postings, torch.int32), _dev(ent_vals, torch.int32),
        _dev(np.array([0, E], dtype=np.int64), torch.int64),
        model.log_norm, model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.attr_const, 4321, 11, out,
        _dev(np.zeros(N, np.int64), torch.int64), err,
        torch.empty(0, dtype=torch.uint8, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int32, device=DEV),
        torch.empty(0, dtype=torch.int32, device=DEV),
    )
    assert int(err.cpu()) == 0
    sel = out.cpu().numpy()
    emp = np.bincount(sel, minlength=E) / N
    assert tv_distance(emp, exact) < 0.02, (emp, exact)


@gpu
def test_value_kernel_distribution():
    """Collapsed value update: E identical single-record clusters; empirical
    value frequencies vs the exact mixture P(v) = (base(v) + w_v) / (1 + W)
    (GibbsUpdates.scala:576-599)."""
    cache, model = make_model(DEV)
    a = 1
    ia = cache.indexed_attributes[a]
    idx = ia.index
    V = idx.num_values
    x = 1
    theta = np.array([[0.05], [0.08]])
    model.theta.copy_(torch.from_numpy(theta).float())
    E = 40000
    # entity e linked to exactly one record with name value x (observed)
    rec_values = np.tile(np.array([[3, x]], dtype=np.int32), (E, 1))
    rec_dist = np.ones((E, 2), dtype=np.uint8)
    ent_vals = np.zeros((E, 2), dtype=np.int32)
    ent_rec_ptr = np.arange(E + 1, dtype=np.int64)
    ent_rec_idx = np.arange(E, dtype=np.int64)

    # exact distribution (k=1): base = phi*norm/Z1; pert per reference
    base = idx.probs * idx.sim_norms / idx.sim_norm_total(1)
    th = 0.08
    px = idx.probability_of(x)
    normx = idx.sim_norms[x]
    cols, sims = idx.sim_index.row(x)
    vw = {}
    for v, es in zip(cols.tolist(), sims.tolist()):
        f = es + (1 / th - 1) / (px * normx) if v == x else es
        vw[v] = f
    w = np.zeros(V)
    for v, f in vw.items():
        w[v] = base[v] * (f - 1.0)
    W = w.sum()
    exact = (base + w) / (1.0 + W)

    ev = _dev(ent_vals, torch.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    C.value_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(E, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64),
        ev, model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 777, 5, 0, err,
        torch.arange(E * 2, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        model.csr_excl, model.csr_rawsum, model.z1,
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int32, device=DEV),
    )
    got = ev.cpu().numpy()[:, a]
    emp = np.bincount(got, minlength=V) / E
    assert tv_distance(emp, exact) < 0.02, (emp[:10], exact[:10])

    # same distribution via the table-based k1 thread kernel
    ev2 = _dev(ent_vals, torch.int32)
    C.value_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(E, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64),
        ev2, model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 777, 5, 0, err,
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.arange(E * 2, dtype=torch.int64, device=DEV),
        model.csr_excl, model.csr_rawsum, model.z1,
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int32, device=DEV),
    )
    got2 = ev2.cpu().numpy()[:, a]
    emp2 = np.bincount(got2, minlength=V) / E
    assert tv_distance(emp2, exact) < 0.02, (emp2[:10], exact[:10])


@gpu
def test_summary_loglik_matches_cpu():
    from dblink_amd.engine.cpu_engine import compute_summary
    from dblink_amd.engine.state import ChainState
    from dblink_amd.models.distortion import DistortionProbs

    cache, model = make_model(DEV)
    rng = np.random.default_rng(5)
    E, R, A = 300, 500, 2
    Vs = [cache.indexed_attributes[a].index.num_values for a in range(A)]
    ent_values = np.stack([rng.integers(0, Vs[a], E) for a in range(A)], 1).astype(np.int32)
    rec_values = np.stack([rng.integers(-1, Vs[a], R) for a in range(A)], 1).astype(np.int32)
    rec_ent = rng.integers(0, E, R).astype(np.int64)
    rec_dist = (rng.random((R, A)) < 0.3).astype(np.uint8)
    state = ChainState(
        iteration=0, ent_values=ent_values, ent_part=np.zeros(E, np.int32),
        rec_values=rec_values, rec_file=np.zeros(R, np.int32), rec_ent=rec_ent,
        rec_dist=rec_dist, rec_gid=np.arange(R, dtype=np.int64),
        dist_probs=DistortionProbs(np.full((A, 1), 0.05)), population_size=E,
        start_seed=0, current_seed=0,
    )
    ref = compute_summary(state, cache, state.dist_probs)

    out = torch.zeros(256, dtype=torch.float64, device=DEV)  # 256-slot spread
    C.summary_loglik(
        _dev(ent_values, torch.int32), _dev(rec_values, torch.int32),
        _dev(rec_dist, torch.uint8), _dev(rec_ent, torch.int64),
        model.log_phi, model.log_norm, model.voff, model.csr_row_ptr,
        model.csr_col, model.csr_sim, model.attr_const, out,
    )
    assert float(out.sum().cpu()) == pytest.approx(ref.log_likelihood, rel=1e-5)


@gpu
def test_gpu_end_to_end_accuracy(tmp_path):
    """Full GPU chain on synthetic RLdata-shaped data; F1/ARI oracle."""
    import bench as b
    from dblink_amd.analysis import chain as chain_q
    from dblink_amd.analysis import metrics as metrics_m
    from dblink_amd.engine import sampler as sampler_m
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner
    from dblink_amd.utils.synthdata import generate

    n = 300
    cols, header = generate(n, dup_fraction=0.1, seed=42)
    cache, rec_values, rec_files = b.build_cache_and_records(n, seed=42)
    partitioner = KDTreePartitioner(1, [3])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=319158)
    engine = GpuEngine(cache, partitioner, device=DEV)
    engine.rec_id_of = lambda gid: str(gid + 1)  # rec_id = row + 1 in synthdata
    engine.initial_summary(state)
    out = str(tmp_path)
    sampler_m.sample(engine, state, sample_size=100, output_path=out,
                     burnin_interval=100, thinning_interval=4,
                     checkpoint_interval=0, flags=SamplerFlags.for_sampler("PCG-I"))
    table = chain_q.load_chain(out, 150)
    smpc = chain_q.shared_most_probable_clusters(table)
    truth = metrics_m.membership_to_clusters(
        {cols["rec_id"][i]: cols["ent_id"][i] for i in range(n)}
    )
    pm = metrics_m.PairwiseMetrics.compute(smpc, truth)
    ari = metrics_m.adjusted_rand_index(smpc, truth)
    # chain-to-chain F1 variance at n=300 is large (measured 0.42-0.62 for
    # CPU chains across seeds; scripts/pairband.py shows the GPU posterior
    # matches the CPU one on long-run linked-pair counts) — this asserts the
    # sampler finds real structure, not a tight accuracy band
    assert pm.f1score > 0.40, (pm.precision, pm.recall)
    assert ari > 0.40


@gpu
def test_gpu_vs_cpu_posterior_band(tmp_path):
    """GPU and CPU engines must land in the same posterior band on the same
    data (log-likelihood trajectories agree within a few percent)."""
    import bench as b
    from dblink_amd.engine.cpu_engine import CpuEngine, SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    n = 200
    cache, rec_values, rec_files = b.build_cache_and_records(n, seed=9)
    flags = SamplerFlags.for_sampler("PCG-I")

    lls = {}
    for kind in ("cpu", "gpu"):
        partitioner = KDTreePartitioner(0, [])
        state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                                   cache, partitioner, seed=1)
        eng = (CpuEngine(cache, partitioner) if kind == "cpu"
               else GpuEngine(cache, partitioner, device=DEV))
        eng.initial_summary(state)
        tail = []
        for i in range(60):
            eng.step(state, flags)
            if i >= 40:
                tail.append(state.summary.log_likelihood)
        lls[kind] = np.mean(tail)
    assert abs(lls["cpu"] - lls["gpu"]) / abs(lls["cpu"]) < 0.03, lls


@gpu
def test_gpu_resume_deterministic(tmp_path):
    """Counter-based RNG makes the GPU chain a deterministic function of
    (seed, iteration, state): continuing from a saved state must reproduce
    the uninterrupted chain bitwise."""
    import bench as b
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.engine.state import ChainState
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    n = 400
    cache, rec_values, rec_files = b.build_cache_and_records(n, seed=31)
    flags = SamplerFlags.for_sampler("PCG-I")

    partitioner = KDTreePartitioner(1, [3])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=77)
    engine = GpuEngine(cache, partitioner, device=DEV)
    engine.initial_summary(state)
    for _ in range(4):
        engine.step(state, flags)
    engine.sync_state(state)
    out = str(tmp_path)
    state.save(out)
    for _ in range(3):
        engine.step(state, flags)
    engine.sync_state(state)

    state2 = ChainState.load(out)
    engine2 = GpuEngine(cache, partitioner, device=DEV)
    for _ in range(3):
        engine2.step(state2, flags)
    engine2.sync_state(state2)

    assert state2.iteration == state.iteration
    np.testing.assert_array_equal(np.sort(state2.rec_gid), np.sort(state.rec_gid))
    # compare per-record linked-entity VALUES keyed by gid (row order may differ)
    def linkmap(st):
        return {int(g): st.ent_values[st.rec_ent[i]].tolist()
                for i, g in enumerate(st.rec_gid)}
    assert linkmap(state2) == linkmap(state)


@gpu
@pytest.mark.parametrize("sampler", ["PCG-II", "Gibbs", "Gibbs-Sequential"])
def test_gpu_sampler_variants(sampler, tmp_path):
    """All four sampler variants run on the GPU with finite likelihoods and
    sane summary counts."""
    import bench as b
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    n = 300
    cache, rec_values, rec_files = b.build_cache_and_records(n, seed=8)
    partitioner = KDTreePartitioner(1, [3])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=5)
    engine = GpuEngine(cache, partitioner, device=DEV)
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(sampler)
    for _ in range(15):
        engine.step(state, flags)
    s = state.summary
    assert np.isfinite(s.log_likelihood)
    assert 0 <= s.num_isolates <= state.population_size
    assert s.rec_distortions.sum() == n
    engine.sync_state(state)
    assert state.rec_ent.min() >= 0 and state.rec_ent.max() < state.num_entities


@gpu
def test_gpu_project_pipeline(tmp_path):
    """Full user path on GPU: HOCON config -> Project -> sample/summarize/
    evaluate steps with engine 'auto' (selects the GPU engine)."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from test_end_to_end_cpu import CONF_TEMPLATE
    from dblink_amd.api.project import Project, parse_steps
    from dblink_amd.utils import hocon
    from dblink_amd.utils.synthdata import write_csv

    data = str(tmp_path / "data.csv")
    write_csv(data, 250, dup_fraction=0.1, seed=12)
    out = str(tmp_path / "results")
    conf = CONF_TEMPLATE.format(
        data=data, out=out, samples=30, burnin=20, thin=2, cutoff=30,
        sampler="PCG-I", levels=1, part_attrs='"fname_c1"',
    ).replace('engine : "cpu"', 'engine : "auto"')
    cfg = hocon.parse_string(conf)
    project = Project(cfg, rank=0, world_size=1)
    os.makedirs(project.output_path, exist_ok=True)
    for step in parse_steps(cfg, project):
        step.execute()
    from dblink_amd.engine.gpu_engine import GpuEngine

    assert isinstance(project.engine(), GpuEngine), "auto engine must pick the GPU"
    for f in ("diagnostics.csv", "evaluation-results.txt",
              "cluster-size-distribution.csv", "driver-state"):
        assert os.path.exists(os.path.join(out, f)), f
    import numpy as np
    with open(os.path.join(out, "diagnostics.csv")) as fh:
        fh.readline()
        ll = [float(line.split(",")[3]) for line in fh if line.strip()]
    assert len(ll) >= 30 and all(np.isfinite(ll))


TWO_RANK_GPU = r"""
import json, os, sys
sys.path.insert(0, "__ROOT__")
import numpy as np
import torch
import torch.distributed as dist

from dblink_amd.parallel import comm
from dblink_amd.parallel.partitioning import KDTreePartitioner
from dblink_amd.engine.init import deterministic_init
from dblink_amd.engine.cpu_engine import SamplerFlags
from dblink_amd.engine.gpu_engine import GpuEngine
import bench as b

rank, world, device = comm.init_from_env(backend="gloo")
device = torch.device("cuda", 0)  # both ranks share the single test GPU
n = 400
cache, rec_values, rec_files = b.build_cache_and_records(n, seed=17)
partitioner = KDTreePartitioner(2, [3, 4])
bounds = np.linspace(0, n, world + 1).astype(np.int64)
lo, hi = int(bounds[rank]), int(bounds[rank + 1])
state = deterministic_init(rec_values[lo:hi], rec_files[lo:hi],
                           np.arange(lo, hi, dtype=np.int64), cache, partitioner,
                           seed=3, rank=rank, world_size=world)
import copy
state_eager = copy.deepcopy(state)
engine = GpuEngine(cache, partitioner, world_size=world, rank=rank, device=device)
assert engine._overlap, "overlapped migration must be the default"
engine.initial_summary(state)
flags = SamplerFlags.for_sampler("PCG-I")
for i in range(12):
    engine.step(state, flags)
engine.sync_state(state)
assert np.all(state.ent_part % world == rank), "ownership violated"
assert np.isfinite(state.summary.log_likelihood)

# posterior parity: the overlapped path must replay the eager path bitwise
engine2 = GpuEngine(cache, partitioner, world_size=world, rank=rank, device=device)
engine2._overlap = False
engine2.initial_summary(state_eager)
for i in range(12):
    engine2.step(state_eager, flags)
engine2.sync_state(state_eager)
for f in ("ent_values", "ent_part", "rec_values", "rec_ent", "rec_dist", "rec_gid"):
    assert np.array_equal(getattr(state, f), getattr(state_eager, f)), f
assert state.summary.log_likelihood == state_eager.summary.log_likelihood
gids = comm.all_gather_object(sorted(state.rec_gid.tolist()))
t = torch.tensor([state.num_entities], dtype=torch.float64)
comm.all_reduce_sum_(t)
if rank == 0:
    allg = sorted(g for lst in gids for g in lst)
    assert allg == list(range(n)), "records lost in GPU migration"
    assert int(t[0]) == state.population_size
    print(json.dumps({"ok": True, "ll": state.summary.log_likelihood}))
dist.destroy_process_group()
"""


@gpu
def test_gpu_two_rank_chain():
    """Multi-rank GpuEngine integration: two processes share one GPU (gloo
    comm with device bridging) — exercises the eager multi-rank sweep,
    packed migration and the overlapped summary reduce on CUDA state."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = TWO_RANK_GPU.replace("__ROOT__", root)
    env = dict(os.environ)
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29731", WORLD_SIZE="2",
               GLOO_SOCKET_IFNAME="lo", LOCAL_RANK="0")
    procs = []
    for r in range(2):
        e = dict(env, RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, "-c", script], env=e,
                                      stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, out in zip(procs, outs):
        assert p.returncode == 0, f"worker failed:\n{out}"
    assert any('"ok": true' in o for o in outs), outs


@gpu
def test_gpu_missing_values_chain(tmp_path):
    """GPU chain over data with missing values (x = -1 flows through link
    candidate generation, k_obs counting, distortions and summaries)."""
    import bench as b
    from dblink_amd.engine.cpu_engine import SamplerFlags
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.models.records import RecordsCache, RecordsTable
    from dblink_amd.parallel.partitioning import KDTreePartitioner
    from dblink_amd.utils.synthdata import generate

    n = 400
    cols, _ = generate(n, dup_fraction=0.1, seed=23, missing_fraction=0.15)
    from dblink_amd.models.records import Attribute, BetaShapeParameters
    from dblink_amd.models.similarity import ConstantSimilarityFn, LevenshteinSimilarityFn

    attr_names = ["by", "bm", "bd", "fname_c1", "lname_c1"]
    columns = [np.where(cols[a] == "NA", None, cols[a]) for a in attr_names]
    table = RecordsTable(cols["rec_id"], cols["file_id"], columns)
    prior = BetaShapeParameters(0.5, 50.0)
    attrs = [
        Attribute("by", ConstantSimilarityFn(), prior),
        Attribute("bm", ConstantSimilarityFn(), prior),
        Attribute("bd", ConstantSimilarityFn(), prior),
        Attribute("fname_c1", LevenshteinSimilarityFn(7.0, 10.0), prior),
        Attribute("lname_c1", LevenshteinSimilarityFn(7.0, 10.0), prior),
    ]
    cache = RecordsCache.build(table, attrs, max_cluster_size=10)
    rec_values, rec_files = cache.transform_records(table)
    assert (rec_values < 0).any()

    partitioner = KDTreePartitioner(1, [3])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=2)
    engine = GpuEngine(cache, partitioner, device=DEV)
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler("PCG-I")
    for _ in range(20):
        engine.step(state, flags)
    assert np.isfinite(state.summary.log_likelihood)
    engine.sync_state(state)
    # missing values never mutate: align the state's missing mask by gid
    aligned = np.zeros_like(rec_values, dtype=bool)
    aligned[state.rec_gid] = state.rec_values < 0
    np.testing.assert_array_equal(aligned, rec_values < 0)


@gpu
def test_value_kernel_large_cluster_rare_path():
    """k_obs > Kc: the cached power tables don't cover the cluster size, so
    the kernel computes log Z_k by wave reduction and draws the base via a
    dense Gumbel scan (GibbsUpdates.scala computes the distribution on
    demand). Empirical frequencies vs exact fp64 mixture probabilities."""
    cache, model = make_model(DEV, Kc=3)  # force the rare path at k > 3
    a = 1
    ia = cache.indexed_attributes[a]
    idx = ia.index
    V = idx.num_values
    x = 1
    k = 5  # > Kc
    theta = np.array([[0.05], [0.08]])
    model.theta.copy_(torch.from_numpy(theta).float())
    E = 30000
    # each entity linked to k identical observed records
    rec_values = np.tile(np.array([[3, x]], dtype=np.int32), (E * k, 1))
    rec_dist = np.ones((E * k, 2), dtype=np.uint8)
    ent_vals = np.zeros((E, 2), dtype=np.int32)
    ent_rec_ptr = (np.arange(E + 1, dtype=np.int64) * k)
    ent_rec_idx = np.arange(E * k, dtype=np.int64)

    # exact distribution: base = phi * norm^k / Z_k; pert factors multiply
    # across the k records (identical rows)
    base_w = idx.probs * idx.sim_norms ** k
    Zk = base_w.sum()
    base = base_w / Zk
    th = 0.08
    px = idx.probability_of(x)
    normx = idx.sim_norms[x]
    cols, sims = idx.sim_index.row(x)
    w = np.zeros(V)
    for v, es in zip(cols.tolist(), sims.tolist()):
        f = es + (1 / th - 1) / (px * normx) if v == x else es
        w[v] = base[v] * (f ** k - 1.0)
    W = w.sum()
    exact = (base + w) / (1.0 + W)

    ev = _dev(ent_vals, torch.int32)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    kobs = torch.zeros(E * 2, dtype=torch.int32, device=DEV)
    kobs.view(E, 2)[:, a] = k
    # only attr `a` pairs are active (attr 0 stays k=0 -> phi draw, ignored)
    C.value_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(E * k, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64),
        ev, model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 999, 4, 0, err,
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        torch.empty(0, dtype=torch.int64, device=DEV),
        model.csr_excl, model.csr_rawsum, model.z1,
        torch.empty(0, dtype=torch.int64, device=DEV),
        kobs,
    )
    got = ev.cpu().numpy()[:, a]
    emp = np.bincount(got, minlength=V) / E
    assert tv_distance(emp, exact) < 0.025, (emp[:8], exact[:8])


@gpu
def test_link_kernel_parity_on_realistic_state():
    """Link-update conditionals on a REAL mid-chain state: evolve a CPU chain,
    freeze its entity table, then for records with diverse patterns (missing
    values, distorted names, multiple candidates) compare GPU empirical
    selection frequencies against the exact fp64 conditional probabilities
    computed with the CPU oracle's code path."""
    import bench as b
    from dblink_amd.engine.cpu_engine import (
        CpuEngine,
        SamplerFlags,
        _build_inverted_index,
        _get_possible_entities,
    )
    from dblink_amd.engine.gpu_engine import GpuModel
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    n = 250
    cache, rec_values, rec_files = b.build_cache_and_records(n, seed=71)
    partitioner = KDTreePartitioner(0, [])
    state = deterministic_init(rec_values, rec_files, np.arange(n, dtype=np.int64),
                               cache, partitioner, seed=8)
    engine = CpuEngine(cache, partitioner)
    engine.initial_summary(state)
    for _ in range(15):
        engine.step(state, SamplerFlags.for_sampler("PCG-I"))

    attrs = cache.indexed_attributes
    A = len(attrs)
    E = state.num_entities
    inv = _build_inverted_index(state.ent_values)

    def exact_probs(rv, rd):
        cands, obs_dist = _get_possible_entities(rv, rd, inv, E, None)
        w = np.ones(len(cands))
        for a in obs_dist:
            ia = attrs[a]
            if ia.is_constant:
                continue
            x = int(rv[a])
            y = state.ent_values[cands, a]
            w *= ia.index.sim_norms[y] * np.array(
                [ia.index.exp_sim_of(x, int(yy)) for yy in y]
            )
        return cands, w / w.sum()

    # At the frozen stationary state every record resolves to a singleton
    # candidate set (a vacuous check), so craft the distortion-indicator
    # input: keep exactly one attribute non-distorted (candidates = that
    # value's posting list, weights from BOTH Levenshtein attrs), plus one
    # all-distorted case exercising the nd_n==0 whole-partition scan.
    picks = []
    for r, keep in ((5, 1), (17, 2), (42, 3)):
        rv = state.rec_values[r]
        assert rv[keep] >= 0
        rd = np.ones(A, dtype=bool)
        rd[keep] = False
        cands, p = exact_probs(rv, rd)
        assert len(cands) >= 2
        picks.append((r, rv, rd, cands, p))
    rv = state.rec_values[7]
    rd = np.ones(A, dtype=bool)
    cands, p = exact_probs(rv, rd)
    assert len(cands) == E
    picks.append((7, rv, rd, cands, p))

    model = GpuModel(cache, DEV, 10)
    N = 20000
    for r, rv, rd, cands, exact in picks:
        rec_v = np.tile(rv, (N, 1)).astype(np.int32)
        rec_d = np.tile(rd, (N, 1)).astype(np.uint8)
        # posting build identical to the engine (slot-major keys)
        keys = ((0 * A + np.repeat(np.arange(A), E)) * model.Vmax
                + state.ent_values.T.reshape(-1)).astype(np.int64)
        order = np.argsort(keys, kind="stable")
        sorted_keys = keys[order]
        postings = (order % E).astype(np.int32)
        qk = np.array([(0 * A + a) * model.Vmax + max(int(rv[a]), 0)
                       for a in range(A)], dtype=np.int64)
        lo = np.searchsorted(sorted_keys, qk, "left")
        hi = np.searchsorted(sorted_keys, qk, "right")
        out = torch.empty(N, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        C.link_update(
            _dev(rec_v, torch.int32), _dev(rec_d, torch.uint8),
            _dev(np.arange(N, dtype=np.int64), torch.int64),
            _dev(np.zeros(N, np.int32), torch.int32),
            _dev(np.tile(lo, (N, 1)), torch.int64), _dev(np.tile(hi, (N, 1)), torch.int64),
            _dev(postings, torch.int32), _dev(state.ent_values, torch.int32),
            _dev(np.array([0, E], dtype=np.int64), torch.int64),
            model.log_norm, model.voff, model.csr_row_ptr, model.csr_col,
            model.csr_sim, model.attr_const, 9090, 2, out,
            _dev(np.zeros(N, np.int64), torch.int64), err,
            torch.empty(0, dtype=torch.uint8, device=DEV),
            torch.empty(0, dtype=torch.int64, device=DEV),
            torch.empty(0, dtype=torch.int32, device=DEV),
            torch.empty(0, dtype=torch.int32, device=DEV),
        )
        assert int(err.cpu()) == 0
        sel = out.cpu().numpy()
        emp = np.zeros(E)
        np.add.at(emp, sel, 1.0 / N)
        full = np.zeros(E)
        full[cands] = exact
        # multinomial sampling noise: E[TV] ~ 0.5 * sum sqrt(p(1-p)/N)
        noise = 0.5 * np.sum(np.sqrt(full * (1 - full) / N))
        assert tv_distance(emp, full) < 3 * noise + 0.01, (
            r, tv_distance(emp, full), noise, emp[cands][:6], exact[:6]
        )


def _link_paths_inputs(n_vals, seed=3, E=600, R=512):
    """Pure-numpy inputs for the wave/thread agreement test: E entities in one
    partition, R records copied from random entities and perturbed into five
    kinds (attr 0 = constant 'year', attr 1 = Levenshtein 'name'):
      0 year non-distorted, name distorted     (the only kind with an od attr)
      1 name non-distorted, year distorted
      2 both non-distorted
      3 year missing, name non-distorted
      4 name missing, year non-distorted
    Kind 0 takes 6 records in 10 so most records score a real od log-weight.
    Returns the arrays plus, per record, the number of entities passing the
    equality checks and whether od_mask is non-empty."""
    rng = np.random.default_rng(seed)
    A = len(n_vals)
    Vmax = max(n_vals)
    ent_values = np.stack([rng.integers(0, v, size=E) for v in n_vals], 1).astype(np.int32)
    kind = np.array([0, 0, 0, 0, 0, 0, 1, 2, 3, 4])[np.arange(R) % 10]
    rec_values = ent_values[rng.integers(0, E, size=R)].copy()
    rec_dist = np.zeros((R, A), dtype=np.uint8)
    k0, k1 = kind == 0, kind == 1
    rec_dist[k0, 1] = 1
    rec_values[k0, 1] = rng.integers(0, n_vals[1], size=k0.sum())
    rec_dist[k1, 0] = 1
    rec_values[k1, 0] = rng.integers(0, n_vals[0], size=k1.sum())
    rec_values[kind == 3, 0] = -1
    rec_values[kind == 4, 1] = -1

    # posting build identical to the engine (slot-major keys, one partition)
    keys = (np.repeat(np.arange(A), E) * Vmax + ent_values.T.reshape(-1)).astype(np.int64)
    order = np.argsort(keys, kind="stable")
    postings = (order % E).astype(np.int32)
    qk = np.arange(A)[None, :] * Vmax + np.maximum(rec_values, 0)
    cand_lo = np.searchsorted(keys[order], qk, "left")
    cand_hi = np.searchsorted(keys[order], qk, "right")

    nd = (rec_values >= 0) & (rec_dist == 0)
    match = ((ent_values[None] == rec_values[:, None]) | ~nd[:, None]).all(2)
    has_od = (rec_values[:, 1] >= 0) & (rec_dist[:, 1] == 1)  # attr 0 is constant
    return dict(ent_values=ent_values, rec_values=rec_values, rec_dist=rec_dist,
                kind=kind, postings=postings, cand_lo=cand_lo, cand_hi=cand_hi,
                nd=nd, n_match=match.sum(1), has_od=has_od)


@gpu
def test_link_wave_and_thread_paths_agree_bitwise(monkeypatch):
    """Routing a record to the wave or the thread link kernel is a performance
    decision, and LDS sim-row staging is an optimisation: all three must draw
    the SAME entity for every record. Identical inputs, seed and iteration
    through (a) the wave path, (b) the thread path, (c) the wave path with
    staging off; outputs must be torch.equal. Year postings hold ~60 entities,
    so staging engages in (a); every record has an observed non-distorted
    attribute, as the thread kernel's routing guarantees."""
    cache, model = make_model(DEV)
    n_vals = [ia.index.num_values for ia in cache.indexed_attributes]
    d = _link_paths_inputs(n_vals)
    E, R = d["ent_values"].shape[0], d["rec_values"].shape[0]

    # the check must not be vacuous
    assert d["nd"].any(1).all()
    assert (d["n_match"] >= 1).all()
    assert ((d["n_match"] >= 2) & d["has_od"]).sum() >= R // 2
    assert set(d["kind"].tolist()) == {0, 1, 2, 3, 4}
    year_nd = d["nd"][:, 0]
    assert ((d["cand_hi"] - d["cand_lo"])[year_nd, 0] >= 32).all()

    args_head = (
        _dev(d["rec_values"], torch.int32), _dev(d["rec_dist"], torch.uint8),
        _dev(np.arange(R, dtype=np.int64), torch.int64),
        _dev(np.zeros(R, np.int32), torch.int32),
        _dev(d["cand_lo"], torch.int64), _dev(d["cand_hi"], torch.int64),
        _dev(d["postings"], torch.int32), _dev(d["ent_values"], torch.int32),
        _dev(np.array([0, E], dtype=np.int64), torch.int64),
        model.log_norm, model.voff, model.csr_row_ptr, model.csr_col,
        model.csr_sim, model.attr_const, 4242, 7,
    )
    rec_ent_in = _dev(np.zeros(R, np.int64), torch.int64)
    no_pairs = torch.empty(0, dtype=torch.int32, device=DEV)

    def run(small_mask):
        out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        C.link_update(*args_head, out, rec_ent_in, err, small_mask,
                      torch.empty(0, dtype=torch.int64, device=DEV),
                      no_pairs, no_pairs)
        assert int(err.cpu()) == 0
        return out

    wave = run(torch.empty(0, dtype=torch.uint8, device=DEV))
    thread = run(torch.ones(R, dtype=torch.uint8, device=DEV))
    monkeypatch.setenv("DBLINK_SIMH", "0")  # re-read per launch; restored on exit
    wave_global = run(torch.empty(0, dtype=torch.uint8, device=DEV))

    assert torch.equal(wave, thread)
    assert torch.equal(wave, wave_global)
    sel = wave.cpu().numpy()
    assert (sel >= 0).all() and (sel < E).all()
    # every draw is a legal candidate (equal on all non-distorted attrs)
    assert ((d["ent_values"][sel] == d["rec_values"]) | ~d["nd"]).all()


@gpu
def test_link_heavy_kernel_distribution():
    """Hierarchical A* link sampler (link_update_heavy_kernel) vs exact
    weights: class-U records (no non-distorted attr -> pool = whole
    partition) and single-nd records (one big posting range). The sampler
    must draw the same categorical as the scan path
    (GibbsUpdates.scala:398-430), in O(|similar set| + tens) work."""
    cache, model = make_model(DEV)
    ia = cache.indexed_attributes[1]
    idx = ia.index
    rng = np.random.default_rng(7)
    E = 1500
    ent_vals = np.zeros((E, 2), dtype=np.int32)
    ent_vals[:800, 0] = 3                       # posting(year=3) = 800 > 512
    ent_vals[800:, 0] = rng.integers(0, 3, E - 800)
    ent_vals[:, 1] = rng.integers(0, idx.num_values, E).astype(np.int32)

    A, T, Vmax = 2, 2, model.Vmax
    nk = 1 * T * Vmax
    keys = ((np.repeat([0, 1], E)) * Vmax + ent_vals.T.reshape(-1)).astype(np.int64)
    counts = np.bincount(keys, minlength=nk)
    idx_ptr = np.zeros(nk + 1, dtype=np.int64)
    idx_ptr[1:] = np.cumsum(counts)
    order = np.argsort(keys, kind="stable")
    postings = (order % E).astype(np.int32)

    x = 0  # record's (distorted) name value
    for case, dist_row, rec_row in (
        ("classU", [1, 1], [3, x]),      # no nd attr: pool = all entities
        ("single-nd", [0, 1], [3, x]),   # nd = {year}: base = posting(year=3)
    ):
        N = 40000
        rec_values = np.tile(np.array([rec_row], dtype=np.int32), (N, 1))
        rec_dist = np.tile(np.array([dist_row], dtype=np.uint8), (N, 1))
        w = np.array([
            idx.sim_norms[y] * idx.exp_sim_of(x, int(y)) for y in ent_vals[:, 1]
        ])
        if case == "single-nd":
            w = w * (ent_vals[:, 0] == 3)
        exact = w / w.sum()

        qk = np.array([0 * Vmax + rec_row[0], 1 * Vmax + x], dtype=np.int64)
        cand_lo = np.tile(idx_ptr[qk], (N, 1)).astype(np.int64)
        cand_hi = np.tile(idx_ptr[qk + 1], (N, 1)).astype(np.int64)

        mode = torch.empty(N, dtype=torch.uint8, device=DEV)
        ent_ptr = _dev(np.array([0, E], dtype=np.int64), torch.int64)
        rec_part = _dev(np.zeros(N, np.int32), torch.int32)
        rv = _dev(rec_values, torch.int32)
        rd = _dev(rec_dist, torch.uint8)
        C.classify_modes(rv, rd, rec_part, ent_ptr,
                         _dev(cand_lo, torch.int64), _dev(cand_hi, torch.int64),
                         0, 16, 512, mode)
        assert int(mode.to(torch.int64).min().cpu()) == 2, case

        out = torch.empty(N, dtype=torch.int64, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        stats = torch.zeros(4, dtype=torch.int64, device=DEV)
        C.link_update_heavy(
            mode, rv, rd,
            _dev(np.arange(N, dtype=np.int64), torch.int64), rec_part,
            _dev(ent_vals, torch.int32), ent_ptr,
            model.log_norm, model.voff, model.csr_row_ptr, model.csr_col,
            model.csr_sim, model.attr_const,
            model.csr_row_ptr_big, model.csr_col_big, model.csr_sim_big,
            model.heavy_tau,
            _dev(postings, torch.int32), _dev(idx_ptr, torch.int64),
            Vmax, 0, 4321, 11, torch.empty(0, dtype=torch.int64, device=DEV),
            out, _dev(np.zeros(N, np.int64), torch.int64), err, stats)
        assert int(err.cpu()) == 0, case
        sel = out.cpu().numpy()
        emp = np.bincount(sel, minlength=E) / N
        # per-entity TV at 1500 cells is dominated by multinomial noise
        # (~0.033 even for a perfect sampler at N=40000); entities sharing a
        # (year-match, name-value) profile are exchangeable, so aggregate
        # onto those groups where the noise floor is negligible
        group = ent_vals[:, 1].astype(np.int64) * 2 + (ent_vals[:, 0] == 3)
        ng = int(group.max()) + 1
        emp_g = np.bincount(group, weights=emp, minlength=ng)
        exact_g = np.bincount(group, weights=exact, minlength=ng)
        assert tv_distance(emp_g, exact_g) < 0.01, (case, tv_distance(emp_g, exact_g))
        st = stats.cpu().numpy()
        # the whole point: few A* iterations per record, no fallback storms
        assert st[0] / N < 100, ("A* iterations per record too high", st)
        assert st[1] / N < 0.01, ("too many full-scan fallbacks", st)


@gpu
def test_mfma_scorer_matches_scalar():
    """MFMA one-hot categorical scorer vs the LDS scalar scorer: identical
    scores up to bf16 truncation (the VERDICT #4 experiment's correctness
    gate; see scripts/mfma_experiment.py and profiles/README.md)."""
    rng = np.random.default_rng(3)
    R, E = 256, 512
    VS = [100, 12, 28]
    BASE = np.cumsum([0] + VS)[:3]
    K = ((sum(VS) + 31) // 32) * 32
    rcode = np.stack([rng.integers(0, v, R) + b for v, b in zip(VS, BASE)], 1)
    ecode = np.stack([rng.integers(0, v, E) + b for v, b in zip(VS, BASE)], 1)
    rbonus = rng.uniform(1.0, 12.0, (R, 3))
    t_rc = _dev(rcode, torch.int32)
    t_ec = _dev(ecode, torch.int32)
    t_rb = _dev(rbonus, torch.float32)
    s1 = torch.empty((R, E), dtype=torch.float32, device=DEV)
    s2 = torch.empty((R, E), dtype=torch.float32, device=DEV)
    C.scalar_score_bench(t_rc, t_rb, t_ec, s1)
    C.mfma_score_bench(t_rc, t_rb, t_ec, K, s2)
    # oracle in numpy
    want = ((rcode[:, None, :] == ecode[None, :, :]) * rbonus[:, None, :]).sum(2)
    np.testing.assert_allclose(s1.cpu().numpy(), want, rtol=1e-6)
    np.testing.assert_allclose(s2.cpu().numpy(), want, rtol=2 ** -7, atol=0.1)


@gpu
def test_value_kd1_kernel_distribution():
    """k=2 single-shared-value clusters (the kd1 table path): empirical value
    frequencies vs the exact mixture P(v) = (base2(v) + w(v)) / (1 + W) with
    w(v) = base2(v) (f(v)^2 - 1), f(x) boosted by the collapsed self term."""
    cache, model = make_model(DEV)
    assert model.ktab_max >= 2
    a = 1
    ia = cache.indexed_attributes[a]
    idx = ia.index
    x = 0
    th = 0.1
    model.theta.copy_(torch.full((2, 1), th))
    N = 40000
    # N entities, each with two linked records of value x (file 0)
    rec_values = np.tile(np.array([[-1, x]], dtype=np.int32), (2 * N, 1))
    rec_dist = np.ones((2 * N, 2), dtype=np.uint8)
    ent_vals = np.zeros((N, 2), dtype=np.int32)
    ent_rec_ptr = np.arange(0, 2 * N + 1, 2, dtype=np.int64)
    ent_rec_idx = np.arange(2 * N, dtype=np.int64)
    kobs = np.zeros((N, 2), dtype=np.int32)
    kobs[:, a] = 2

    C.set_value_ktables(model.ktab_excl, model.ktab_rawsum, model.self_expsim,
                        model.ktab_max, int(model.csr_col.numel()))
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ev = _dev(ent_vals, torch.int32)
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    C.value_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(2 * N, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64), ev,
        model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 777, 5, 0, err, empty64, empty64, empty64,
        model.csr_excl, model.csr_rawsum, model.z1, empty64,
        _dev(kobs.reshape(-1), torch.int32))
    sel = ev.cpu().numpy()[:, a]

    V = idx.num_values
    phi = idx.probs
    norms = idx.sim_norms
    z2 = idx.sim_norm_total(2)
    base2 = phi * norms ** 2 / z2
    w = np.zeros(V)
    si = idx.sim_index
    se = (1.0 / th - 1.0) / (phi[x] * norms[x])
    for j in range(si.row_ptr[x], si.row_ptr[x + 1]):
        c = si.col[j]
        f = si.expsim[j] + (se if c == x else 0.0)
        w[c] = base2[c] * (f * f - 1.0)
    W = w.sum()
    exact = (base2 + w) / (1.0 + W)
    emp = np.bincount(sel, minlength=V) / N
    assert tv_distance(emp, exact) < 0.02, tv_distance(emp, exact)
    # reset globals so later direct-kernel tests see a clean slate
    z = torch.empty(0, dtype=torch.float64)
    C.set_value_ktables(z, z, torch.empty(0, dtype=torch.float32), 0, 0)


@gpu
def test_value_kd2_kernel_distribution():
    """k=2 clusters with TWO distinct values (the kd2 table path): empirical
    frequencies vs the exact mixture with w(v) = base2(v) (F1 F2 - 1),
    F_i boosted by the collapsed self term at v = x_i."""
    import os

    os.environ["DBLINK_KTAB2"] = "1"  # experiment tables are off by default
    try:
        cache, model = make_model(DEV)
    finally:
        os.environ.pop("DBLINK_KTAB2", None)
    assert model.k2tab_max >= 2
    a = 1
    idx = cache.indexed_attributes[a].index
    x1, x2 = 0, 1
    th = 0.1
    model.theta.copy_(torch.full((2, 1), th))
    N = 40000
    rec_values = np.tile(np.array([[-1, x1], [-1, x2]], dtype=np.int32), (N, 1))
    rec_dist = np.ones((2 * N, 2), dtype=np.uint8)
    ent_vals = np.zeros((N, 2), dtype=np.int32)
    ent_rec_ptr = np.arange(0, 2 * N + 1, 2, dtype=np.int64)
    ent_rec_idx = np.arange(2 * N, dtype=np.int64)
    kobs = np.zeros((N, 2), dtype=np.int32)
    kobs[:, a] = 2

    C.set_value_ktables(model.ktab_excl, model.ktab_rawsum, model.self_expsim,
                        model.ktab_max, int(model.csr_col.numel()))
    C.set_value_k2tables(model.k2tab_excl, model.k2tab_rawsum, model.k2tab_max)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ev = _dev(ent_vals, torch.int32)
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    C.value_update(
        _dev(rec_values, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(2 * N, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64), ev,
        model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 909, 4, 0, err, empty64, empty64, empty64,
        model.csr_excl, model.csr_rawsum, model.z1, empty64,
        _dev(kobs.reshape(-1), torch.int32))
    sel = ev.cpu().numpy()[:, a]

    V = idx.num_values
    phi = idx.probs
    norms = idx.sim_norms
    z2 = idx.sim_norm_total(2)
    base2 = phi * norms ** 2 / z2
    F1 = np.ones(V)
    F2 = np.ones(V)
    si = idx.sim_index
    for x, F, se in ((x1, F1, (1/th - 1)/(phi[x1]*norms[x1])),
                     (x2, F2, (1/th - 1)/(phi[x2]*norms[x2]))):
        for j in range(si.row_ptr[x], si.row_ptr[x + 1]):
            c = si.col[j]
            F[c] = si.expsim[j] + (se if c == x else 0.0)
    w = base2 * (F1 * F2 - 1.0)
    W = w.sum()
    exact = (base2 + w) / (1.0 + W)
    emp = np.bincount(sel, minlength=V) / N
    assert tv_distance(emp, exact) < 0.02, tv_distance(emp, exact)
    z = torch.empty(0, dtype=torch.float64)
    C.set_value_ktables(z, z, torch.empty(0, dtype=torch.float32), 0, 0)
    C.set_value_k2tables(z, z, 0)


@functools.lru_cache(maxsize=None)
def _mutation_ball_model():
    """(cache, model) over a 650-name mutation ball at threshold 7: every pair
    within edit distance 4, so sim rows are ~V long (609 rows of 262-384
    entries, 41 of 650). Built once per session (the pure-Python pair sweep
    takes ~11 s); callers must not modify the returned model."""
    rng = np.random.default_rng(11)
    base = list("ABCABCABCA")
    pool = set()
    while len(pool) < 650:
        s = base.copy()
        for _ in range(rng.integers(1, 3)):
            s[rng.integers(0, 10)] = "ABCDE"[rng.integers(0, 5)]
        pool.add("".join(s))
    return make_model(DEV, threshold=7.0, names=sorted(pool))


@gpu
def test_value_dense_merge_distribution():
    """k=2 clusters over TWO distinct values whose sim rows overflow the LDS
    hash (total entries > 3/4 * HASH_CAP): exercises the chunked
    hash-accumulate dense path of value_update_kernel_t<2>. Empirical value
    frequencies vs the exact fp64 mixture (GibbsUpdates.scala:533-570):
    w(v) = base2(v) * (f_x1(v) * f_x2(v) - 1), f_x(x) boosted by the
    collapsed self term."""
    cache, model = _mutation_ball_model()
    a = 1
    idx = cache.indexed_attributes[a].index
    V = idx.num_values
    si = idx.sim_index
    row_lens = np.diff(si.row_ptr)
    x2i, x1i = np.argsort(row_lens)[-2:]
    x1, x2 = int(x1i), int(x2i)
    assert x1 != x2
    # the dense path must actually engage (HASH_CAP = 1024 in kernels.hip)
    assert row_lens[x1] + row_lens[x2] > (1024 * 3) // 4, (
        row_lens[x1], row_lens[x2])

    th = 0.1
    theta = torch.full((2, 1), th, dtype=torch.float32, device=DEV)
    N = 80000
    # N entities, each with one record of value x1 and one of x2 (file 0)
    rv = np.full((2 * N, 2), -1, dtype=np.int32)
    rv[0::2, a] = x1
    rv[1::2, a] = x2
    rec_dist = np.ones((2 * N, 2), dtype=np.uint8)
    ent_vals = np.zeros((N, 2), dtype=np.int32)
    ent_rec_ptr = np.arange(0, 2 * N + 1, 2, dtype=np.int64)
    ent_rec_idx = np.arange(2 * N, dtype=np.int64)
    kobs = np.zeros((N, 2), dtype=np.int32)
    kobs[:, a] = 2

    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ev = _dev(ent_vals, torch.int32)
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    C.value_update(
        _dev(rv, torch.int32), _dev(rec_dist, torch.uint8),
        _dev(np.zeros(2 * N, np.int32), torch.int32),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64), ev,
        theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, 4242, 9, 0, err, empty64, empty64, empty64,
        model.csr_excl, model.csr_rawsum, model.z1, empty64,
        _dev(kobs.reshape(-1), torch.int32))
    sel = ev.cpu().numpy()[:, a]

    phi = idx.probs
    norms = idx.sim_norms
    z2 = idx.sim_norm_total(2)
    base2 = phi * norms ** 2 / z2
    L = np.zeros(V)
    for x in (x1, x2):
        se = (1.0 / th - 1.0) / (phi[x] * norms[x])
        for j in range(si.row_ptr[x], si.row_ptr[x + 1]):
            c = si.col[j]
            f = si.expsim[j] + (se if c == x else 0.0)
            L[c] += np.log(f)
    w = base2 * np.expm1(L)
    W = w.sum()
    exact = (base2 + w) / (1.0 + W)
    emp = np.bincount(sel, minlength=V) / N
    assert tv_distance(emp, exact) < 0.05, tv_distance(emp, exact)


@gpu
def test_value_pairlist_and_kobs_paths_agree_bitwise(monkeypatch):
    """Explicit pair-list mode (value_update_kernel_t<0>) and kobs
    self-selection mode (kernel_t<1>, kernel_t<2>, value_base_draw_kernel)
    run one value_update_pair body on every k >= 2 pair and draw k = 0 pairs
    from phi under one Philox tag, so with the k-tables cleared and no k = 1
    pair the two modes must return identical ent_values. Seven pair classes
    of 64 entities route through every k >= 2 path: (a) d=1 hash, (b) d=2
    hash, (c) two 650-entry rows (dense), (d) three short rows (dense),
    (e) one value in two files (two groups), (f) 17 distinct rows (more than
    VAL_DMAX groups and k > Kc), (g) k = 0. Checked at DBLINK_VCHUNK=1
    (chunked hash) and 0 (union merge); the two settings sum W in different
    orders and need not agree with each other. 64 draws per class over
    ~300-1300 support values are far too few for a frequency comparison
    within multinomial noise, so union-merge correctness rests on this
    bitwise check plus the distribution tests above."""
    cache, model = _mutation_ball_model()
    z = torch.empty(0, dtype=torch.float64)
    C.set_value_ktables(z, z, torch.empty(0, dtype=torch.float32), 0, 0)
    C.set_value_k2tables(z, z, 0)

    A, a, NC = 2, 1, 64
    row_lens = np.diff(cache.indexed_attributes[a].index.sim_index.row_ptr)
    order = np.argsort(row_lens, kind="stable")
    short = order[row_lens[order] < 650]
    long_ = order[row_lens[order] == 650]
    assert len(short) >= NC + 17 and len(long_) >= 2

    # per class: entity i -> list of (name value, file)
    classes = {
        "a": lambda i: [(short[i], 0)] * 2,
        "b": lambda i: [(short[i], 0), (short[i + 1], 0)],
        "c": lambda i: [(long_[i % len(long_)], 0), (long_[(i + 1) % len(long_)], 0)],
        "d": lambda i: [(short[i + j], 0) for j in range(3)],
        "e": lambda i: [(short[i], 0), (short[i], 1)],
        "f": lambda i: [(short[i + j], 0) for j in range(17)],
        "g": lambda i: [],
    }
    rv, rf, ptr, entries, cls_of = [], [], [0], [], []
    for name, recs_of in classes.items():
        for i in range(NC):
            recs = recs_of(i)
            for j, (x, f) in enumerate(recs):
                rv.append([(len(ptr) + j) % 10, int(x)])  # both attributes observed
                rf.append(f)
            ptr.append(len(rv))
            # the kernel's total_entries: one row per distinct (value, file) group
            entries.append(sum(int(row_lens[x]) for x, f in set(recs)))
            cls_of.append(name)
    E, R = len(cls_of), len(rv)
    entries, cls_of = np.array(entries), np.array(cls_of)
    kobs = np.repeat(np.diff(ptr), A).astype(np.int32)  # [E*A]
    # non-vacuity (HASH_CAP = 1024: the hash path holds <= 768 entries)
    assert (entries[np.isin(cls_of, ["a", "b", "e"])] <= 768).all()
    assert (entries[np.isin(cls_of, ["a", "b", "e"])] > 0).all()
    assert (entries[np.isin(cls_of, ["c", "d", "f"])] > 768).all()
    assert not (kobs == 1).any()
    assert (kobs[cls_of.repeat(A) == "f"] > model.Kc).all()

    theta = _dev(np.array([[0.05, 0.2], [0.1, 0.3]]), torch.float32)  # [A, F=2]
    t_rv = _dev(np.array(rv, dtype=np.int32).reshape(R, A), torch.int32)
    t_rd = torch.ones((R, A), dtype=torch.uint8, device=DEV)
    t_rf = _dev(np.array(rf, dtype=np.int32), torch.int32)
    t_ptr = _dev(np.array(ptr, dtype=np.int64), torch.int64)
    t_idx = torch.arange(R, dtype=torch.int64, device=DEV)
    empty64 = torch.empty(0, dtype=torch.int64, device=DEV)
    all_pairs = torch.arange(E * A, dtype=torch.int64, device=DEV)
    no_kobs = torch.empty(0, dtype=torch.int32, device=DEV)
    t_kobs = _dev(kobs, torch.int32)

    def run(wave_pairs, kobs_t):
        ev = torch.zeros((E, A), dtype=torch.int32, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        C.value_update(
            t_rv, t_rd, t_rf, t_ptr, t_idx, ev,
            theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
            model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
            model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
            model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
            1, 0, 2718, 3, 0, err, wave_pairs, empty64, empty64,
            model.csr_excl, model.csr_rawsum, model.z1, empty64, kobs_t)
        torch.cuda.synchronize()
        return ev.cpu()

    for vchunk in ("1", "0"):
        monkeypatch.setenv("DBLINK_VCHUNK", vchunk)
        by_list = run(all_pairs, no_kobs)
        by_kobs = run(empty64, t_kobs)
        differ = (by_list != by_kobs).any(dim=1).numpy()
        print(f"DBLINK_VCHUNK={vchunk}: differing entities per class",
              {c: int(differ[cls_of == c].sum()) for c in classes},
              "nonzero fraction", float((by_list != 0).float().mean()))
        assert torch.equal(by_list, by_kobs), (vchunk, sorted(set(cls_of[differ])))
        assert (by_list != 0).float().mean() > 0.5
        assert (by_kobs != 0).float().mean() > 0.5
