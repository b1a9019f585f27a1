"""The dense link kernel (PCG-II and Gibbs-Sequential), the Gibbs-Sequential
value kernel, the log-likelihood fused into the distortion kernel and the
integer outputs of ``summary_counts``, each against a plain reference.

The sampling kernels are checked as ``test_gpu`` checks the others: many
replicas of one configuration in one launch, empirical frequencies against
exact fp64 probabilities (``kernel_refs``, held to the per-record CPU oracle
in ``test_kernel_refs``). Bounds are not hand-picked: for each class the test
draws 200 multinomial samples of its own size from the exact probabilities,
takes the largest total-variation distance among them and multiplies by 1.5
(``kernel_refs.calibrated_bound``); the reference maxima and bounds this
gives are written at the assertions.
"""

import numpy as np
import pytest

import kernel_refs as kr
from test_gpu import _dev, _mutation_ball_model, make_model

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)


def _empty(dtype):
    return torch.empty(0, dtype=dtype, device=DEV)


def _model_tail(model):
    return (model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
            model.attr_const)


# ---- dense link kernel -------------------------------------------------------------

# theta[a, f]: four distinct values, so a transposed or file-blind index shows
THETA = np.array([[0.30, 0.55], [0.45, 0.15]])
# one partition shorter than a wave, one of 70 (second stride: 6 live lanes),
# one of 128 (two full strides)
ENT_PTR = np.array([0, 5, 75, 203], dtype=np.int64)
N_LINK = 30000

# (rec_values [year, name], rec_file, partition); names sort to
# ANNA, ANNAH, ANNE, BOB, BORB, CLAIR, CLAIRE, DAVE = 0..7
COLLAPSED_CLASSES = [
    ("both observed, file 0", [3, 0], 0, 0),
    ("both observed, file 1", [4, 2], 1, 1),
    ("name missing", [6, -1], 1, 2),
    ("year missing", [-1, 1], 0, 1),
]
# (rec_values, rec_dist, partition)
SEQ_CLASSES = [
    ("name distorted, year held", [4, 2], [0, 1], 1),
    ("both distorted", [3, 0], [1, 1], 0),
    ("year distorted, name held", [6, 5], [1, 0], 2),
    ("name missing, year held", [4, -1], [0, 1], 1),
]


def _dense_entities():
    """203 entities over 10 years x 8 names. The five of partition 0 are set
    by hand; (4, 2) in partition 1 and (6, 5) in partition 2 make every
    Gibbs-Sequential class feasible in its partition."""
    rng = np.random.default_rng(17)
    ev = np.stack([rng.integers(0, 10, 203), rng.integers(0, 8, 203)], 1).astype(np.int32)
    ev[:5] = [[3, 0], [3, 1], [4, 0], [4, 2], [5, 3]]
    ev[5] = [4, 2]
    ev[75] = [6, 5]
    return ev


def _dense_records(classes, collapsed):
    """Class k on records k, k + 4, ...; one record more than 4 N, so the
    last block is partial."""
    R = 4 * N_LINK + 1
    kind = np.arange(R) % 4
    rv = np.array([c[1] for c in classes], dtype=np.int32)[kind]
    if collapsed:
        rd = np.zeros((R, 2), dtype=np.uint8)  # not read
        rf = np.array([c[2] for c in classes], dtype=np.int32)[kind]
        part = np.array([c[3] for c in classes], dtype=np.int32)[kind]
    else:
        rd = np.array([c[2] for c in classes], dtype=np.uint8)[kind]
        rf = (np.arange(R) % 2).astype(np.int32)  # not read
        part = np.array([c[3] for c in classes], dtype=np.int32)[kind]
    return kind, rv, rd, rf, part


def _profile_groups(ev, rv, p, ent_ptr):
    """Exchangeable entities of partition p share a (name, year-match) cell;
    everything outside the partition shares the last cell."""
    inside = (np.arange(len(ev)) >= ent_ptr[p]) & (np.arange(len(ev)) < ent_ptr[p + 1])
    g = ev[:, 1].astype(np.int64) * 2 + (ev[:, 0] == rv[0])
    ng = int(ev[:, 1].max()) * 2 + 2
    return np.where(inside, g, ng), ng + 1


def _class_exact(attrs, ev, ent_ptr, cls, collapsed):
    """Exact probability of each of the E entities for one class."""
    if collapsed:
        _, rv, f, p = cls
    else:
        _, rv, rd, p = cls
    e0, e1 = int(ent_ptr[p]), int(ent_ptr[p + 1])
    if collapsed:
        w = kr.dense_collapsed_weights(attrs, THETA, rv, f, ev[e0:e1])
    else:
        w = kr.dense_seq_weights(attrs, rv, rd, ev[e0:e1])
    assert w.sum() > 0  # the kernel has no empty-set tail
    exact = np.zeros(len(ev))
    exact[e0:e1] = w / w.sum()
    return exact


def _launch_dense(model, ev, ent_ptr, rv, rd, rf, part, collapsed, seed, gid0=5000):
    R = len(rv)
    out = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    C.link_update_dense(
        _dev(rv, torch.int32), _dev(rd, torch.uint8),
        _dev(np.arange(R) + gid0, torch.int64), _dev(part, torch.int32),
        _dev(rf, torch.int32), _dev(ev, torch.int32), _dev(ent_ptr, torch.int64),
        _dev(THETA, torch.float32), model.phi, model.norm_lin, *_model_tail(model),
        collapsed, seed, 6, out, _empty(torch.int64))
    return out


def _staging_engages(model, ent_ptr, rv, rd, p, collapsed):
    """The kernel's staging condition: (e1 - e0) * popcount(st_mask) >= 32."""
    const = model.attr_const.cpu().numpy()
    st = [a for a in range(2)
          if rv[a] >= 0 and not const[a] and (collapsed or rd[a])]
    return (int(ent_ptr[p + 1]) - int(ent_ptr[p])) * len(st) >= 32


@gpu
@pytest.mark.parametrize("collapsed", [1, 0])
def test_dense_link_distribution(collapsed, monkeypatch):
    """link_update_dense_kernel against the exact conditional of each class,
    and bitwise-equal with similarity staging off."""
    cache, model = make_model(DEV)
    attrs = cache.indexed_attributes
    classes = COLLAPSED_CLASSES if collapsed else SEQ_CLASSES
    ev = _dense_entities()
    kind, rv, rd, rf, part = _dense_records(classes, collapsed)
    assert len(rv) % 4 != 0

    staged = [_staging_engages(model, ENT_PTR, np.array(c[1]),
                               np.zeros(2) if collapsed else np.array(c[2]),
                               c[3], collapsed) for c in classes]
    assert any(staged) and not all(staged), staged

    monkeypatch.setenv("DBLINK_SIMH", "1")
    out = _launch_dense(model, ev, ENT_PTR, rv, rd, rf, part, collapsed, 2024)
    monkeypatch.setenv("DBLINK_SIMH", "0")  # re-read per launch
    out_global = _launch_dense(model, ev, ENT_PTR, rv, rd, rf, part, collapsed, 2024)
    assert torch.equal(out, out_global)

    sel = out.cpu().numpy()
    assert ((sel >= ENT_PTR[part]) & (sel < ENT_PTR[part + 1])).all()
    for k, cls in enumerate(classes):
        exact = _class_exact(attrs, ev, ENT_PTR, cls, collapsed)
        mine = sel[kind == k]
        n = len(mine)
        emp = np.bincount(mine, minlength=len(ev)) / n
        group, ng = _profile_groups(ev, cls[1], cls[3], ENT_PTR)
        exact_g = kr.group_probs(exact, group, ng)
        worst, bound = kr.calibrated_bound(exact_g, n, seed=100 + k)
        got = kr.tv(kr.group_probs(emp, group, ng), exact_g)
        print(f"dense collapsed={collapsed} class {k} ({cls[0]}): tv {got:.5f} "
              f"reference max {worst:.5f} bound {bound:.5f}")
        # calibrated bound = 1.5 x the largest TV among 200 multinomial samples
        # of this size from the exact probabilities. Reference maximum -> bound
        # for classes 0..3 (n = 30001 for class 0, 30000 for the others):
        #   collapsed=1: 0.00355 -> 0.00533, 0.00632 -> 0.00947,
        #                0.01303 -> 0.01955, 0.00201 -> 0.00302
        #   collapsed=0: 0.00014 -> 0.00021, 0.00967 -> 0.01450,
        #                0.00447 -> 0.00671, 0.00947 -> 0.01420
        # (a theta index transposed to [f, a] moves collapsed classes 1 and 2
        # by 0.033 and 0.087 in the same metric)
        assert got < bound, (cls[0], got, worst, bound)


@gpu
def test_dense_link_wide_vocabulary():
    """One PCG-II class over the 650-name mutation ball: 128 entities holding
    distinct names in a partition that starts at entity 7, a record whose name
    none of them holds (so the mass spreads over the similarity row; rows of
    262+ entries exceed the staging table and take the global lookup)."""
    cache, model = _mutation_ball_model()
    attrs = cache.indexed_attributes
    V = attrs[1].index.num_values
    rng = np.random.default_rng(23)
    ent_ptr = np.array([0, 7, 135], dtype=np.int64)
    names = rng.permutation(V)
    ev = np.stack([rng.integers(0, 10, 135), names[:135]], 1).astype(np.int32)
    x = int(names[200])
    assert x not in ev[7:, 1] and len(set(ev[7:, 1].tolist())) == 128
    cls = ("wide", [int(ev[20, 0]), x], 1, 1)
    N = N_LINK
    rv = np.tile(np.array([cls[1]], dtype=np.int32), (N, 1))
    out = _launch_dense(model, ev, ent_ptr, rv, np.zeros((N, 2), np.uint8),
                        np.ones(N, np.int32), np.ones(N, np.int32), 1, 777)
    sel = out.cpu().numpy()
    assert ((sel >= 7) & (sel < 135)).all()
    exact = _class_exact(attrs, ev, ent_ptr, cls, 1)
    group = kr.heaviest_plus_rest(exact, 20)
    exact_g = kr.group_probs(exact, group, 21)
    emp_g = kr.group_probs(np.bincount(sel, minlength=135) / N, group, 21)
    worst, bound = kr.calibrated_bound(exact_g, N, seed=110)
    got = kr.tv(emp_g, exact_g)
    print(f"dense wide: tv {got:.5f} reference max {worst:.5f} bound {bound:.5f}")
    # calibrated as above (21 cells, n = 30000): 0.01479 -> 0.02219
    assert got < bound, (got, worst, bound)


# ---- sequential value kernel -------------------------------------------------------

N_VAL = 20000


def _seq_value_state(x1, x2, n=N_VAL, with_extra=True):
    """Entities in blocks of n, one class per block (attribute 1 = name,
    attribute 0 = year, constant):
      0  two records, names x1 and x2 distorted; years 3 and 5 distorted
      1  the same plus a third record with the name missing
      2  name x1 distorted, then name x2 held; year 3 held, then 5 distorted
      3  no record
      4  one record, name missing, year 7 held
    Record rows are shuffled, so ent_rec_idx is not the identity; the order
    inside an entity is kept."""
    recs, owner = [], []

    def add(e, year, yd, name, nd):
        recs.append((year, name, yd, nd))
        owner.append(e)

    for i in range(n):
        add(i, 3, 1, x1, 1)
        add(i, 5, 1, x2, 1)
    if with_extra:
        for i in range(n, 2 * n):
            add(i, 3, 1, x1, 1)
            add(i, 5, 1, x2, 1)
            add(i, 6, 1, -1, 1)
        for i in range(2 * n, 3 * n):
            add(i, 3, 0, x1, 1)
            add(i, 5, 1, x2, 0)
        for i in range(4 * n, 5 * n):
            add(i, 7, 0, -1, 0)
    E = 5 * n if with_extra else n
    recs = np.array(recs, dtype=np.int64)
    owner = np.array(owner, dtype=np.int64)
    R = len(recs)
    rows = np.random.default_rng(3).permutation(R)   # record i lives in row rows[i]
    rv = np.empty((R, 2), dtype=np.int32)
    rd = np.empty((R, 2), dtype=np.uint8)
    rv[rows] = recs[:, :2]
    rd[rows] = recs[:, 2:]
    ent_rec_ptr = np.zeros(E + 1, dtype=np.int64)
    ent_rec_ptr[1:] = np.cumsum(np.bincount(owner, minlength=E))
    ent_rec_idx = rows.astype(np.int64)              # owner is already ascending
    return rv, rd, ent_rec_ptr, ent_rec_idx, E


def _launch_seq_value(model, rv, rd, ent_rec_ptr, ent_rec_idx, E, seed):
    ev = torch.full((E, 2), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    e64 = _empty(torch.int64)
    C.value_update(
        _dev(rv, torch.int32), _dev(rd, torch.uint8),
        torch.zeros(len(rv), dtype=torch.int32, device=DEV),
        _dev(ent_rec_ptr, torch.int64), _dev(ent_rec_idx, torch.int64), ev,
        model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        0, 1, seed, 4, 0, err, e64, e64, e64,
        model.csr_excl, model.csr_rawsum, model.z1, e64, _empty(torch.int32))
    assert int(err.cpu()) == 0
    return ev.cpu().numpy()


def _assert_value_class(label, got, exact, seed, group=None):
    n = len(got)
    emp = np.bincount(got, minlength=len(exact)) / n
    if group is not None:
        ng = int(group.max()) + 1
        emp, exact = kr.group_probs(emp, group, ng), kr.group_probs(exact, group, ng)
    worst, bound = kr.calibrated_bound(exact, n, seed=seed)
    tvd = kr.tv(emp, exact)
    print(f"seq value {label}: tv {tvd:.5f} reference max {worst:.5f} bound {bound:.5f}")
    assert tvd < bound, (label, tvd, worst, bound)


@gpu
def test_seq_value_distribution():
    """value_update_seq_kernel: five entity classes of 20000 replicas in one
    launch (the Philox element is per entity), both attributes."""
    cache, model = make_model(DEV)
    year, name = cache.indexed_attributes
    x1, x2 = 0, 2   # ANNA, ANNE
    n = N_VAL
    rv, rd, ptr, idx, E = _seq_value_state(x1, x2)
    assert not np.array_equal(idx, np.arange(len(idx)))
    ev = _launch_seq_value(model, rv, rd, ptr, idx, E, 31337)
    assert (ev >= 0).all()
    assert (ev[:, 0] < year.index.num_values).all()
    assert (ev[:, 1] < name.index.num_values).all()

    two = kr.seq_value_probs(name, [x1, x2])
    phi_name = kr.seq_value_probs(name, [])
    phi_year = kr.seq_value_probs(year, [3, 5])     # constant: phi whatever is linked
    assert kr.tv(two, phi_name) > 0.2               # the classes are distinguishable
    # calibrated bounds (kernel_refs.calibrated_bound, n = 20000), reference
    # maximum -> bound, in the order asserted: 0.01093 -> 0.01640,
    # 0.01252 -> 0.01878, 0.01465 -> 0.02197, 0.01520 -> 0.02280,
    # 0.01425 -> 0.02138, 0.01745 -> 0.02618
    _assert_value_class("two distorted", ev[:n, 1], two, 200)
    _assert_value_class("two distorted + missing", ev[n:2 * n, 1], two, 201)
    _assert_value_class("no record", ev[3 * n:4 * n, 1], phi_name, 202)
    _assert_value_class("missing only", ev[4 * n:, 1], phi_name, 203)
    _assert_value_class("constant, all distorted", ev[:n, 0], phi_year, 204)
    _assert_value_class("constant, no record", ev[3 * n:4 * n, 0], phi_year, 205)
    # a held value decides: the second record's name, the first record's year
    assert (ev[2 * n:3 * n, 1] == x2).all()
    assert (ev[2 * n:3 * n, 0] == 3).all()
    assert (ev[4 * n:, 0] == 7).all()


@gpu
def test_seq_value_wide_vocabulary():
    """The two-distorted-records class over the 650-name mutation ball: eleven
    lane strides over the domain, the last with 10 live lanes, then the
    cross-lane argmax."""
    cache, model = _mutation_ball_model()
    name = cache.indexed_attributes[1]
    V = name.index.num_values
    assert V > 64 and V % 64 != 0
    x1, x2 = 5, 300
    rv, rd, ptr, idx, E = _seq_value_state(x1, x2, with_extra=False)
    ev = _launch_seq_value(model, rv, rd, ptr, idx, E, 4711)
    exact = kr.seq_value_probs(name, [x1, x2])
    # calibrated (21 cells, n = 20000): 0.01521 -> 0.02282
    _assert_value_class("wide", ev[:, 1], exact, 210,
                        group=kr.heaviest_plus_rest(exact, 20))
    assert ev[:, 1].max() < V


# ---- fused log-likelihood ------------------------------------------------------------


@gpu
def test_distortion_update_fused_loglik():
    """E = 300, R = 1001, A = 2: 2602 items in 256-thread blocks, so block 2
    straddles the entity/record boundary at item 600 and the last block is
    partial. The 256-slot buffer must sum to the log-likelihood of the state
    the kernel wrote."""
    from dblink_amd.engine.cpu_engine import compute_summary
    from dblink_amd.engine.state import ChainState
    from dblink_amd.models.distortion import DistortionProbs

    cache, model = make_model(DEV)
    rng = np.random.default_rng(8)
    E, R, A = 300, 1001, 2
    Vs = [ia.index.num_values for ia in cache.indexed_attributes]
    ent_values = np.stack([rng.integers(0, Vs[a], E) for a in range(A)], 1).astype(np.int32)
    rec_ent = rng.integers(0, E, R).astype(np.int64)
    # half the observed values agree with the entity, a fifth are missing
    rec_values = ent_values[rec_ent].copy()
    other = np.stack([rng.integers(0, Vs[a], R) for a in range(A)], 1).astype(np.int32)
    flip = rng.random((R, A)) < 0.5
    rec_values[flip] = other[flip]
    rec_values[rng.random((R, A)) < 0.2] = -1
    assert (rec_values < 0).any()
    theta = torch.tensor([[0.3], [0.4]], dtype=torch.float32, device=DEV)

    def run(loglik):
        d = torch.full((R, A), 9, dtype=torch.uint8, device=DEV)
        C.distortion_update(
            _dev(rec_values, torch.int32), d, torch.zeros(R, dtype=torch.int32, device=DEV),
            _dev(np.arange(R) + 70, torch.int64), _dev(rec_ent, torch.int64),
            _dev(ent_values, torch.int32), theta, model.phi, model.norm_lin,
            model.self_expsim, model.voff, model.attr_const, 555, 12,
            _empty(torch.int64), model.log_phi, model.log_norm, model.csr_row_ptr,
            model.csr_col, model.csr_sim, loglik)
        return d

    fused = torch.zeros(256, dtype=torch.float64, device=DEV)
    dist = run(fused)
    assert torch.equal(run(_empty(torch.float64)), dist)
    rec_dist = dist.cpu().numpy()
    assert set(np.unique(rec_dist).tolist()) == {0, 1}
    # distorted and held values both occur on observed and on missing slots
    for miss in (True, False):
        assert len(set(rec_dist[(rec_values < 0) == miss].tolist())) == 2

    state = ChainState(
        iteration=0, ent_values=ent_values, ent_part=np.zeros(E, np.int32),
        rec_values=rec_values, rec_file=np.zeros(R, np.int32), rec_ent=rec_ent,
        rec_dist=rec_dist, rec_gid=np.arange(R, dtype=np.int64),
        dist_probs=DistortionProbs(np.full((A, 1), 0.05)), population_size=E,
        start_seed=0, current_seed=0)
    ref = compute_summary(state, cache, state.dist_probs)
    total = float(fused.sum().cpu())
    # the kernel's terms are f32 (as in test_summary_loglik_matches_cpu)
    assert total == pytest.approx(ref.log_likelihood, rel=1e-5)

    alone = torch.zeros(256, dtype=torch.float64, device=DEV)
    C.summary_loglik(
        _dev(ent_values, torch.int32), _dev(rec_values, torch.int32), dist,
        _dev(rec_ent, torch.int64), model.log_phi, model.log_norm, model.voff,
        model.csr_row_ptr, model.csr_col, model.csr_sim, model.attr_const, alone)
    # both add the same f32 terms in f64 and differ only in summation order:
    # 1e-9 of the sum of absolute terms, computed here in fp64
    attrs = cache.indexed_attributes
    abs_terms = sum(float(np.abs(attrs[a].index.log_probs[ent_values[:, a]]).sum())
                    for a in range(A))
    for r, a in zip(*np.nonzero((rec_dist == 1) & (rec_values >= 0))):
        ix, x = attrs[a].index, int(rec_values[r, a])
        term = np.log(ix.probability_of(x))
        if not attrs[a].is_constant:
            y = int(ent_values[rec_ent[r], a])
            term += np.log(ix.sim_norms[y] * ix.exp_sim_of(x, y))
        abs_terms += abs(term)
    assert abs(total - float(alone.sum().cpu())) <= 1e-9 * abs_terms


# ---- summary counts ------------------------------------------------------------------


@gpu
def test_summary_counts_every_slot():
    """A = 3, F = 2, E + R = 257 (one past a block), the entity/record
    boundary at item 100 inside block 0."""
    A, F, E, R = 3, 2, 100, 157
    rng = np.random.default_rng(12)
    rec_dist = (rng.random((R, A)) < 0.4).astype(np.uint8)
    rec_file = rng.integers(0, F, size=R).astype(np.int32)
    # a third of the entities without records
    owners = rng.permutation(E)[: E - E // 3]
    rec_ent = np.concatenate([owners, rng.choice(owners, R - len(owners))])
    cnt = np.bincount(rec_ent, minlength=E)
    ptr = np.zeros(E + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(cnt)
    assert (cnt == 0).sum() == E // 3

    n_counts = 1 + A * F + A + 1
    loglik = _dev(rng.normal(size=256), torch.float64)
    packed = torch.full((1 + n_counts + 1,), -7.0, dtype=torch.float64, device=DEV)
    C.summary_counts(_dev(rec_dist, torch.uint8), _dev(rec_file, torch.int32),
                     _dev(ptr, torch.int64), E,
                     torch.zeros(n_counts, dtype=torch.int64, device=DEV),
                     loglik, packed, _dev([0], torch.int32))
    host = packed.cpu().numpy()

    agg = np.zeros((A, F), dtype=np.int64)
    for a in range(A):
        agg[a] = np.bincount(rec_file[rec_dist[:, a] == 1], minlength=F)
    hist = np.bincount(rec_dist.sum(1), minlength=A + 1)
    assert len(set(agg.reshape(-1).tolist())) > 1 and (hist > 0).all()
    assert host[0] == pytest.approx(float(loglik.sum().cpu()), abs=1e-9)
    assert host[1] == E // 3
    np.testing.assert_array_equal(host[2:2 + A * F], agg.reshape(-1))
    np.testing.assert_array_equal(host[2 + A * F:2 + A * F + A + 1], hist)
    assert host[-1] == 0
