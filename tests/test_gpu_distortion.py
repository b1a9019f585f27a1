"""``distortion_update_kernel`` and the k = 0 base draw, elementwise-exact.

Both are deterministic functions of one Philox call per (record, attribute)
or (entity, attribute), so they are compared entry by entry with numpy: the
uniform from ``kernel_refs.gpu_uniform`` (the Philox transcription held to the
known-answer vectors in ``test_kernel_refs``), the probability in fp64.

The kernels hold the uniform and the probability in f32, so an entry whose
uniform lies within 1e-6 of its threshold could legitimately fall either way.
No entry is excluded for that: the seeds below are chosen so that no such
entry exists, and ``test_references_have_no_borderline_entry`` (no GPU)
asserts it.
"""

import numpy as np
import pytest

import kernel_refs as kr
from test_gpu import _dev, make_model

torch = pytest.importorskip("torch")

gpu = pytest.mark.gpu

if torch.cuda.is_available():
    from dblink_amd import ops

    C = ops.native()
    DEV = torch.device("cuda", 0)

PH_DIST, PH_VALM = 2, 4     # phase tags of kernels.hip
EDGE = 1e-6                 # f32 rounding of a uniform in (0, 1) is below 6e-8

# ---- distortion --------------------------------------------------------------------

R_DIST, E_DIST = 6001, 500  # 12002 items: the last 256-thread block is partial
# theta[a, f]; file 2 holds the two degenerate values
THETA = np.array([[0.05, 0.3, 0.0], [0.12, 0.45, 1.0]])
DIST_SEED, DIST_ITER = 20240611, 13


def distortion_state(attrs):
    """6001 records over 500 entities and 3 files. Per (record, attribute):
    missing (20 %), equal to the entity's value (50 %) or different (30 %);
    entity values are uniform over the domain, so 'equal' happens on every
    value of both attributes."""
    rng = np.random.default_rng(21)
    R, E, A = R_DIST, E_DIST, len(attrs)
    Vs = [ia.index.num_values for ia in attrs]
    ent_values = np.stack([rng.integers(0, Vs[a], E) for a in range(A)], 1).astype(np.int32)
    rec_ent = rng.integers(0, E, R).astype(np.int64)
    rec_file = rng.integers(0, 3, R).astype(np.int32)
    rec_gid = rng.integers(0, 1 << 40, R).astype(np.int64)
    # gid * 32 + a crosses 32 bits from gid = 2^27 on
    rec_gid[:4] = [(1 << 27) - 1, 1 << 27, (1 << 40) - 1, 3]
    kind = rng.choice(3, size=(R, A), p=[0.2, 0.5, 0.3])
    y = ent_values[rec_ent]
    shift = np.stack([rng.integers(1, Vs[a], R) for a in range(A)], 1)
    other = (y + shift) % np.array(Vs)[None, :]
    rec_values = np.where(kind == 0, -1, np.where(kind == 1, y, other)).astype(np.int32)
    return dict(ent_values=ent_values, rec_ent=rec_ent, rec_file=rec_file,
                rec_gid=rec_gid, rec_values=rec_values, kind=kind)


def distortion_reference(attrs, st, seed, iteration):
    """(u, p, z) per (record, attribute) (GibbsUpdates.scala:324-359): p is
    theta for a missing value, pr1 / (pr0 + pr1) with pr1 = theta self_mass[x]
    and pr0 = 1 - theta where record and entity agree, 1 where they differ.
    theta is the f32 value the kernel reads."""
    A = len(attrs)
    theta = THETA.astype(np.float32).astype(np.float64)
    elem = st["rec_gid"].astype(np.uint64)[:, None] * np.uint64(32) \
        + np.arange(A, dtype=np.uint64)[None, :]
    u = kr.gpu_uniform(seed, iteration, PH_DIST, elem, 0)
    th = np.stack([theta[a][st["rec_file"]] for a in range(A)], 1)
    x = st["rec_values"]
    mass = np.stack([attrs[a].index.self_mass[np.maximum(x[:, a], 0)] for a in range(A)], 1)
    pr1, pr0 = th * mass, 1.0 - th
    agree = pr1 / (pr0 + pr1)
    p = np.where(st["kind"] == 0, th, np.where(st["kind"] == 1, agree, 1.0))
    return u, p, (u < p).astype(np.uint8)


def borderline(u, p):
    """Entries that f32 arithmetic could decide either way. A probability of
    exactly 0 cannot (u > 0 in any precision); a probability of exactly 1 is
    kept in: a uniform that close to 1 rounds to 1.0f."""
    return (np.abs(u - p) <= EDGE) & (p != 0.0)


# ---- k = 0 base draw ---------------------------------------------------------------

E_BASE = 3001
ENT_ID_BASE = 2 ** 31 + 5   # (base + e) * 32 + a needs 37 bits
BASE_SEED, BASE_ITER = 77001, 3


def base_draw_reference(attrs, seed, iteration):
    """The alias draw of value_base_draw_pair: slot i = floor(u1 V), kept when
    u2 < prob[i] (the f32 table entry), else alias[i]; u1, u2 are words 0 and
    1 of the Philox call tagged 0xFFFF0000. Returns (draw [E, A], borderline)."""
    e = np.arange(E_BASE, dtype=np.uint64) + np.uint64(ENT_ID_BASE)
    out = np.empty((E_BASE, len(attrs)), dtype=np.int32)
    edge = np.zeros((E_BASE, len(attrs)), dtype=bool)
    for a, ia in enumerate(attrs):
        table = ia.index.distribution
        prob = table.prob.astype(np.float32).astype(np.float64)
        n = len(prob)
        elem = e * np.uint64(32) + np.uint64(a)
        u1 = kr.gpu_uniform(seed, iteration, PH_VALM, elem, 0xFFFF0000, 0)
        u2 = kr.gpu_uniform(seed, iteration, PH_VALM, elem, 0xFFFF0000, 1)
        i = np.minimum(np.floor(u1 * n).astype(np.int64), n - 1)
        out[:, a] = np.where(u2 < prob[i], i, table.alias[i])
        frac = u1 * n - np.floor(u1 * n)
        edge[:, a] = (np.minimum(frac, 1.0 - frac) / n <= EDGE) | (np.abs(u2 - prob[i]) <= EDGE)
    return out, edge


def test_references_have_no_borderline_entry():
    """On the references alone (no GPU): with the seeds above no uniform lies
    within 1e-6 of its threshold, so the exact comparisons exclude nothing."""
    cache, _ = make_model(torch.device("cpu"))
    attrs = cache.indexed_attributes
    st = distortion_state(attrs)
    u, p, z = distortion_reference(attrs, st, DIST_SEED, DIST_ITER)
    assert not borderline(u, p).any()
    assert len(np.unique(st["rec_gid"])) == R_DIST
    assert (st["rec_gid"] >= 1 << 27).sum() > 1000 and (st["rec_gid"] < 1 << 27).any()
    assert not np.array_equal(st["rec_ent"], np.arange(R_DIST) % E_DIST)
    for a in range(2):
        for kind in range(3):
            assert (st["kind"][:, a] == kind).sum() > 1000
        agree_on = np.unique(st["rec_values"][st["kind"][:, a] == 1, a])
        assert len(agree_on) == attrs[a].index.num_values   # every value
        # both outcomes occur on missing and on agreeing values of files 0, 1
        live = st["rec_file"] < 2
        for kind in (0, 1):
            assert set(z[live & (st["kind"][:, a] == kind), a].tolist()) == {0, 1}
    _, edge = base_draw_reference(attrs, BASE_SEED, BASE_ITER)
    assert not edge.any()


def _run_distortion(model, st, seed, iteration, ctrl=None):
    R = R_DIST
    d = torch.full((R, 2), 9, dtype=torch.uint8, device=DEV)
    C.distortion_update(
        _dev(st["rec_values"], torch.int32), d, _dev(st["rec_file"], torch.int32),
        _dev(st["rec_gid"], torch.int64), _dev(st["rec_ent"], torch.int64),
        _dev(st["ent_values"], torch.int32), _dev(THETA, torch.float32), model.phi,
        model.norm_lin, model.self_expsim, model.voff, model.attr_const, seed, iteration,
        torch.empty(0, dtype=torch.int64, device=DEV) if ctrl is None else ctrl,
        model.log_phi, model.log_norm, model.csr_row_ptr, model.csr_col, model.csr_sim,
        torch.empty(0, dtype=torch.float64, device=DEV))
    return d


@gpu
def test_distortion_kernel_exact():
    """rec_dist equals the numpy reference on all 12002 entries: F = 3, the
    constant-attribute agree branch, rec_file, the rec_ent indirection and gid
    keying past 32 bits all enter the expected bit."""
    cache, model = make_model(DEV)
    attrs = cache.indexed_attributes
    st = distortion_state(attrs)
    u, p, want = distortion_reference(attrs, st, DIST_SEED, DIST_ITER)
    assert not borderline(u, p).any()      # nothing is excluded below

    got_t = _run_distortion(model, st, DIST_SEED, DIST_ITER)
    got = got_t.cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (len(wrong), wrong[:5], got[got != want][:5])

    # theta = 0 (year, file 2): never distorted unless the values differ;
    # theta = 1 (name, file 2): always distorted
    f2 = st["rec_file"] == 2
    zero = f2 & (st["kind"][:, 0] != 2)
    assert zero.sum() > 1000 and (got[zero, 0] == 0).all()
    assert (got[f2 & (st["kind"][:, 0] == 2), 0] == 1).all()
    assert f2.sum() > 1500 and (got[f2, 1] == 1).all()

    # seed and iteration from a device ctrl tensor override the scalars
    ctrl = _dev(np.array([DIST_SEED, DIST_ITER]), torch.int64)
    by_ctrl = _run_distortion(model, st, DIST_SEED + 1, DIST_ITER + 5, ctrl)
    assert torch.equal(by_ctrl, got_t)
    # and the scalars matter without it
    assert not torch.equal(_run_distortion(model, st, DIST_SEED + 1, DIST_ITER + 5), got_t)


@gpu
def test_base_draw_exact():
    """value_update in kobs mode with kobs = 0 everywhere: every pair is a
    phi alias draw keyed by (ent_id_base + e) * 32 + a, here past 32 bits."""
    cache, model = make_model(DEV)
    attrs = cache.indexed_attributes
    want, edge = base_draw_reference(attrs, BASE_SEED, BASE_ITER)
    assert not edge.any()                  # nothing is excluded below
    for a, ia in enumerate(attrs):         # the table the kernel reads
        v0 = int(model.voff[a])
        np.testing.assert_array_equal(
            model.phi_prob[v0:v0 + ia.index.num_values].cpu().numpy(),
            ia.index.distribution.prob.astype(np.float32))

    E = E_BASE
    ev = torch.full((E, 2), -7, dtype=torch.int32, device=DEV)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    e64 = torch.empty(0, dtype=torch.int64, device=DEV)
    C.value_update(
        torch.full((1, 2), -1, dtype=torch.int32, device=DEV),   # one unlinked record
        torch.zeros((1, 2), dtype=torch.uint8, device=DEV),
        torch.zeros(1, dtype=torch.int32, device=DEV),
        torch.zeros(E + 1, dtype=torch.int64, device=DEV),
        torch.zeros(1, dtype=torch.int64, device=DEV), ev,
        model.theta, model.phi, model.log_phi, model.norm_lin, model.log_norm,
        model.voff, model.csr_row_ptr, model.csr_col, model.csr_sim,
        model.phi_prob, model.phi_alias, model.pow_prob, model.pow_alias,
        model.pow_off, model.log_pow_total, model.attr_const, model.Kc,
        1, 0, BASE_SEED, BASE_ITER, ENT_ID_BASE, err, e64, e64, e64,
        model.csr_excl, model.csr_rawsum, model.z1, e64,
        torch.zeros(E * 2, dtype=torch.int32, device=DEV))
    assert int(err.cpu()) == 0
    got = ev.cpu().numpy()
    wrong = np.argwhere(got != want)
    assert len(wrong) == 0, (len(wrong), wrong[:5])
    for a, ia in enumerate(attrs):         # not a constant column by accident
        assert len(np.unique(got[:, a])) == ia.index.num_values
