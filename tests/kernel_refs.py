"""Plain numpy / fp64 references shared by ``test_gpu_link_index``,
``test_gpu_dense_seq``, ``test_gpu_value_dist``, ``test_gpu_distortion`` and
``test_kernel_refs`` (which holds them to the per-record oracle of
``cpu_engine`` and to known-answer vectors without a GPU).

Nothing here touches a device or the native extension: the formulas are
written from the update rules (GibbsUpdates.scala line references at each
function), over ``cache.indexed_attributes[a].index`` in fp64.
"""

import numpy as np

# ---- inverted index --------------------------------------------------------------

PB_THREADS = 1024  # items per block of the two counting passes
PB_TBL = 2048      # slots of their per-block open-addressing table


def pb_hash(key):
    """numpy copy of ``pb_hash`` (kernels.hip): Knuth multiplicative hash of
    the int32 key, bits 16..26."""
    k = np.asarray(key, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    h = (k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    return ((h >> np.uint64(16)) & np.uint64(PB_TBL - 1)).astype(np.int64)


def probe_table(keys):
    """Linear-probing insert of the DISTINCT keys of one block into a
    PB_TBL-slot table. Returns (home, final) slot per distinct key. Which key
    ends where depends on insertion order, but the occupied slots and the
    number of probes crossing each slot boundary do not, so 'some key wrapped
    past slot 2047' is a property of the key set."""
    keys = np.unique(np.asarray(keys, dtype=np.int64))
    home = pb_hash(keys)
    table = np.full(PB_TBL, -1, dtype=np.int64)
    final = np.empty_like(home)
    for i, (k, h) in enumerate(zip(keys.tolist(), home.tolist())):
        s = h
        while table[s] != -1:
            s = (s + 1) & (PB_TBL - 1)
        table[s] = k
        final[i] = s
    return keys, home, final


def slot_values(values, pairs, missing_to=None):
    """[N, A] value ids -> [N, T] slot values, T = A + len(pairs): the A
    single attributes, then one composite ``v1 * V2 + v2`` per pair
    ``(a1, a2, V2)``. A negative (missing) constituent makes the slot
    ``missing_to`` (records; entities never hold missing values)."""
    values = np.asarray(values, dtype=np.int64)
    cols = [values[:, a] for a in range(values.shape[1])]
    for a1, a2, v2 in pairs:
        comp = values[:, a1] * v2 + values[:, a2]
        if missing_to is not None:
            comp = np.where((values[:, a1] < 0) | (values[:, a2] < 0), -1, comp)
        cols.append(comp)
    out = np.stack(cols, 1)
    if missing_to is not None:
        out = np.where(out < 0, missing_to, out)
    return out


def index_reference(ent_part, ent_values, pairs, vmax, num_parts):
    """The inverted index by definition. key = (part * T + t) * Vmax + v.

    Returns ``keys`` [T * E] in the kernels' slot-major item order
    (item = t * E + e), ``counts`` [nk], ``ptr`` [nk + 1] and ``postings``
    [T * E] with entities ascending inside each key."""
    ent_part = np.asarray(ent_part, dtype=np.int64)
    sv = slot_values(ent_values, pairs)            # [E, T]
    E, T = sv.shape
    nk = num_parts * T * vmax
    keys = ((ent_part[None, :] * T + np.arange(T)[:, None]) * vmax + sv.T).reshape(-1)
    counts = np.bincount(keys, minlength=nk)
    ptr = np.zeros(nk + 1, dtype=np.int64)
    ptr[1:] = np.cumsum(counts)
    order = np.argsort(keys, kind="stable")
    postings = (order % E).astype(np.int32)
    return keys, counts, ptr, postings


def query_keys(rec_part, rec_values, pairs, vmax):
    """Per (record, slot): key, with -1 where the slot is missing."""
    rec_part = np.asarray(rec_part, dtype=np.int64)
    sv = slot_values(rec_values, pairs, missing_to=-1)   # [R, T]
    T = sv.shape[1]
    keys = (rec_part[:, None] * T + np.arange(T)[None, :]) * vmax + sv
    return np.where(sv < 0, -1, keys)


def sort_within_segments(postings, ptr):
    """postings with each [ptr[k], ptr[k+1]) segment sorted ascending."""
    postings = np.asarray(postings, dtype=np.int64)
    seg = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return postings[np.lexsort((postings, seg))]


def classify_modes_reference(rec_values, rec_dist, rec_part, ent_ptr, cand_lo,
                             cand_hi, small_threshold, heavy_threshold):
    """Routing rule of the indexed link phase, record by record: 2 = the
    hierarchical sampler (no non-distorted attribute and a partition above the
    threshold, or exactly one with a posting range above it; only with a
    positive threshold), else 1 = thread scan when the smallest non-distorted
    single-attribute range is at most ``small_threshold``, else 0. cand_* are
    [R, T]; only the A single-attribute columns count."""
    R, A = rec_values.shape
    mode = np.zeros(R, dtype=np.uint8)
    for r in range(R):
        sizes = [int(cand_hi[r, a] - cand_lo[r, a]) for a in range(A)
                 if rec_values[r, a] >= 0 and not rec_dist[r, a]]
        m = 0
        if heavy_threshold > 0:
            pool = int(ent_ptr[rec_part[r] + 1] - ent_ptr[rec_part[r]])
            if not sizes and pool > heavy_threshold:
                m = 2
            elif len(sizes) == 1 and sizes[0] > heavy_threshold:
                m = 2
        if m == 0 and sizes and min(sizes) <= small_threshold:
            m = 1
        mode[r] = m
    return mode


# ---- exact conditionals ------------------------------------------------------------


def _expsim_row(index, x, ys):
    """expsim(x, y) for an array of y, by scalar lookups (1 off the index)."""
    return np.array([index.exp_sim_of(int(x), int(y)) for y in ys], dtype=np.float64)


def dense_collapsed_weights(attrs, theta, rv, f, ent_values):
    """PCG-II link weights with distortions integrated out
    (GibbsUpdates.scala:363-395): over observed attributes the product of
    (x == y)(1 - theta[a, f]) + theta[a, f] phi(x) [norm(y) expsim(x, y)];
    the bracket only for a non-constant attribute."""
    w = np.ones(ent_values.shape[0], dtype=np.float64)
    for a, ia in enumerate(attrs):
        x = int(rv[a])
        if x < 0:
            continue
        th = float(theta[a][f])
        ys = ent_values[:, a]
        like = np.full(len(ys), ia.index.probability_of(x), dtype=np.float64)
        if not ia.is_constant:
            like = like * ia.index.sim_norms[ys] * _expsim_row(ia.index, x, ys)
        w *= (ys == x) * (1.0 - th) + th * like
    return w


def dense_seq_weights(attrs, rv, rd, ent_values):
    """Gibbs-Sequential link weights (GibbsUpdates.scala:434-466): zero unless
    the entity equals the record on every observed non-distorted attribute,
    else the product over observed distorted non-constant attributes of
    norm(y) expsim(x, y) (phi(x) and constant attributes cancel)."""
    w = np.ones(ent_values.shape[0], dtype=np.float64)
    for a, ia in enumerate(attrs):
        x = int(rv[a])
        if x < 0:
            continue
        ys = ent_values[:, a]
        if not rd[a]:
            w *= ys == x
        elif not ia.is_constant:
            w *= ia.index.sim_norms[ys] * _expsim_row(ia.index, x, ys)
    return w


def seq_value_probs(ia, xs_dist):
    """Gibbs-Sequential value conditional over the whole domain when every
    observed linked record is distorted (GibbsUpdates.scala:652-698):
    w(v) = phi(v) prod_r norm(v) expsim(x_r, v); phi alone for a constant
    attribute or without observed records."""
    index = ia.index
    w = index.probs.astype(np.float64).copy()
    if not ia.is_constant:
        vs = np.arange(index.num_values)
        for x in xs_dist:
            w *= index.sim_norms * _expsim_row(index, x, vs)
    return w / w.sum()


def value_probs(ia, theta_a, recs, collapsed):
    """The value conditional over the whole domain, in PRODUCT form
    (GibbsUpdates.scala:576-646): P(v) ~ b(v) prod_i F_i(v). The kernels and
    the CPU oracle draw from the equivalent mixture of the base distribution
    and a perturbation on the union of the similarity rows; nothing of that
    (no Z_k, no ``- 1``, no support set) appears here.

    ``recs`` lists ``(x, file)`` of the observed linked records (k of them),
    ``theta_a`` is theta[a, :]. b(v) = phi(v) norm(v)^k for a non-constant
    attribute with k > 0, else phi(v). F_i(v) = expsim(x_i, v) (1 off the
    truncated index, 1 everywhere for a constant attribute); collapsed adds
    [v == x_i] (1 / theta[f_i] - 1) / (phi(x_i) norm(x_i)) to it, without the
    norm for a constant attribute. Non-collapsed takes every record as
    distorted and ignores theta, which leaves phi for a constant attribute."""
    index = ia.index
    phi = index.probs.astype(np.float64)
    k = len(recs)
    w = phi.copy()
    if not ia.is_constant and k > 0:
        w *= index.sim_norms.astype(np.float64) ** k
    vs = np.arange(index.num_values)
    for x, f in recs:
        x = int(x)
        fac = np.ones(len(vs)) if ia.is_constant else _expsim_row(index, x, vs)
        if collapsed:
            mass = phi[x] if ia.is_constant else phi[x] * float(index.sim_norms[x])
            fac[x] += (1.0 / float(theta_a[f]) - 1.0) / mass
        w *= fac
    return w / w.sum()


# ---- Philox with the GPU keying -----------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def philox4x32(seed, c0, c1, c2, c3):
    """Philox4x32-10 (Salmon et al. 2011) as ``common.h`` keys it: key = low
    and high word of ``seed``, counter = the four words, nothing else folded
    into the key. Counter words broadcast; returns the four output words as
    uint32 arrays."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0 = np.uint64(seed & 0xFFFFFFFF)
    k1 = np.uint64(seed >> 32)
    x = [np.asarray(c, dtype=np.uint64) & _M32 for c in np.broadcast_arrays(c0, c1, c2, c3)]
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = x[0] * m0            # 32 x 32 bits: fits uint64
        p1 = x[2] * m1
        x = [(p1 >> s32) ^ x[1] ^ k0, p1 & _M32, (p0 >> s32) ^ x[3] ^ k1, p0 & _M32]
        k0 = (k0 + w0) & _M32
        k1 = (k1 + w1) & _M32
    return tuple(c.astype(np.uint32) for c in x)


def gpu_uniform(seed, iteration, phase, elem, draw, word=0):
    """fp64 value (x + 0.5) 2^-32 of output word ``word`` of the Philox call
    behind ``philox_uniform`` / ``philox_uniform2`` / ``value_uniforms``:
    counter = (elem low, elem high, iteration ^ (phase << 24), draw). The
    kernels round the same word to f32 where they hold it as a float."""
    elem = np.asarray(elem, dtype=np.uint64)
    c2 = (int(iteration) ^ (int(phase) << 24)) & 0xFFFFFFFF
    out = philox4x32(seed, elem & _M32, elem >> np.uint64(32), c2, int(draw) & 0xFFFFFFFF)
    return (out[word].astype(np.float64) + 0.5) * 2.0 ** -32


# ---- comparison ---------------------------------------------------------------------


def tv(emp, exact):
    return 0.5 * float(np.abs(np.asarray(emp) - np.asarray(exact)).sum())


def group_probs(p, group, ngroups=None):
    """Sum cell probabilities onto groups of exchangeable cells."""
    ng = int(np.max(group)) + 1 if ngroups is None else ngroups
    return np.bincount(group, weights=p, minlength=ng)


def heaviest_plus_rest(exact, k=20):
    """Group map: the k heaviest cells keep a cell each, the others share one."""
    exact = np.asarray(exact)
    group = np.full(len(exact), k, dtype=np.int64)
    top = np.argsort(-exact, kind="stable")[:k]
    group[top] = np.arange(len(top))
    return group


def calibrated_bound(exact_g, n, seed, draws=200, margin=1.5):
    """Total-variation bound for ``n`` draws from ``exact_g``: the largest TV
    among ``draws`` multinomial samples of that size, times ``margin`` (which
    covers the gap between ``draws`` and infinitely many). Returns
    (reference maximum, bound)."""
    exact_g = np.asarray(exact_g, dtype=np.float64)
    exact_g = exact_g / exact_g.sum()
    rng = np.random.default_rng(seed)
    samples = rng.multinomial(n, exact_g, size=draws) / float(n)
    worst = float((0.5 * np.abs(samples - exact_g[None, :]).sum(1)).max())
    return worst, margin * worst
