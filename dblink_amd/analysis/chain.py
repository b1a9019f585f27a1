"""Posterior linkage-chain queries (parity: ``LinkageChain.scala:27-212``).

Host-side numpy/pyarrow implementations — these run once per project over the
saved chain, not per iteration, so they are not performance-critical.
"""

from __future__ import annotations

import os
from collections import Counter, defaultdict

import numpy as np

from ..engine.writers import read_linkage_chain


def _iter_clusters(table):
    """Yield (iteration, partitionId, clusters) from a linkage-chain table."""
    iters = table["iteration"].to_pylist()
    pids = table["partitionId"].to_pylist()
    structs = table["linkageStructure"].to_pylist()
    yield from zip(iters, pids, structs)


def most_probable_clusters(table):
    """{record_id -> (cluster frozenset, frequency)} (LinkageChain.scala:52-64)."""
    iterations = set(table["iteration"].to_pylist())
    num_samples = len(iterations)
    freq = Counter()
    for _, _, clusters in _iter_clusters(table):
        for cluster in clusters:
            if cluster:
                freq[frozenset(cluster)] += 1
    best = {}
    for cluster, count in freq.items():
        f = count / num_samples
        for rid in cluster:
            cur = best.get(rid)
            if cur is None or f > cur[1]:
                best[rid] = (cluster, f)
    return best


def shared_most_probable_clusters(table):
    """Steorts et al. sMPC point estimate -> list of clusters (sets of record
    ids) (LinkageChain.scala:75-109)."""
    mpc = most_probable_clusters(table)
    agg = defaultdict(set)
    for rid, (cluster, _) in mpc.items():
        agg[cluster].add(rid)
    return [set(v) for v in agg.values()]


def partition_sizes(table):
    """{iteration -> {pid -> number of clusters}} (LinkageChain.scala:118-128)."""
    out = defaultdict(dict)
    for it, pid, clusters in _iter_clusters(table):
        out[it][pid] = len(clusters)
    return dict(out)


def cluster_size_distribution(table):
    """{iteration -> {size -> count}} (LinkageChain.scala:137-154)."""
    out = defaultdict(Counter)
    for it, _, clusters in _iter_clusters(table):
        for cluster in clusters:
            out[it][len(cluster)] += 1
    return {it: dict(c) for it, c in out.items()}


def save_cluster_size_distribution(dist, output_path):
    """CSV: header `iteration,0..maxSize` (LinkageChain.scala:162-185)."""
    path = os.path.join(output_path, "cluster-size-distribution.csv")
    max_size = max((max(c) for c in dist.values() if c), default=0)
    with open(path, "w", encoding="utf-8") as f:
        f.write("iteration," + ",".join(str(k) for k in range(max_size + 1)) + "\n")
        for it in sorted(dist):
            row = [str(dist[it].get(k, 0)) for k in range(max_size + 1)]
            f.write(f"{it}," + ",".join(row) + "\n")
    return path


def save_partition_sizes(sizes, output_path):
    """CSV: header `iteration,<pid...>` (LinkageChain.scala:193-211)."""
    path = os.path.join(output_path, "partition-sizes.csv")
    pids = sorted({p for m in sizes.values() for p in m})
    with open(path, "w", encoding="utf-8") as f:
        f.write("iteration," + ",".join(str(p) for p in pids) + "\n")
        for it in sorted(sizes):
            f.write(f"{it}," + ",".join(str(sizes[it].get(p, 0)) for p in pids) + "\n")
    return path


def save_clusters_csv(clusters, path):
    """One cluster per line, comma-separated record ids (analysis/package.scala:99-108)."""
    with open(path, "w", encoding="utf-8") as f:
        for cluster in clusters:
            f.write(", ".join(sorted(cluster)) + "\n")
    return path


def read_clusters_csv(path):
    out = []
    with open(path, "r", encoding="utf-8") as f:
        for line in f:
            line = line.strip()
            if line:
                out.append({x.strip() for x in line.split(",")})
    return out


def load_chain(output_path, lower_iteration_cutoff=0):
    d = os.path.join(output_path, "linkage-chain.parquet")
    if not os.path.isdir(d):
        return None
    table = read_linkage_chain(output_path, lower_iteration_cutoff)
    if table is None or table.num_rows == 0:
        return None
    return table


def _flatten_chain(table):
    """Flatten the nested linkage column -> (record_ids, cluster_gidx,
    iteration_per_cluster, cluster_sizes). cluster_gidx is a dense global
    cluster-instance index across all rows."""
    import pyarrow as pa

    col = table["linkageStructure"].combine_chunks()
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    iters = np.asarray(table["iteration"].to_numpy())
    # outer level: clusters per (iteration, pid) row
    outer = col
    outer_offsets = np.asarray(outer.offsets)
    clusters = outer.flatten()  # list<string> per cluster
    inner_offsets = np.asarray(clusters.offsets)
    record_ids = clusters.flatten().to_numpy(zero_copy_only=False)
    n_clusters = len(clusters)
    cluster_sizes = np.diff(inner_offsets)
    # iteration of each cluster: repeat row iteration by clusters-per-row
    clusters_per_row = np.diff(outer_offsets)
    iter_per_cluster = np.repeat(iters, clusters_per_row)
    cluster_gidx = np.repeat(np.arange(n_clusters, dtype=np.int64), cluster_sizes)
    return record_ids, cluster_gidx, iter_per_cluster, cluster_sizes, inner_offsets


# widest (code | count | index) packing that fits a signed int64 composite
# sort key; beyond it _mpc_core falls back to a 3-key lexsort
_PACK_BITS = 62


def _native_mpc():
    """The OpenMP MPC helpers, or None (numpy fallback). Their integer
    arithmetic is bitwise-identical to the numpy expressions they stand
    in for (DBLINK_NATIVE_MPC=0 forces the numpy path)."""
    import os

    if os.environ.get("DBLINK_NATIVE_MPC", "1") == "0":
        return None
    try:
        from .. import ops

        if ops.have_native() and hasattr(ops.native(), "mpc_cluster_keys"):
            return ops.native()
    except Exception:
        pass
    return None


def _mpc_keys_numpy(codes, off64, cluster_sizes):
    """Order-independent cluster content keys: two splitmix-derived per-code
    hashes summed per cluster mod 2^64 (zero-prefixed cumsum + segment
    diff), combined with the cluster size. mpc_cluster_keys computes the
    exact same integers natively."""

    def mix(x):  # splitmix64 finalizer
        x = (x + np.uint64(0x9E3779B97F4A7C15))
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
        return x

    h1 = mix(codes)
    # second independent sum: a nonlinear remix of h1 (h1 is already
    # well-mixed, so one multiply round suffices for pair independence)
    h2 = (h1 ^ (h1 >> np.uint64(29))) * np.uint64(0xD6E8FEB86659FD93)
    h2 ^= h2 >> np.uint64(32)
    n_flat = len(h1)
    cc1 = np.empty(n_flat + 1, dtype=np.uint64)
    cc1[0] = np.uint64(0)
    np.cumsum(h1, out=cc1[1:])
    cc2 = np.empty(n_flat + 1, dtype=np.uint64)
    cc2[0] = np.uint64(0)
    np.cumsum(h2, out=cc2[1:])
    s1 = cc1[off64[1:]] - cc1[off64[:-1]]
    s2 = cc2[off64[1:]] - cc2[off64[:-1]]
    return (s1 ^ (s2 * np.uint64(0x9E3779B97F4A7C15))) + cluster_sizes.astype(
        np.uint64)


def _mpc_core(table):
    """Vectorized MPC internals over large chains: clusters are identified
    by an order-independent composite hash of their member record ids (two
    independent 64-bit mixes of the records' dictionary codes + size —
    collisions are negligible). All grouping runs on integer codes with
    contiguous-segment reductions (clusters are contiguous in the flattened
    layout), so no per-entry string hashing or string groupbys. Returns
    (best_codes, best_keys, best_freq, first_idx, inner_offsets, codes_i,
    uniq_rids, kcode)."""
    import pandas as pd
    import pyarrow as pa

    # flatten in Arrow and dictionary-encode the member ids natively: no
    # 50M-element python-object string arrays, no string factorize
    col = table["linkageStructure"].combine_chunks()
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    clusters = col.flatten()
    inner_offsets = np.asarray(clusters.offsets)
    cluster_sizes = np.diff(inner_offsets)
    members = clusters.flatten()
    if isinstance(members, pa.ChunkedArray):
        members = members.combine_chunks()
    enc = members.dictionary_encode()
    codes_i = np.asarray(enc.indices)
    uniq_rids = np.asarray(enc.dictionary.to_numpy(zero_copy_only=False))
    num_samples = len(np.unique(np.asarray(table["iteration"].to_numpy())))
    codes = codes_i.astype(np.uint64)
    off64 = inner_offsets.astype(np.int64)
    nat = _native_mpc()
    if nat is not None:
        import torch

        c32 = np.ascontiguousarray(codes_i, dtype=np.int32)
        if not c32.flags.writeable:  # arrow buffers are read-only
            c32 = c32.copy()
        codes32 = torch.from_numpy(c32)
        off_t = torch.from_numpy(np.ascontiguousarray(off64))
        key = nat.mpc_cluster_keys(codes32, off_t).numpy().view(np.uint64)
    else:
        with np.errstate(over="ignore"):
            key = _mpc_keys_numpy(codes, off64, cluster_sizes)
    # frequency of each distinct cluster content
    kcode, _ = pd.factorize(key)
    kcounts = np.bincount(kcode)
    freq_per_cluster = kcounts[kcode] / num_samples
    # one representative cluster instance per distinct key: first occurrence
    if nat is not None:
        first_idx = nat.first_occurrence(
            __import__("torch").from_numpy(
                np.ascontiguousarray(kcode, dtype=np.int64)),
            int(len(kcounts))).numpy()
    else:
        # reversed fancy assignment leaves the FIRST occurrence (no sort)
        first_idx = np.zeros(len(kcounts), dtype=np.int64)
        first_idx[kcode[::-1]] = np.arange(len(kcode) - 1, -1, -1,
                                           dtype=np.int64)
    # per record-code: best (max count, first entry on ties) cluster entry
    # via ONE composite int64 sort: code | count | inverted entry index
    n_ent = len(codes)
    idx_bits = max(1, int(n_ent - 1).bit_length())
    cnt_bits = max(1, int(num_samples).bit_length())
    code_bits = max(1, int(len(uniq_rids) - 1).bit_length())
    if code_bits + cnt_bits + idx_bits <= _PACK_BITS:
        if nat is not None:
            import torch

            combo = nat.mpc_combo(
                codes32, off_t,
                torch.from_numpy(kcounts[kcode].astype(np.int64)),
                int(cnt_bits), int(idx_bits)).numpy()
        else:
            entry_counts = np.repeat(kcounts[kcode].astype(np.int64),
                                     cluster_sizes)
            inv_idx = (np.int64(n_ent - 1) - np.arange(n_ent, dtype=np.int64))
            combo = ((codes.astype(np.int64) << np.int64(cnt_bits + idx_bits))
                     | (entry_counts << np.int64(idx_bits)) | inv_idx)
        combo.sort()
        dec_code = combo >> np.int64(cnt_bits + idx_bits)
        last = np.flatnonzero(np.r_[dec_code[1:] != dec_code[:-1], True])
        best_entries = (np.int64(n_ent - 1)
                        - (combo[last]
                           & ((np.int64(1) << np.int64(idx_bits)) - 1)))
        best_codes = dec_code[last]
    else:  # astronomically large chains: 3-key lexsort instead of packing
        entry_counts = np.repeat(kcounts[kcode].astype(np.int64),
                                 cluster_sizes)
        order = np.lexsort((-np.arange(n_ent, dtype=np.int64), entry_counts,
                            codes.astype(np.int64)))
        c_sorted = codes[order].astype(np.int64)
        last = np.flatnonzero(np.r_[c_sorted[1:] != c_sorted[:-1], True])
        best_entries = order[last]
        best_codes = c_sorted[last]
    # cluster of each winning entry: searchsorted over the offsets (only
    # ~n_records winners, so no 50M-element repeat of cluster ids needed)
    best_cluster = np.searchsorted(off64, best_entries, side="right") - 1
    best_keys = kcode[best_cluster]
    best_freq = freq_per_cluster[best_cluster]
    return (best_codes, best_keys, best_freq, first_idx, inner_offsets,
            codes_i, uniq_rids, kcode)


def most_probable_clusters_fast(table):
    """{record_id -> (most-probable cluster frozenset, frequency)} — the
    per-record dict view over _mpc_core (LinkageChain.scala:52-64)."""
    (best_codes, best_keys, best_freq, first_idx, inner_offsets, codes_i,
     uniq_rids, _kcode) = _mpc_core(table)
    uniq_list = uniq_rids.tolist()
    bc = best_codes.tolist()
    bk = best_keys.tolist()
    bf = best_freq.tolist()
    out = {}
    fs_cache = {}
    for rc, k, f in zip(bc, bk, bf):
        fs = fs_cache.get(k)
        if fs is None:
            ci = first_idx[k]  # representative cluster instance for this key
            lo, hi = inner_offsets[ci], inner_offsets[ci + 1]
            fs = frozenset(uniq_rids[codes_i[lo:hi]].tolist())
            fs_cache[k] = fs
        out[uniq_list[rc]] = (fs, float(f))
    return out


def shared_most_probable_clusters_fast(table):
    """Vectorized sMPC (LinkageChain.scala:75-109 semantics): records
    grouped by the content key of their most-probable cluster — built
    straight from the integer core, no per-record dict or frozensets."""
    (best_codes, best_keys, _bf, _fi, _io, _ci, uniq_rids, _kc) = (
        _mpc_core(table))
    order = np.argsort(best_keys, kind="stable")
    sk = best_keys[order]
    bounds = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    bounds = np.r_[bounds, len(sk)]
    members = uniq_rids[best_codes[order]]
    return [set(members[bounds[i]:bounds[i + 1]].tolist())
            for i in range(len(bounds) - 1)]


# ---- posterior pairwise link probabilities ----------------------------------

MAX_PAIR_IDS = 2**31 - 1  # rank codes a < b must fit 31 bits of a pair key
DEFAULT_CHUNK_PAIRS = 1 << 24
PAIR_PROB_FILE = "pairwise-link-probabilities.csv"


def _check_id_count(n):
    if n > MAX_PAIR_IDS:
        raise ValueError(
            f"the chain holds {n} distinct record ids; pairwise link counts "
            f"pack two id ranks into one 64-bit key and support at most "
            f"{MAX_PAIR_IDS}")


def _chain_rank_codes(table):
    """Flatten the chain -> (uniq_ids, codes, offsets, S): the distinct
    member ids in Python string order, each member's rank among them (int32)
    and the int64 offsets of the cluster instances in ``codes``."""
    import pyarrow as pa

    col = table["linkageStructure"].combine_chunks()
    if isinstance(col, pa.ChunkedArray):
        col = col.combine_chunks()
    clusters = col.flatten()
    offsets = np.asarray(clusters.offsets).astype(np.int64)
    members = clusters.flatten()
    if isinstance(members, pa.ChunkedArray):
        members = members.combine_chunks()
    enc = members.dictionary_encode()
    ids = enc.dictionary.to_pylist()
    _check_id_count(len(ids))
    # re-rank the dictionary codes by the sorted id strings, so that code
    # order is the canonical output order
    order = sorted(range(len(ids)), key=ids.__getitem__)
    rank = np.empty(len(ids), dtype=np.int32)
    rank[order] = np.arange(len(ids), dtype=np.int32)
    uniq_ids = np.empty(len(ids), dtype=object)
    uniq_ids[:] = [ids[i] for i in order]
    codes = rank[np.asarray(enc.indices)] if len(ids) else np.empty(0, np.int32)
    S = len(np.unique(np.asarray(table["iteration"].to_numpy())))
    return uniq_ids, np.ascontiguousarray(codes, dtype=np.int32), offsets, S


def _pairs_per_cluster(offsets):
    s = np.diff(offsets)
    return s * (s - 1) // 2


def _pair_chunks(pair_ptr, chunk_pairs):
    """Cluster ranges [c0, c1) of at most ``chunk_pairs`` pairs each; a
    single cluster above that goes alone."""
    C = len(pair_ptr) - 1
    c0 = 0
    while c0 < C:
        c1 = int(np.searchsorted(pair_ptr, pair_ptr[c0] + chunk_pairs,
                                 side="right")) - 1
        c1 = min(max(c1, c0 + 1), C)
        yield c0, c1
        c0 = c1


def _tri_decode(t):
    """Pair index t -> (i, j), i < j, t = j (j - 1) / 2 + i: an fp64 root,
    then an integer fix-up (the same decode as pair_counts.hip)."""
    j = ((1.0 + np.sqrt(1.0 + 8.0 * t.astype(np.float64))) * 0.5).astype(np.int64)
    np.maximum(j, 1, out=j)
    while True:
        high = j * (j - 1) // 2 > t
        low = (j + 1) * j // 2 <= t
        if not (high.any() or low.any()):
            break
        j = j - high + low
    return t - j * (j - 1) // 2, j


def _pair_keys_numpy(codes, offsets, pair_ptr, c0, c1):
    """The (a << 32 | b) key, a < b, of every member pair of clusters
    [c0, c1); a pair of equal codes (a duplicated member) is skipped."""
    n_pairs = np.diff(pair_ptr[c0:c1 + 1])
    cl = np.repeat(np.arange(c0, c1, dtype=np.int64), n_pairs)
    t = np.arange(pair_ptr[c0], pair_ptr[c1], dtype=np.int64) - pair_ptr[cl]
    i, j = _tri_decode(t)
    base = offsets[cl]
    x = codes[base + i].astype(np.int64)
    y = codes[base + j].astype(np.int64)
    keep = x != y
    x, y = x[keep], y[keep]
    return (np.minimum(x, y) << np.int64(32)) | np.maximum(x, y)


def _merge_key_counts(keys, counts):
    """Distinct sorted keys and their summed counts."""
    if len(keys) == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    return keys[starts], np.add.reduceat(counts, starts).astype(np.int64)


def _pair_counts_numpy(codes, offsets, pair_ptr, chunk_pairs):
    ks, cs = [], []
    for c0, c1 in _pair_chunks(pair_ptr, chunk_pairs):
        k, c = np.unique(_pair_keys_numpy(codes, offsets, pair_ptr, c0, c1),
                         return_counts=True)
        ks.append(k)
        cs.append(c.astype(np.int64))
    if not ks:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    return _merge_key_counts(np.concatenate(ks), np.concatenate(cs))


def _pair_counts_gpu(codes, offsets, pair_ptr, chunk_pairs, initial_capacity=None,
                     after_add=None):
    """Counts through the device hash table; ``after_add(table)`` is called
    after every chunk (tests watch the table grow through it)."""
    import torch

    from ..ops import PairCountTable

    kw = {} if initial_capacity is None else {"initial_capacity": initial_capacity}
    tab = PairCountTable(device="cuda", **kw)
    codes_d = torch.from_numpy(codes).to(tab.device)
    for c0, c1 in _pair_chunks(pair_ptr, chunk_pairs):
        lo, hi = int(offsets[c0]), int(offsets[c1])
        off_d = torch.from_numpy(offsets[c0:c1 + 1] - lo).to(tab.device)
        tab.add(codes_d[lo:hi], off_d, int(pair_ptr[c1] - pair_ptr[c0]))
        if after_add is not None:
            after_add(tab)
    keys, counts = tab.finish()
    return keys.cpu().numpy(), counts.cpu().numpy()


def pair_counts_from_codes(codes, offsets, device=None, chunk_pairs=None, **gpu_kw):
    """Sorted distinct pair keys ``(a << 32) | b`` (a < b) and their int64
    counts over the clusters ``codes[offsets[c]:offsets[c + 1]]``.
    ``device`` "cpu" / "cuda" forces the arm; None asks
    ``ops.pair_counts_route``."""
    from .. import ops

    codes = np.ascontiguousarray(codes, dtype=np.int32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if len(codes) and (codes.min() < 0):
        raise ValueError("member codes must be non-negative")
    chunk_pairs = DEFAULT_CHUNK_PAIRS if chunk_pairs is None else int(chunk_pairs)
    if chunk_pairs < 1:
        raise ValueError("chunk_pairs must be positive")
    pair_ptr = np.zeros(len(offsets), dtype=np.int64)
    np.cumsum(_pairs_per_cluster(offsets), out=pair_ptr[1:])
    if device is None:
        cuda = False
        if ops.have_pair_table():
            import torch

            cuda = torch.cuda.is_available()
        route = ops.pair_counts_route(int(pair_ptr[-1]), cuda)
    else:
        kind = str(device).split(":")[0]
        if kind not in ("cpu", "cuda"):
            raise ValueError(f"device must be 'cpu', 'cuda' or None, not {device!r}")
        route = "gpu" if kind == "cuda" else "numpy"
    if route == "gpu":
        return _pair_counts_gpu(codes, offsets, pair_ptr, chunk_pairs, **gpu_kw)
    return _pair_counts_numpy(codes, offsets, pair_ptr, chunk_pairs)


def pairwise_link_counts(table, device=None, chunk_pairs=None):
    """Co-clustering counts of record pairs along the chain.

    Returns ``(uniq_ids, a, b, count, S)``: the distinct record ids in
    string order, the rank codes ``a < b`` into them of every pair that
    shares a cluster at least once (sorted by ``(a, b)``), the number of
    cluster instances holding both (int64) and the number of samples S
    (distinct iterations). ``count / S`` is the posterior link probability.
    """
    uniq_ids, codes, offsets, S = _chain_rank_codes(table)
    keys, count = pair_counts_from_codes(codes, offsets, device, chunk_pairs)
    a = (keys >> np.int64(32)).astype(np.int64)
    b = (keys & np.int64(0xFFFFFFFF)).astype(np.int64)
    return uniq_ids, a, b, count, S


def min_link_count(min_probability, S):
    """Smallest integer count with ``count / S >= min_probability``. The
    probability is read as the decimal number it prints as (0.1 is one
    tenth), so the comparison is exact: 0.5 with S = 4 gives 2."""
    from fractions import Fraction

    p = float(min_probability)
    if not 0.0 <= p <= 1.0:
        raise ValueError("min_probability must lie in [0, 1]")
    need = Fraction(repr(p)) * S
    return -(-need.numerator // need.denominator)


def pairwise_link_probabilities(table, min_probability=0.0, device=None):
    """DataFrame (recordId1, recordId2, probability) of the pairs whose
    posterior link probability is positive and at least ``min_probability``;
    recordId1 < recordId2, rows sorted by (recordId1, recordId2)."""
    return link_probability_frame(
        *pairwise_link_counts(table, device=device), min_probability)


def link_probability_frame(uniq_ids, a, b, count, S, min_probability=0.0):
    """The ``pairwise_link_probabilities`` frame from link counts as
    ``pairwise_link_counts`` (or the online accumulator) returns them."""
    import pandas as pd

    keep = count >= max(1, min_link_count(min_probability, S))
    a, b, count = a[keep], b[keep], count[keep]
    return pd.DataFrame({
        "recordId1": uniq_ids[a],
        "recordId2": uniq_ids[b],
        "probability": count / float(S) if S else count.astype(np.float64),
    })


def save_pairwise_link_probabilities(df, output_path):
    """CSV ``recordId1,recordId2,probability``; the probability is written
    with repr(), so it reads back to the same float."""
    import csv

    path = os.path.join(output_path, PAIR_PROB_FILE)
    with open(path, "w", encoding="utf-8", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["recordId1", "recordId2", "probability"])
        w.writerows(zip(df["recordId1"].tolist(), df["recordId2"].tolist(),
                        (repr(float(p)) for p in df["probability"].tolist())))
    return path


def read_pairwise_link_probabilities(path):
    import csv

    import pandas as pd

    if os.path.isdir(path):
        path = os.path.join(path, PAIR_PROB_FILE)
    id1, id2, prob = [], [], []
    with open(path, "r", encoding="utf-8", newline="") as f:
        rows = csv.reader(f)
        header = next(rows)
        if header != ["recordId1", "recordId2", "probability"]:
            raise ValueError(f"{path}: unexpected header {header}")
        for r in rows:
            id1.append(r[0])
            id2.append(r[1])
            prob.append(float(r[2]))
    return pd.DataFrame({
        "recordId1": np.array(id1, dtype=object),
        "recordId2": np.array(id2, dtype=object),
        "probability": np.array(prob, dtype=np.float64),
    })


# ---- most probable clusters from cluster counts -------------------------------
#
# Cluster frequencies counted while the chain is sampled (the device
# ClusterCountTable, or the numpy arm below) instead of from the saved chain.
# One distinct cluster is one entry of five parallel arrays
#
#   keys [n] int64     content key (cluster_keys_numpy), distinct
#   counts [n] int64   number of samples that contain the cluster
#   first [n] int64    chain iteration at which it was first seen
#   offsets [n + 1]    int64 offsets of its members in ``members``
#   members            int32 gids, in any order inside a cluster
#
# As in _mpc_core, a cluster is identified by its 64-bit content key; two
# different member sets with one key would be counted as one, which is
# negligible (two independent 64-bit sums plus the size).

CLUSTER_KEY_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)  # the tables' free-slot marker
SMPC_FILE = "shared-most-probable-clusters.csv"


def cluster_keys_numpy(gids, offsets):
    """int64 content keys of the clusters ``gids[offsets[c]:offsets[c + 1]]``:
    the integers of ``_mpc_keys_numpy`` over the gids, with the all-ones
    pattern (the device table's EMPTY marker) remapped to 0xFFFF...FE. The
    device kernel computes the same integers."""
    off64 = np.asarray(offsets, dtype=np.int64)
    codes = np.asarray(gids).astype(np.uint64)
    with np.errstate(over="ignore"):
        key = _mpc_keys_numpy(codes, off64, np.diff(off64))
    key = np.asarray(key, dtype=np.uint64).copy()
    key[key == CLUSTER_KEY_EMPTY] = CLUSTER_KEY_EMPTY - np.uint64(1)
    return key.view(np.int64)


def _empty_cluster_counts():
    z = np.empty(0, np.int64)
    return z, z.copy(), z.copy(), np.zeros(1, np.int64), np.empty(0, np.int32)


def _gather_segments(starts, sizes):
    """Indices of the concatenated ranges [starts[i], starts[i] + sizes[i])."""
    total = int(sizes.sum())
    out_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=out_off[1:])
    idx = np.arange(total, dtype=np.int64) + np.repeat(starts - out_off[:-1], sizes)
    return idx, out_off


def cluster_counts_of_sample(gids, offsets, iteration):
    """One sample's clusters as a cluster-count tuple (every count 1, first
    = ``iteration``); empty clusters are dropped."""
    offsets = np.asarray(offsets, dtype=np.int64)
    sizes = np.diff(offsets)
    keys = cluster_keys_numpy(gids, offsets)
    keep = sizes > 0
    idx, out_off = _gather_segments(offsets[:-1][keep], sizes[keep])
    n = int(keep.sum())
    part = (keys[keep], np.ones(n, np.int64), np.full(n, int(iteration), np.int64),
            out_off, np.asarray(gids)[idx].astype(np.int32))
    return merge_cluster_counts([part])


def merge_cluster_counts(parts):
    """Merge ``(keys, counts, first, offsets, members)`` tuples (the ranks of
    a run, or a loaded file and the device table) into one, sorted by key:
    equal keys add their counts, ``first`` becomes the minimum, and the
    members are taken from one of the parts."""
    parts = [p for p in parts if len(p[0])]
    if not parts:
        return _empty_cluster_counts()
    keys = np.concatenate([np.asarray(p[0], np.int64) for p in parts])
    counts = np.concatenate([np.asarray(p[1], np.int64) for p in parts])
    first = np.concatenate([np.asarray(p[2], np.int64) for p in parts])
    sizes = np.concatenate([np.diff(np.asarray(p[3], np.int64)) for p in parts])
    members = np.concatenate([np.asarray(p[4], np.int32) for p in parts])
    base = np.cumsum([0] + [len(p[4]) for p in parts[:-1]])
    starts = np.concatenate([np.asarray(p[3], np.int64)[:-1] + b
                             for p, b in zip(parts, base)])
    order = np.argsort(keys, kind="stable")
    keys = keys[order]
    grp = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    rep = order[grp]  # the members of a group's first part stand for all
    idx, out_off = _gather_segments(starts[rep], sizes[rep])
    return (keys[grp], np.add.reduceat(counts[order], grp).astype(np.int64),
            np.minimum.reduceat(first[order], grp).astype(np.int64), out_off,
            members[idx])


def _mpc_best(keys, counts, first, offsets, members):
    """(gids, cluster index): for every gid in ``members`` (sorted,
    distinct) the cluster with the largest count, the smallest ``first``
    among equal counts. The clusters are ranked once (count descending,
    then ``first`` ascending) and their members laid out in that order, so
    a gid's winner is its first occurrence: no sort over the members unless
    the gids are too sparse for a dense position table."""
    counts, first = np.asarray(counts, np.int64), np.asarray(first, np.int64)
    offsets = np.asarray(offsets, np.int64)
    ranked = np.lexsort((first, -counts))
    sizes = np.diff(offsets)[ranked]
    idx, _ = _gather_segments(offsets[:-1][ranked], sizes)
    gid = np.asarray(members)[idx].astype(np.int64)
    cl = np.repeat(ranked, sizes)
    n = len(gid)
    if n == 0:
        return np.empty(0, np.int64), np.empty(0, np.int64)
    top = int(gid.max())
    if top < 4 * n + 1024:
        # reversed fancy assignment leaves the FIRST occurrence
        pos = np.full(top + 1, -1, dtype=np.int64)
        pos[gid[::-1]] = np.arange(n - 1, -1, -1, dtype=np.int64)
        gids = np.flatnonzero(pos >= 0)
        return gids, cl[pos[gids]]
    order = np.argsort(gid, kind="stable")  # keeps the first occurrence first
    g = gid[order]
    lead = np.flatnonzero(np.r_[True, g[1:] != g[:-1]])
    return g[lead], cl[order][lead]


def mpc_from_cluster_counts(keys, counts, first, offsets, members, S):
    """Per record the most probable cluster: ``(gids, best_key, best_count,
    best_freq)`` with ``best_freq = best_count / S``, gids sorted.

    The winner has the largest count; ties go to the cluster with the
    smallest ``first``. Two clusters that hold one record cannot first
    appear in the same iteration, so the winner is unique. This is the tie
    rule of ``most_probable_clusters`` and ``_mpc_core`` on a chain table
    whose rows are in iteration order (they keep the cluster met first)."""
    gids, best = _mpc_best(keys, counts, first, offsets, members)
    cnt = np.asarray(counts, np.int64)[best]
    return gids, np.asarray(keys, np.int64)[best], cnt, cnt / S


def smpc_from_cluster_counts(keys, counts, first, offsets, members, S, ids=None):
    """The sMPC estimate as ``save_clusters_csv`` takes it: records grouped
    by their most probable cluster (tie rule of ``mpc_from_cluster_counts``,
    equal to ``shared_most_probable_clusters`` on a chain table in
    iteration order). Members are ``ids[gid]``, or the gids without ``ids``."""
    gids, best = _mpc_best(keys, counts, first, offsets, members)
    order = np.argsort(best, kind="stable")
    sb = best[order]
    bounds = np.r_[np.flatnonzero(np.r_[True, sb[1:] != sb[:-1]]), len(sb)] \
        if len(sb) else np.zeros(1, np.int64)
    names = gids[order].tolist()
    if ids is not None:
        names = [ids[g] for g in names]
    return [set(names[bounds[i]:bounds[i + 1]]) for i in range(len(bounds) - 1)]


def mpc_dict(keys, counts, first, offsets, members, S, ids=None):
    """``{record id: (frozenset of the most probable cluster, frequency)}``,
    the view ``most_probable_clusters`` gives over a chain table in
    iteration order (same tie rule, see ``mpc_from_cluster_counts``)."""
    gids, best = _mpc_best(keys, counts, first, offsets, members)
    offsets = np.asarray(offsets, np.int64)
    counts = np.asarray(counts, np.int64)
    name = (lambda g: int(g)) if ids is None else (lambda g: ids[int(g)])
    sets, out = {}, {}
    for g, c in zip(gids.tolist(), best.tolist()):
        fs = sets.get(c)
        if fs is None:
            fs = sets[c] = frozenset(
                name(m) for m in np.asarray(members)[offsets[c]:offsets[c + 1]].tolist())
        out[name(g)] = (fs, int(counts[c]) / S)
    return out
