"""Three ways to count the chain's co-clustered record pairs, on one input.

    python scripts/pair_counts_bench.py [--records 10000 100000 1000000]
                                        [--samples 100] [--reps 5]

Arms, all from the same host arrays (member codes + cluster offsets) to
host (sorted keys, counts), so transfers are inside every GPU figure:
  (a) numpy   the reference arm of analysis.chain (np.unique per chunk)
  (b) hash    the device pair-count hash table (pair_counts.hip)
  (c) sort    torch only: emit keys, torch.sort, unique_consecutive, merge

The chain is synthetic and flattened directly (no Parquet, no sampler): R
records in clusters of the RLdata-like size mix, S samples, and a fraction
of the records re-linked at random in every sample so that the number of
distinct pairs grows with S. Each arm gets one warm-up run, then up to
--reps timed runs (fewer once --budget seconds are spent; an arm whose
warm-up alone takes longer, as numpy does at 10^6 records, reports that one
run and says so); the device is synchronised around every timed
run. Reported: median and min..max in ms, pair occurrences per second at the
median, and the hash table's final capacity and bytes. (b) and (c) must
equal (a) exactly at the smallest shape before anything is timed.
"""

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dblink_amd.analysis import chain as chain_q  # noqa: E402

SIZE_MIX = (1, 1, 1, 2, 2, 3, 5, 17)


def synthetic_chain(R, S, move_fraction=0.02, seed=0):
    """-> (codes int32 [R * S], offsets int64): per sample, the records
    grouped by entity; entities come from one base clustering with
    move_fraction of the records re-linked to a random entity."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice(SIZE_MIX, size=R)  # more than enough clusters
    sizes = sizes[: int(np.searchsorted(np.cumsum(sizes), R)) + 1]
    base = np.repeat(np.arange(len(sizes)), sizes)[:R]
    base = base[rng.permutation(R)]
    E = int(base.max()) + 1
    codes = np.empty(R * S, dtype=np.int32)
    offsets = [np.zeros(1, dtype=np.int64)]
    n_move = int(R * move_fraction)
    for s in range(S):
        ent = base.copy()
        ent[rng.choice(R, n_move, replace=False)] = rng.integers(0, E, n_move)
        codes[s * R:(s + 1) * R] = np.argsort(ent, kind="stable")
        cnt = np.bincount(ent, minlength=E)
        offsets.append(np.cumsum(cnt[cnt > 0]) + s * R)
    return codes, np.concatenate(offsets).astype(np.int64)


def _tri_decode_torch(t):
    j = ((1.0 + torch.sqrt(1.0 + 8.0 * t.double())) * 0.5).long().clamp_(min=1)
    j -= (j * (j - 1) // 2 > t).long()
    j += ((j + 1) * j // 2 <= t).long()
    return t - j * (j - 1) // 2, j  # fp64 is within one row for t < 2^52


def _unique_counts(keys, weights=None):
    keys, order = torch.sort(keys)
    uk, cnt = torch.unique_consecutive(keys, return_counts=True)
    if weights is None:
        return uk, cnt
    csum = torch.cumsum(weights[order], 0)
    ends = torch.cumsum(cnt, 0) - 1
    tot = csum[ends]
    tot[1:] -= csum[ends[:-1]]
    return uk, tot


def sort_arm(codes, offsets, pair_ptr, chunk_pairs, device="cuda"):
    dev = torch.device(device)
    codes_d = torch.from_numpy(codes).to(dev)
    ks, cs = [], []
    for c0, c1 in chain_q._pair_chunks(pair_ptr, chunk_pairs):
        n_pairs = torch.from_numpy(np.diff(pair_ptr[c0:c1 + 1])).to(dev)
        base = torch.from_numpy(offsets[c0:c1]).to(dev)
        ptr = torch.from_numpy(pair_ptr[c0:c1] - pair_ptr[c0]).to(dev)
        cl = torch.repeat_interleave(torch.arange(c1 - c0, device=dev), n_pairs)
        t = torch.arange(int(pair_ptr[c1] - pair_ptr[c0]), device=dev) - ptr[cl]
        i, j = _tri_decode_torch(t)
        x = codes_d[base[cl] + i].long()
        y = codes_d[base[cl] + j].long()
        keep = x != y
        x, y = x[keep], y[keep]
        k, c = _unique_counts((torch.minimum(x, y) << 32) | torch.maximum(x, y))
        ks.append(k)
        cs.append(c)
    if len(ks) == 1:
        k, c = ks[0], cs[0]
    else:
        k, c = _unique_counts(torch.cat(ks), torch.cat(cs))
    return k.cpu().numpy(), c.cpu().numpy()


def timed(fn, reps, budget):
    t0 = time.perf_counter()
    out = fn()  # warm-up
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    if warm > budget:  # one run already spends the budget: it is the figure
        return out, [warm * 1e3], False
    times, spent = [], 0.0
    while len(times) < reps and (not times or spent < budget):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
        spent += times[-1] / 1e3
    return out, times, True


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, nargs="+", default=[10**4, 10**5, 10**6])
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=45.0,
                    help="seconds of timed runs per arm and shape")
    ap.add_argument("--chunk-pairs", type=int, default=chain_q.DEFAULT_CHUNK_PAIRS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the hash and sort arms need a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
          flush=True)

    for n, R in enumerate(sorted(args.records)):
        codes, offsets = synthetic_chain(R, args.samples)
        pair_ptr = np.zeros(len(offsets), dtype=np.int64)
        np.cumsum(chain_q._pairs_per_cluster(offsets), out=pair_ptr[1:])
        P = int(pair_ptr[-1])
        table = {}

        def keep_table(tab):
            table.update(capacity=tab.capacity, bytes=tab.nbytes,
                         grow_count=tab.grow_count)

        arms = {
            "numpy": lambda: chain_q._pair_counts_numpy(
                codes, offsets, pair_ptr, args.chunk_pairs),
            "hash": lambda: chain_q._pair_counts_gpu(
                codes, offsets, pair_ptr, args.chunk_pairs, after_add=keep_table),
            "sort": lambda: sort_arm(codes, offsets, pair_ptr, args.chunk_pairs),
        }
        if n == 0:  # exact agreement before any timing
            ref = arms["numpy"]()
            for name in ("hash", "sort"):
                got = arms[name]()
                assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), name
            print(f"R={R}: hash and sort arms equal the numpy arm exactly "
                  f"({len(ref[0])} distinct pairs)", flush=True)
        for name, fn in arms.items():
            (keys, _), times, warmed = timed(fn, args.reps, args.budget)
            med = statistics.median(times)
            row = {
                "records": R, "samples": args.samples, "pair_occurrences": P,
                "distinct_pairs": int(len(keys)), "arm": name, "runs": len(times),
                "warmed_up": warmed,
                "median_ms": round(med, 3), "min_ms": round(min(times), 3),
                "max_ms": round(max(times), 3),
                "pairs_per_s": round(P / (med / 1e3)),
            }
            if name == "hash":
                row.update(table)
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
