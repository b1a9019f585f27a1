"""Pair counts fed from device-resident links against the offline route.

    python scripts/pair_links_bench.py [--records 10000 100000 1000000]
                                       [--samples 100] [--reps 5]
                                       [--arms online offline]

The input is the synthetic chain of ``pair_counts_bench.py`` (same size mix,
same share of re-linked records per sample, same random draws), held two ways:
  online   each sample as (rec_ent, rec_gid), int64, resident on the device;
           a run is S x ``PairCountTable.add_links`` plus ``finish()`` to the
           host. Reported per run and per sample (run / S).
  offline  the same samples written once as a Parquet linkage chain (not
           timed); a run is ``load_chain`` -> ``_chain_rank_codes`` ->
           ``pair_counts_from_codes(device="cuda")``, what a summarize step
           does for the quantity.
Each arm gets one warm-up run, then up to --reps timed runs with the device
synchronised around each (fewer once --budget seconds are spent; an arm
whose warm-up alone takes longer reports that one run and says so). Median
and min..max in ms. At the smallest shape the online counts must equal the
numpy arm on the host-grouped links exactly before anything is timed.

The split of ``add_links`` into its kernels comes from a profiler run of the
online arm alone (``--arms online`` under a kernel trace with statistics).
"""

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pair_counts_bench import SIZE_MIX, timed  # noqa: E402

from dblink_amd import ops  # noqa: E402
from dblink_amd.analysis import chain as chain_q  # noqa: E402
from dblink_amd.engine.writers import LinkageChainWriter  # noqa: E402


def synthetic_links(R, S, move_fraction=0.02, seed=0):
    """-> (list of S rec_ent int64 [R], E): the samples of
    ``pair_counts_bench.synthetic_chain`` (the same draws in the same order)
    as link vectors; record r has gid r."""
    rng = np.random.default_rng(seed)
    sizes = rng.choice(SIZE_MIX, size=R)
    sizes = sizes[: int(np.searchsorted(np.cumsum(sizes), R)) + 1]
    base = np.repeat(np.arange(len(sizes)), sizes)[:R]
    base = base[rng.permutation(R)]
    E = int(base.max()) + 1
    n_move = int(R * move_fraction)
    samples = []
    for _ in range(S):
        ent = base.copy()
        ent[rng.choice(R, n_move, replace=False)] = rng.integers(0, E, n_move)
        samples.append(ent.astype(np.int64))
    return samples, E


def grouped(ent):
    """One sample -> (gids grouped by entity, offsets of the non-empty ones)."""
    cnt = np.bincount(ent, minlength=1)
    return (np.argsort(ent, kind="stable"),
            np.r_[0, np.cumsum(cnt[cnt > 0])].astype(np.int64))


def write_chain(samples, path):
    """The samples as a one-partition linkage chain under ``path``."""
    R = len(samples[0])
    ids = np.array([str(i) for i in range(R)], dtype=object)
    w = LinkageChainWriter(path, buffer_size=10)
    for s, ent in enumerate(samples):
        gids, offsets = grouped(ent)
        w.append_arrays(s + 1, np.zeros(1, np.int32),
                        np.array([0, len(offsets) - 1], np.int64), offsets, gids,
                        id_dictionary=ids)
    w.close()


def online_run(ents_d, gid_d, E):
    tab = ops.PairCountTable(device="cuda")
    for ent in ents_d:
        tab.add_links(ent, gid_d, E)
    keys, counts = tab.finish()
    return keys.cpu().numpy(), counts.cpu().numpy(), tab


def offline_run(path):
    table = chain_q.load_chain(path, 0)
    _, codes, offsets, _ = chain_q._chain_rank_codes(table)
    return chain_q.pair_counts_from_codes(codes, offsets, device="cuda")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, nargs="+", default=[10**4, 10**5, 10**6])
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=60.0,
                    help="seconds of timed runs per arm and shape")
    ap.add_argument("--arms", nargs="+", default=["online", "offline"],
                    choices=["online", "offline"])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "both arms need a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
          flush=True)

    for n, R in enumerate(sorted(args.records)):
        samples, E = synthetic_links(R, args.samples)
        P = 0
        for ent in samples:
            cnt = np.bincount(ent)
            P += int((cnt * (cnt - 1) // 2).sum())
        common = {"records": R, "entities": E, "samples": args.samples,
                  "pair_occurrences": P}
        ents_d = [torch.from_numpy(e).cuda() for e in samples]
        gid_d = torch.arange(R, dtype=torch.int64, device="cuda")
        if n == 0:  # exact agreement before any timing
            parts = [chain_q.pair_counts_from_codes(*grouped(e), device="cpu")
                     for e in samples]
            ref = chain_q._merge_key_counts(np.concatenate([k for k, _ in parts]),
                                            np.concatenate([c for _, c in parts]))
            got = online_run(ents_d, gid_d, E)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
            print(f"R={R}: add_links equals the numpy arm exactly "
                  f"({len(ref[0])} distinct pairs)", flush=True)

        def report(arm, out, times, warmed, **extra):
            med = statistics.median(times)
            row = dict(common, arm=arm, distinct_pairs=int(len(out[0])),
                       runs=len(times), warmed_up=warmed,
                       median_ms=round(med, 3), min_ms=round(min(times), 3),
                       max_ms=round(max(times), 3), **extra)
            print(json.dumps(row), flush=True)
            return med

        med = {}
        if "online" in args.arms:
            out, times, warmed = timed(lambda: online_run(ents_d, gid_d, E),
                                       args.reps, args.budget)
            med["online"] = report(
                "online", out, times, warmed,
                per_sample_ms=round(statistics.median(times) / args.samples, 4),
                capacity=out[2].capacity, grow_count=out[2].grow_count)
        if "offline" in args.arms:
            tmp = tempfile.mkdtemp(prefix="pair_links_bench_")
            try:
                write_chain(samples, tmp)
                out, times, warmed = timed(lambda: offline_run(tmp), args.reps,
                                           args.budget)
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
            med["offline"] = report("offline", out, times, warmed)
        if len(med) == 2:
            print(json.dumps(dict(common, offline_over_online=round(
                med["offline"] / med["online"], 2))), flush=True)


if __name__ == "__main__":
    main()
