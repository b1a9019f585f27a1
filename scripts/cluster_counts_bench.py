"""sMPC from cluster counts taken on the device against the offline route.

    python scripts/cluster_counts_bench.py [--records 10000 100000]
                                           [--samples 100] [--reps 5]

The input is the synthetic chain of ``pair_links_bench.py`` (same size mix,
2% of the records re-linked per sample, same random draws), held two ways:
  online   each sample as (rec_ent, rec_gid), int64, resident on the device;
           a run is S x ``ClusterCountTable.add_links``, then ``finish()`` to
           the host, then ``smpc_from_cluster_counts``. The three parts are
           timed inside the run (device synchronised between them); the add
           part is also given per sample (adds / S).
  offline  the same samples as an Arrow linkage-chain table already in
           memory (written and loaded once, not timed); a run is
           ``shared_most_probable_clusters_fast`` over it, what a summarize or
           evaluate step does after loading the chain.
Each arm gets one warm-up run, then up to --reps timed runs; median and
min..max in ms. At every shape the device table must equal the numpy arm
exactly (keys, counts, first iterations, member sets), and the online sMPC
the offline one, before anything is timed.
"""

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from pair_counts_bench import timed  # noqa: E402
from pair_links_bench import grouped, synthetic_links, write_chain  # noqa: E402

from dblink_amd import ops  # noqa: E402
from dblink_amd.analysis import chain as chain_q  # noqa: E402


def online_run(ents_d, gid_d, E, ids):
    """-> (clusters, local counts, table, [adds, finish, resolve] in ms)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tab = ops.ClusterCountTable(device="cuda")
    for s, ent in enumerate(ents_d):
        tab.add_links(ent, gid_d, E, s + 1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    local = tuple(t.cpu().numpy() for t in tab.finish())
    t2 = time.perf_counter()
    clusters = chain_q.smpc_from_cluster_counts(*local, len(ents_d), ids=ids)
    t3 = time.perf_counter()
    return clusters, local, tab, [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]


def numpy_arm(samples):
    parts = []
    for s, ent in enumerate(samples):
        gids, offsets = grouped(ent)
        parts.append(chain_q.cluster_counts_of_sample(gids, offsets, s + 1))
    return chain_q.merge_cluster_counts(parts)


def member_sets(local):
    _, _, _, offsets, members = local
    return [frozenset(members[offsets[i]:offsets[i + 1]].tolist())
            for i in range(len(offsets) - 1)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--records", type=int, nargs="+", default=[10**4, 10**5])
    ap.add_argument("--samples", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--budget", type=float, default=60.0,
                    help="seconds of timed runs per arm and shape")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the online arm needs a GPU"
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
          flush=True)

    for R in sorted(args.records):
        samples, E = synthetic_links(R, args.samples)
        ids = [str(i) for i in range(R)]
        common = {"records": R, "entities": E, "samples": args.samples}
        ents_d = [torch.from_numpy(e).cuda() for e in samples]
        gid_d = torch.arange(R, dtype=torch.int64, device="cuda")
        tmp = tempfile.mkdtemp(prefix="cluster_counts_bench_")
        try:
            write_chain(samples, tmp)
            table = chain_q.load_chain(tmp, 0).sort_by("iteration")
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

        # exact agreement before any timing
        ref = numpy_arm(samples)
        clusters, got, _, _ = online_run(ents_d, gid_d, E, ids)
        for x, y in zip(got[:4], ref[:4]):
            assert np.array_equal(x, y)
        assert member_sets(got) == member_sets(ref)
        offline = chain_q.shared_most_probable_clusters_fast(table)
        assert ({frozenset(c) for c in clusters} == {frozenset(c) for c in offline}
                and len(clusters) == len(offline))
        print(f"R={R}: the device table equals the numpy arm exactly "
              f"({len(ref[0])} distinct clusters, {len(ref[4])} members kept, "
              f"{args.samples * R} seen) and the online sMPC the offline one "
              f"({len(clusters)} clusters)", flush=True)

        def report(arm, times, warmed, **extra):
            row = dict(common, arm=arm, runs=len(times), warmed_up=warmed,
                       median_ms=round(statistics.median(times), 3),
                       min_ms=round(min(times), 3), max_ms=round(max(times), 3),
                       **extra)
            print(json.dumps(row), flush=True)
            return row["median_ms"]

        parts = []

        def online():
            out = online_run(ents_d, gid_d, E, ids)
            parts.append(out[3])
            return out

        out, times, warmed = timed(online, args.reps, args.budget)
        parts = parts[-len(times):]  # the warm-up's split is dropped
        adds, fin, res = (statistics.median(p[i] for p in parts) for i in range(3))
        on = report("online", times, warmed, adds_ms=round(adds, 3),
                    add_per_sample_ms=round(adds / args.samples, 4),
                    finish_ms=round(fin, 3), resolve_ms=round(res, 3),
                    distinct_clusters=int(len(out[1][0])),
                    capacity=out[2].capacity, arena=out[2].arena_capacity,
                    nbytes=out[2].nbytes, grow_count=out[2].grow_count)
        _, times, warmed = timed(
            lambda: chain_q.shared_most_probable_clusters_fast(table),
            args.reps, args.budget)
        off = report("offline", times, warmed)
        print(json.dumps(dict(common, offline_over_online=round(off / on, 2))),
              flush=True)


if __name__ == "__main__":
    main()
