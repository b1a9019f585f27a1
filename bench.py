"""Flagship benchmark: Gibbs iterations/sec on RLdata10000-shaped data.

Driver contract:
    python bench.py --gpus N --steps K --warmup W
(for N > 1 launched via torch.distributed.run with one rank per GPU over RCCL)

Measures the BASELINE.json metric — "Gibbs iterations/sec (whole node) on
RLdata10000-shape" — with the PCG-I sampler on synthetic RLdata-shaped
records (same schema: 3 constant-sim + 2 Levenshtein attributes, 10%
duplicates; there is no network access for the original RLdata files) and
random/deterministic-init latent state. Weak scaling: each GPU holds an
RLdata10000-shaped shard (10,000 records, 4 KD-tree partitions), so the
whole-job iteration size grows with N while iterations/sec is reported for
the whole job.

Timing: W untimed warm-up sweeps, then K sweeps bracketed by a barrier +
torch.cuda.synchronize() on both sides; MAX elapsed over ranks; rank 0
prints one JSON line. Every timed sweep includes the full Markov transition
the reference times in its diagnostics loop: theta update, link/value/
distortion updates, partition reassignment, migration all-to-all, and the
summary all-reduce. Sample/diagnostic file writes are excluded (the
reference amortizes them 1/thinningInterval = 1/10; checkpointing off).

A plain run does only that. ``--full`` adds the secondary figures (ESS and
ESS/sec of the timed region, the sampler's path counters);
``--dump-outputs DIR`` writes the chain state the last timed sweep produced
as ``DIR/<name>.npy`` so two builds can be compared output for output (the
data and the chain are fully determined by the arguments).
"""

from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import numpy as np


def build_cache_and_records(total_records, seed, schema="rldata", num_files=1):
    """Synthetic data + cache for the BASELINE.json configs.

    schema "rldata": 5 attrs (by, bm, bd constant; fname_c1, lname_c1
    Levenshtein) — configs #1-#3 and #5. schema "strings8": 8 Levenshtein
    string attributes — config #4 (10M-record HBM sizing).
    """
    from dblink_amd.models.records import (
        Attribute,
        BetaShapeParameters,
        RecordsCache,
        RecordsTable,
    )
    from dblink_amd.models.similarity import ConstantSimilarityFn, LevenshteinSimilarityFn
    from dblink_amd.utils.synthdata import generate

    extra = 6 if schema == "strings8" else 0
    cols, header = generate(
        total_records, dup_fraction=0.1, seed=seed, num_files=num_files,
        extra_string_attrs=extra,
    )
    prior = BetaShapeParameters(10.0, 1000.0)  # RLdata10000.conf:4
    lev = lambda: LevenshteinSimilarityFn(7.0, 10.0)
    if schema == "strings8":
        attr_names = ["fname_c1", "lname_c1"] + [f"xattr{j}" for j in range(6)]
        attrs = [Attribute(n, lev(), prior) for n in attr_names]
    else:
        attr_names = ["by", "bm", "bd", "fname_c1", "lname_c1"]
        attrs = [
            Attribute("by", ConstantSimilarityFn(), prior),
            Attribute("bm", ConstantSimilarityFn(), prior),
            Attribute("bd", ConstantSimilarityFn(), prior),
            Attribute("fname_c1", lev(), prior),
            Attribute("lname_c1", lev(), prior),
        ]
    columns = [np.where(cols[a] == "NA", None, cols[a]) for a in attr_names]
    table = RecordsTable(cols["rec_id"], cols["file_id"], columns)
    cache = RecordsCache.build(table, attrs, max_cluster_size=10)
    rec_values, rec_files = cache.transform_records(table)
    return cache, rec_values, rec_files


DUMP_MAX_BYTES = 64 << 20


def dump_outputs(dirname, state, loglik_series, nobs_series, rank=0, world=1):
    """Write what the last timed sweep left in ``state`` as DIR/<name>.npy.

    Per-record arrays are put in global-record-id order and entities are named
    by the smallest record id linked to them, so the files do not depend on
    the engine's internal row order or entity numbering. Everything is
    float64 (the ids are far below 2^53). Per-record arrays larger than the
    byte budget are cut down to a fixed, seeded sample of records; the
    sampled ids are written alongside.
    """
    os.makedirs(dirname, exist_ok=True)
    R, A = state.rec_values.shape
    order = np.argsort(state.rec_gid, kind="stable")
    small = {
        "dist_probs": np.asarray(state.dist_probs.probs),
        "summary_scalars": np.array([state.iteration, state.summary.log_likelihood,
                                     state.summary.num_isolates]),
        "summary_agg_distortions": state.summary.agg_distortions,
        "summary_rec_distortions": state.summary.rec_distortions,
        "loglik_series": loglik_series,
        "num_observed_series": nobs_series,
    }
    budget = DUMP_MAX_BYTES - sum(8 * np.size(v) for v in small.values())
    max_rows = max(1, budget // (8 * (2 * A + 2)))
    if R > max_rows:
        pick = np.sort(np.random.default_rng(0).choice(R, size=max_rows, replace=False))
        order = order[pick]
    # cluster label: smallest global record id linked to the same entity
    ent_min_gid = np.full(state.num_entities, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(ent_min_gid, state.rec_ent, state.rec_gid)
    per_record = {
        "rec_gid": state.rec_gid[order],
        "rec_cluster": ent_min_gid[state.rec_ent[order]],
        "rec_entity_values": state.ent_values[state.rec_ent[order]],
        "rec_distortions": state.rec_dist[order],
    }
    suffix = f"_rank{rank}" if world > 1 else ""
    for name, arr in {**small, **per_record}.items():
        np.save(os.path.join(dirname, f"{name}{suffix}.npy"),
                np.ascontiguousarray(arr, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed sweeps; default: auto-calibrated so the timed "
                         "region is >= ~6 s")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--records-per-gpu", type=int, default=10000)
    ap.add_argument("--partitions-per-gpu", type=int, default=4)
    ap.add_argument("--sampler", default="PCG-I")
    ap.add_argument("--seed", type=int, default=319158)
    ap.add_argument("--cpu", action="store_true", help="force the CPU engine")
    ap.add_argument("--schema", default="rldata", choices=["rldata", "strings8"],
                    help="rldata: 3 const + 2 Levenshtein attrs; strings8: 8 Levenshtein attrs")
    ap.add_argument("--num-files", type=int, default=1,
                    help="number of source files (per-file distortion probabilities)")
    ap.add_argument("--dump-state", default=None, metavar="DIR",
                    help="run the warmup sweeps, save the chain state, exit "
                         "(for profiling the stationary regime)")
    ap.add_argument("--init-state", default=None, metavar="DIR",
                    help="resume the chain from a saved state instead of "
                         "deterministic init")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed sweeps, write the chain state the "
                         "last sweep produced as DIR/<name>.npy (float64)")
    ap.add_argument("--full", action="store_true",
                    help="also report the secondary figures: ESS and ESS/sec of "
                         "the timed region and the sampler's path counters")
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch

    from dblink_amd.engine.cpu_engine import CpuEngine, SamplerFlags
    from dblink_amd.engine.init import deterministic_init
    from dblink_amd.parallel import comm
    from dblink_amd.parallel.partitioning import KDTreePartitioner

    rank, world, device = comm.init_from_env()
    n_gpus = world if world > 1 else args.gpus
    use_gpu = torch.cuda.is_available() and not args.cpu

    total_records = args.records_per_gpu * n_gpus
    total_partitions = args.partitions_per_gpu * n_gpus
    num_levels = max(0, int(round(math.log2(total_partitions))))

    t_init = time.time()
    cache, rec_values, rec_files = build_cache_and_records(
        total_records, args.seed, schema=args.schema, num_files=args.num_files
    )
    if rank == 0:
        print(f"[bench] data+cache built in {time.time() - t_init:.1f}s "
              f"(V = {[ia.index.num_values for ia in cache.indexed_attributes]})",
              file=sys.stderr)

    part_attrs = [3, 4] if args.schema == "rldata" else [0, 1]  # Levenshtein attrs
    partitioner = KDTreePartitioner(num_levels, part_attrs)
    if args.init_state:
        from dblink_amd.engine.state import ChainState

        state = ChainState.load(args.init_state, rank=rank, world_size=world)
        saved = getattr(state, "saved_partitioner", None)
        if saved is not None:
            partitioner = saved
    else:
        bounds = np.linspace(0, total_records, world + 1).astype(np.int64)
        lo, hi = int(bounds[rank]), int(bounds[rank + 1])
        state = deterministic_init(
            rec_values[lo:hi], rec_files[lo:hi], np.arange(lo, hi, dtype=np.int64),
            cache, partitioner, args.seed, rank=rank, world_size=world,
        )

    if rank == 0:
        print(f"[bench] init state in {time.time() - t_init:.1f}s total", file=sys.stderr)
    if use_gpu:
        from dblink_amd.engine.gpu_engine import GpuEngine

        engine = GpuEngine(cache, partitioner, world_size=world, rank=rank, device=device)
    else:
        engine = CpuEngine(cache, partitioner, world_size=world, rank=rank)
    engine.initial_summary(state)
    flags = SamplerFlags.for_sampler(args.sampler)

    def sync():
        comm.barrier()
        if use_gpu:
            torch.cuda.synchronize()

    sync()
    t_w = time.time()
    for _ in range(args.warmup):
        engine.step(state, flags)
    sync()
    t_w = time.time() - t_w

    if args.dump_state:
        if hasattr(engine, "sync_state"):
            engine.sync_state(state)
        state.save(args.dump_state, rank=rank, world_size=world,
                   extra={"partitioner": engine.partitioner})
        if rank == 0:
            print(f"[bench] state after {args.warmup} sweeps saved to "
                  f"{args.dump_state}", file=sys.stderr)
        return

    if args.steps is None:
        # calibrate on a WARM probe (the warmup itself includes first-call
        # compile/caching cost) so the timed region lands near the target
        # (a 7 ms timed region is not a measurement)
        probe = 5
        sync()
        t_p = time.time()
        for _ in range(probe):
            engine.step(state, flags)
        sync()
        per_step = (time.time() - t_p) / probe
        args.steps = int(min(max(math.ceil(6.0 / max(per_step, 1e-9)), 50), 50000))
        if comm.is_distributed():
            import torch.distributed as dist

            st = torch.tensor([args.steps], dtype=torch.int64,
                              device=device if use_gpu else "cpu")
            dist.all_reduce(st, op=dist.ReduceOp.MIN)
            args.steps = int(st.cpu())
        if rank == 0:
            print(f"[bench] auto-calibrated --steps {args.steps} "
                  f"({per_step * 1000:.3f} ms/step warm)", file=sys.stderr)

    # per-sweep summary series for the ESS/sec secondary metric
    loglik_series = np.empty(args.steps, dtype=np.float64)
    nobs_series = np.empty(args.steps, dtype=np.float64)
    sync()
    t0 = time.time()
    for k in range(args.steps):
        engine.step(state, flags)
        loglik_series[k] = state.summary.log_likelihood
        nobs_series[k] = state.population_size - state.summary.num_isolates
    sync()
    elapsed = time.time() - t0

    # max over ranks
    t = torch.tensor([elapsed], dtype=torch.float64,
                     device=device if use_gpu else "cpu")
    if comm.is_distributed():
        import torch.distributed as dist

        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.cpu())

    if args.dump_outputs:
        if hasattr(engine, "sync_state"):
            engine.sync_state(state)
        dump_outputs(args.dump_outputs, state, loglik_series, nobs_series,
                     rank=rank, world=world)

    if args.full and rank == 0 and getattr(engine, "_heavy_stats", None) is not None:
        hs = engine._heavy_stats.cpu().numpy()
        if hs[3]:
            print(f"[bench] heavy link sampler: {int(hs[3])} records, "
                  f"{int(hs[2])} similar-set visits, {int(hs[0])} A* iterations, "
                  f"{int(hs[1])} full-scan fallbacks (all sweeps)", file=sys.stderr)

    if args.full and rank == 0 and getattr(engine, "_value_stats", None) is not None:
        vs = engine._value_stats.cpu().numpy()
        print(f"[bench] value k>=2: {int(vs[0])} pairs ({int(vs[1])} hash / "
              f"{int(vs[2])} merge / {int(vs[6])} k>Kc), sum_entries={int(vs[3])} "
              f"(merge {int(vs[7])}), sum_tsize={int(vs[4])}, sum_k={int(vs[5])} "
              f"(all sweeps)", file=sys.stderr)

    phase_ms = None
    if rank == 0 and hasattr(engine, "phase_times") and getattr(engine, "phase_timers", False):
        pt = engine.phase_times()
        total = sum(pt.values()) or 1.0
        nsweeps = args.steps + args.warmup
        phase_ms = {k: v / nsweeps for k, v in sorted(pt.items(), key=lambda kv: -kv[1])}
        detail = ", ".join(f"{k}={v:.3f}ms({100*pt[k]/total:.0f}%)"
                           for k, v in phase_ms.items())
        print(f"[bench] phase times per sweep: {detail}", file=sys.stderr)

    if rank == 0:
        value = args.steps / elapsed
        # ESS/sec secondary metric (BASELINE.json): Geyer initial-monotone
        # ESS of the per-sweep summary series over the timed region (--full)
        ess_loglik = ess_nobs = None
        if args.full and args.steps >= 50:
            from dblink_amd.analysis.diagnostics import ess as _ess

            ess_loglik = _ess(loglik_series)
            ess_nobs = _ess(nobs_series)
        ess_per_sec = (
            min(ess_loglik, ess_nobs) / elapsed if ess_loglik is not None else None
        )
        out = {
            "metric": "Gibbs iterations/sec (whole node) on RLdata10000-shape",
            "value": value,
            "unit": "iterations/sec",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp32",
            "data": "synthetic",
            "ess_per_sec": ess_per_sec,
            "ess": {"logLikelihood": ess_loglik, "numObservedEntities": ess_nobs},
            "phase_ms_per_step": phase_ms,
            "config": {
                "model": "dblink PCG-I partitioned Gibbs (RLdata10000 schema: "
                         "3 constant + 2 Levenshtein attributes, 10% duplicates)",
                "records_per_gpu": args.records_per_gpu,
                "global_records": total_records,
                "partitions": total_partitions,
                "sampler": args.sampler,
                "schema": args.schema,
                "num_files": args.num_files,
                "parallelism": (
                    f"entity-partitioned Gibbs, {n_gpus} rank(s) over "
                    + (torch.distributed.get_backend().upper().replace("NCCL", "RCCL")
                       if comm.is_distributed() else ("RCCL" if use_gpu else "local"))
                ),
                "engine": "gpu" if use_gpu else "cpu",
            },
        }
        print(json.dumps(out))


if __name__ == "__main__":
    main()
