#!/usr/bin/env python3
"""What the longest candidate scans cost link_update at the 10k flagship.

Loads a saved stationary state (bench.py --warmup N --dump-state DIR),
rebuilds the inverted index as GpuEngine._sweep_body does and times
C.link_update with HIP events, once with every record on the wave kernel and
once with the records whose base candidate list exceeds --split masked to
mode 2, which neither kernel of link_update claims. The difference is the
most that taking those records off the wave-per-record path can win. Where
the extension has link_update_split, the split path is timed as well.

    python scripts/link_tail.py STATE_DIR [--split 256] [--reps 200]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def base_lengths(rec_values, rec_dist, rec_part, cand_lo, cand_hi, ent_ptr):
    """Base-list length per record by the rule of link_select_base (no
    constant-pair slots): the shortest posting range among the observed
    non-distorted attributes, else the record's whole partition."""
    nd = (rec_values >= 0) & (rec_dist == 0)
    n = np.where(nd, cand_hi - cand_lo, np.iinfo(np.int64).max).min(axis=1)
    pool = ent_ptr[rec_part + 1] - ent_ptr[rec_part]
    return np.where(nd.any(axis=1), n, pool), nd.any(axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("state")
    ap.add_argument("--split", type=int, default=256)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=319158)
    args = ap.parse_args()

    import torch

    import bench
    from dblink_amd.engine.gpu_engine import GpuEngine
    from dblink_amd.engine.state import ChainState

    cache, _, _ = bench.build_cache_and_records(args.records, args.seed)
    state = ChainState.load(args.state, rank=0, world_size=1)
    eng = GpuEngine(cache, state.saved_partitioner, device=torch.device("cuda", 0))
    gs, m, C, dev = eng._gpu_state(state), eng.model, eng.C, eng.device
    A, E, R, P = m.A, gs.E, gs.R, eng.num_partitions
    assert eng._num_pairs == 0
    assert bool((gs.ent_part[1:] >= gs.ent_part[:-1]).all()), "entities not partition-sorted"
    ent_ptr = torch.searchsorted(gs.ent_part.to(torch.int64).contiguous(),
                                 torch.arange(P + 1, device=dev, dtype=torch.int64))
    eng._ensure_idx_buffers(zero=True)
    C.postings_hist(gs.ent_part, gs.ent_values, eng._pair_a1, eng._pair_a2,
                    eng._pair_v2, m.Vmax, eng._idx_counts)
    C.scan_excl(eng._idx_counts, eng._idx_ptr, eng._idx_cursor)
    postings = torch.empty(A * E, dtype=torch.int32, device=dev)
    C.postings_scatter(gs.ent_part, gs.ent_values, eng._pair_a1, eng._pair_a2,
                       eng._pair_v2, m.Vmax, eng._idx_cursor, postings)
    cand_lo = torch.empty((R, A), dtype=torch.int64, device=dev)
    cand_hi = torch.empty((R, A), dtype=torch.int64, device=dev)
    C.cand_ranges(gs.rec_part, gs.rec_values, eng._pair_a1, eng._pair_a2,
                  eng._pair_v2, eng._idx_ptr, m.Vmax, cand_lo, cand_hi)

    n, has_nd = base_lengths(gs.rec_values.cpu().numpy(), gs.rec_dist.cpu().numpy(),
                             gs.rec_part.cpu().numpy().astype(np.int64),
                             cand_lo.cpu().numpy(), cand_hi.cpu().numpy(),
                             ent_ptr.cpu().numpy())
    edges = [0, 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 1 << 40]
    hist, _ = np.histogram(n, bins=edges)
    print(f"records {R}, entities {E}, candidates {int(n.sum())}, "
          f"median list {int(np.median(n))}, longest {int(n.max())}")
    for lo, hi, c in zip(edges[:-1], edges[1:], hist):
        print(f"  base list in [{lo}, {hi if hi < 1 << 40 else 'inf'}): {c} records")
    for s in (128, 256, 512):
        tail = n > s
        print(f"  above {s}: {int(tail.sum())} records "
              f"({int((tail & ~has_nd).sum())} scan their partition), "
              f"{int(n[tail].sum())} candidates "
              f"({100.0 * n[tail].sum() / n.sum():.1f} %)")

    out = torch.empty(R, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ctrl = torch.empty(0, dtype=torch.int64, device=dev)

    def timed(mask):
        def call():
            C.link_update(gs.rec_values, gs.rec_dist, gs.rec_gid, gs.rec_part, cand_lo,
                          cand_hi, postings, gs.ent_values, ent_ptr, m.log_norm, m.voff,
                          m.csr_row_ptr, m.csr_col, m.csr_sim, m.attr_const, args.seed,
                          7, out, gs.rec_ent, err, mask, ctrl, eng._pair_a1, eng._pair_a2)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / args.reps

    def timed_split(split_len):
        """The same launch with the split path taking lists above split_len."""
        lst = torch.empty(R, dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)

        def call():
            cnt.zero_()
            C.link_update_split(gs.rec_values, gs.rec_dist, gs.rec_gid, gs.rec_part,
                                cand_lo, cand_hi, postings, gs.ent_values, ent_ptr,
                                m.log_norm, m.voff, m.csr_row_ptr, m.csr_col, m.csr_sim,
                                m.attr_const, args.seed, 7, out, gs.rec_ent, err, zeros,
                                ctrl, eng._pair_a1, eng._pair_a2, lst, cnt, split_len, 256)
        for _ in range(20):
            call()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(args.reps):
            call()
        t1.record()
        torch.cuda.synchronize()
        return 1000.0 * t0.elapsed_time(t1) / args.reps

    zeros = torch.zeros(R, dtype=torch.uint8, device=dev)
    no_tail = torch.from_numpy(np.where(n > args.split, 2, 0).astype(np.uint8)).to(dev)
    t_cut, t_all = timed(no_tail), timed(zeros)  # `out` ends as the full result
    print(f"link_update, {args.reps} back-to-back launches (mode_mask present, so "
          f"each is the wave kernel plus an idle thread kernel):")
    print(f"  all records: {t_all:.1f} us   without lists above {args.split}: "
          f"{t_cut:.1f} us   tail: {t_all - t_cut:.1f} us")
    if hasattr(C, "link_update_split"):
        ref = out.clone()
        for s in (128, 256, 512):
            t = timed_split(s)
            print(f"  split path above {s} (plus the counter's fill): {t:.1f} us, "
                  f"draws equal: {bool(torch.equal(out, ref))}")


if __name__ == "__main__":
    main()
