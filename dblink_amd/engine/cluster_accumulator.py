"""Cluster frequencies accumulated while the chain is sampled, for the
shared most probable clusters (sMPC).

``OnlineClusterCounts`` is handed to ``sampler.sample``; every recorded
sample is counted through the engine (``engine.accumulate_clusters``): the
GPU engine feeds the resident links to the device ``ClusterCountTable``, the
CPU engine runs the numpy arm and hands the sample's clusters over. Both
arms identify a cluster by the same 64-bit content key over its record gids
(``chain.cluster_keys_numpy``). ``finish`` resolves the most probable
cluster of every record on rank 0 with the tie rule of
``chain.most_probable_clusters`` over the saved chain in iteration order,
without reading a chain.

Memory: one copy of every distinct cluster ever seen is kept (on the device
in the GPU arm): at most S * R * 4 bytes of members after S samples of R
records, far less on a chain whose clusters recur.
"""

from __future__ import annotations

import os
import re

import numpy as np

from ..analysis import chain as chain_q
from ..parallel import comm

_FILE_RE = re.compile(r"^cluster-counts-rank(\d+)\.npz$")
_FIELDS = ("keys", "counts", "first", "offsets", "members")


def counts_file(output_path, rank):
    return os.path.join(output_path, f"cluster-counts-rank{rank}.npz")


def _saved_files(output_path):
    """{rank index -> path} of the cluster-count files in ``output_path``."""
    if not os.path.isdir(output_path):
        return {}
    out = {}
    for name in os.listdir(output_path):
        m = _FILE_RE.match(name)
        if m:
            out[int(m.group(1))] = os.path.join(output_path, name)
    return out


class OnlineClusterCounts:
    """Running cluster counts of this rank's clusters.

    ``S`` is the number of samples counted, ``iteration`` the chain iteration
    of the last one (None before the first). Host-side samples are merged
    every ``merge_every`` samples, so the pending list stays short."""

    def __init__(self, merge_every=16, initial_capacity=None, initial_arena=None):
        if merge_every < 1:
            raise ValueError("merge_every must be positive")
        self.merge_every = int(merge_every)
        self.S = 0
        self.iteration = None
        self._table = None
        self._table_kw = {}
        if initial_capacity is not None:
            self._table_kw["initial_capacity"] = int(initial_capacity)
        if initial_arena is not None:
            self._table_kw["initial_arena"] = int(initial_arena)
        self._host = chain_q._empty_cluster_counts()
        self._pending = []

    # ---- feeding -------------------------------------------------------------

    def add_sample(self, engine, state):
        engine.accumulate_clusters(state, self)
        self.S += 1
        self.iteration = int(state.iteration)

    def device_table(self, device):
        """The device table of the GPU arm (created on first use). Counts
        loaded from a file stay on the host and are merged in
        ``local_counts``."""
        if self._table is None:
            from ..ops import ClusterCountTable

            self._table = ClusterCountTable(device=device, **self._table_kw)
        return self._table

    def add_host(self, gids, cluster_offsets, iteration):
        """One sample's clusters ``gids[off[c]:off[c + 1]]`` from the numpy arm."""
        self._pending.append(
            chain_q.cluster_counts_of_sample(gids, cluster_offsets, iteration))
        if len(self._pending) >= self.merge_every:
            self._merge_pending()

    def _merge_pending(self):
        if self._pending:
            self._host = chain_q.merge_cluster_counts([self._host] + self._pending)
            self._pending = []

    def local_counts(self):
        """This rank's ``(keys, counts, first, offsets, members)`` over gids,
        sorted by key."""
        self._merge_pending()
        if self._table is None:
            return self._host
        dev = tuple(t.cpu().numpy() for t in self._table.finish())
        if len(self._host[0]) == 0:
            return dev
        return chain_q.merge_cluster_counts([self._host, dev])

    # ---- result --------------------------------------------------------------

    def finish(self, engine):
        """``(clusters, (gids, best_key, best_count, best_freq), S)``: the
        sMPC clusters as sets of record ids, the per-record most probable
        cluster arrays of ``chain.mpc_from_cluster_counts``, and the number
        of samples. Collective: every rank calls it; ranks other than 0 get
        None (a cluster may have been counted on different ranks in
        different iterations, so rank 0 merges all of them)."""
        local = self.local_counts()
        if comm.is_distributed():
            gathered = comm.all_gather_object(local)
            if comm.rank_world()[0] != 0:
                return None
            merged = chain_q.merge_cluster_counts(gathered)
        else:
            merged = local
        ids = getattr(engine, "rec_ids_array", None)
        if ids is None:
            raise ValueError("online cluster counts need engine.rec_ids_array "
                             "(record id of every gid) to name the records")
        clusters = chain_q.smpc_from_cluster_counts(*merged, self.S, ids=ids)
        return clusters, chain_q.mpc_from_cluster_counts(*merged, self.S), self.S

    # ---- persistence ---------------------------------------------------------

    def save(self, output_path, rank, iteration, world_size=None):
        """Write this rank's counts next to the saved state of ``iteration``."""
        local = self.local_counts()
        os.makedirs(output_path, exist_ok=True)
        last = -1 if self.iteration is None else self.iteration
        np.savez(counts_file(output_path, rank), **dict(zip(_FIELDS, local)),
                 S=np.int64(self.S), iteration=np.int64(last),
                 state_iteration=np.int64(iteration))
        if rank == 0 and world_size is not None:
            # files of an earlier, wider run must not leak into a resume
            for r, path in _saved_files(output_path).items():
                if r >= world_size:
                    os.remove(path)

    def load(self, output_path, rank, world_size, state_iteration):
        """Pick up the counts saved with a chain that now continues from
        ``state_iteration``: rank r takes every file whose index is r modulo
        the world size. Raises ValueError when the files are missing or
        do not belong to the state."""
        if self.S or self._table is not None or self._pending:
            raise ValueError("load() needs an empty accumulator")
        files = _saved_files(output_path)
        if not files:
            raise ValueError(
                f"the chain in {output_path} continues from iteration "
                f"{state_iteration}, but {counts_file(output_path, rank)} is "
                "missing: the samples already in the chain were not counted")
        S = last = None
        parts = []
        for r in sorted(files):
            with np.load(files[r]) as z:
                f_S, f_last = int(z["S"]), int(z["iteration"])
                f_state = int(z["state_iteration"])
                if f_last > state_iteration or f_state != state_iteration:
                    raise ValueError(
                        f"{files[r]} counts samples up to iteration {f_last} and "
                        f"was saved with the state of iteration {f_state}, but "
                        f"the chain continues from iteration {state_iteration}: "
                        "the counts do not belong to this state")
                if S is not None and (f_S, f_last) != (S, last):
                    raise ValueError(
                        f"{files[r]} holds {f_S} samples up to iteration {f_last}, "
                        f"other ranks' files {S} up to {last}")
                S, last = f_S, f_last
                if r % world_size == rank:
                    parts.append(tuple(z[f] for f in _FIELDS))
        self._host = chain_q.merge_cluster_counts(parts)
        self.S = S
        self.iteration = last if last >= 0 else None
