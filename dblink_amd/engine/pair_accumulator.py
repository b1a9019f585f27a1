"""Pairwise co-clustering counts accumulated while the chain is sampled.

``OnlinePairCounts`` is handed to ``sampler.sample``; every recorded sample
is counted through the engine (``engine.accumulate_pairs``): the GPU engine
feeds the resident links to the device ``PairCountTable``, the CPU engine
runs the numpy arm and hands the sample's ``(keys, counts)`` over. Keys are
``(a << 32) | b`` over record gids, a < b, in both arms; ``finish`` maps
them to the ranks of the record ids in string order, the same contract as
``chain.pairwise_link_counts`` over the saved chain, without reading it.
"""

from __future__ import annotations

import os
import re

import numpy as np

from ..analysis import chain as chain_q
from ..parallel import comm

_FILE_RE = re.compile(r"^pair-counts-rank(\d+)\.npz$")


def counts_file(output_path, rank):
    return os.path.join(output_path, f"pair-counts-rank{rank}.npz")


def _saved_files(output_path):
    """{rank index -> path} of the pair-count files in ``output_path``."""
    if not os.path.isdir(output_path):
        return {}
    out = {}
    for name in os.listdir(output_path):
        m = _FILE_RE.match(name)
        if m:
            out[int(m.group(1))] = os.path.join(output_path, name)
    return out


class OnlinePairCounts:
    """Running pair counts of this rank's clusters.

    ``S`` is the number of samples counted, ``iteration`` the chain iteration
    of the last one (None before the first). Host-side counts are merged
    every ``merge_every`` samples, so the pending list stays short."""

    def __init__(self, merge_every=16, initial_capacity=None):
        if merge_every < 1:
            raise ValueError("merge_every must be positive")
        self.merge_every = int(merge_every)
        self.S = 0
        self.iteration = None
        self._table = None
        self._table_kw = ({} if initial_capacity is None
                          else {"initial_capacity": int(initial_capacity)})
        self._keys = np.empty(0, np.int64)
        self._counts = np.empty(0, np.int64)
        self._pending = []

    # ---- feeding -------------------------------------------------------------

    def add_sample(self, engine, state):
        engine.accumulate_pairs(state, self)
        self.S += 1
        self.iteration = int(state.iteration)

    def device_table(self, device):
        """The device table of the GPU arm (created on first use; counts
        loaded from a file before that move into it)."""
        if self._table is None:
            from ..ops import PairCountTable

            self._table = PairCountTable(device=device, **self._table_kw)
            self._merge_pending()
            if len(self._keys):
                self._table.load(self._keys, self._counts)
                self._keys = np.empty(0, np.int64)
                self._counts = np.empty(0, np.int64)
        return self._table

    def add_host(self, keys, counts):
        """One sample's distinct keys and counts from the numpy arm."""
        self._pending.append((np.asarray(keys, np.int64), np.asarray(counts, np.int64)))
        if len(self._pending) >= self.merge_every:
            self._merge_pending()

    def _merge_pending(self):
        if self._pending:
            ks = [self._keys] + [k for k, _ in self._pending]
            cs = [self._counts] + [c for _, c in self._pending]
            self._keys, self._counts = chain_q._merge_key_counts(
                np.concatenate(ks), np.concatenate(cs))
            self._pending = []

    def local_counts(self):
        """This rank's sorted distinct keys (gid space) and int64 counts."""
        self._merge_pending()
        if self._table is None:
            return self._keys, self._counts
        keys, counts = self._table.finish()
        keys, counts = keys.cpu().numpy(), counts.cpu().numpy()
        if len(self._keys) == 0:
            return keys, counts
        return chain_q._merge_key_counts(np.concatenate([self._keys, keys]),
                                         np.concatenate([self._counts, counts]))

    # ---- result --------------------------------------------------------------

    def finish(self, engine):
        """``(uniq_ids, a, b, count, S)`` as ``chain.pairwise_link_counts``
        returns it. Collective: every rank calls it; ranks other than 0 get
        None (a pair may have been counted on different ranks in different
        iterations, so rank 0 merges all of them)."""
        local = self.local_counts()
        if comm.is_distributed():
            gathered = comm.all_gather_object(local)
            if comm.rank_world()[0] != 0:
                return None
            keys, counts = chain_q._merge_key_counts(
                np.concatenate([k for k, _ in gathered]),
                np.concatenate([c for _, c in gathered]))
        else:
            keys, counts = local
        ids = getattr(engine, "rec_ids_array", None)
        if ids is None:
            raise ValueError("online pair counts need engine.rec_ids_array "
                             "(record id of every gid) to name the pairs")
        n = len(ids)
        chain_q._check_id_count(n)
        # gid -> rank among the ids in Python string order (the canonical
        # order of chain._chain_rank_codes)
        order = sorted(range(n), key=ids.__getitem__)
        rank = np.empty(n, dtype=np.int64)
        rank[order] = np.arange(n, dtype=np.int64)
        uniq_ids = np.empty(n, dtype=object)
        uniq_ids[:] = [ids[i] for i in order]
        x = rank[keys >> np.int64(32)]
        y = rank[keys & np.int64(0xFFFFFFFF)]
        packed = (np.minimum(x, y) << np.int64(32)) | np.maximum(x, y)
        o = np.argsort(packed, kind="stable")
        packed = packed[o]
        return (uniq_ids, packed >> np.int64(32), packed & np.int64(0xFFFFFFFF),
                counts[o].astype(np.int64), self.S)

    # ---- persistence ---------------------------------------------------------

    def save(self, output_path, rank, iteration, world_size=None):
        """Write this rank's counts next to the saved state of ``iteration``."""
        keys, counts = self.local_counts()
        os.makedirs(output_path, exist_ok=True)
        last = -1 if self.iteration is None else self.iteration
        np.savez(counts_file(output_path, rank), keys=keys, counts=counts,
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
        ahead of the state."""
        if self.S or self._table is not None or self._pending:
            raise ValueError("load() needs an empty accumulator")
        files = _saved_files(output_path)
        if not files:
            raise ValueError(
                f"the chain in {output_path} continues from iteration "
                f"{state_iteration}, but {counts_file(output_path, rank)} is "
                "missing: the samples already in the chain were not counted")
        S = last = None
        ks, cs = [], []
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
                    ks.append(z["keys"].astype(np.int64))
                    cs.append(z["counts"].astype(np.int64))
        if ks:
            self._keys, self._counts = chain_q._merge_key_counts(
                np.concatenate(ks), np.concatenate(cs))
        self.S = S
        self.iteration = last if last >= 0 else None
