"""Growable device cluster-count hash table (holder for the cluster kernels
of ``pair_counts.hip``).

Counts, per distinct cluster (set of record gids), the samples that contain
it, for the most probable clusters. Open addressing with linear probing over
a power-of-two capacity, as ``PairCountTable``; a slot holds the cluster's
64-bit content key (``chain.cluster_keys_numpy`` computes the same integers),
its count, the iteration it was first seen in, its size and the start of its
member list in one shared member arena.

Before every add the table is grown so that the load factor stays <= 0.5
(one sample brings at most min(E, R) new clusters) and the arena so that it
can take R more members (a record lies in one cluster of a sample). The
kernels' error flag is read after every add; flags 1, 2 and 8 are bugs and
raise, flag 4 is a bad link: that sample is not counted.

Memory: the arena keeps one copy of every distinct cluster ever seen. That
is at most S * R * 4 bytes after S samples of R records, reached only when
no cluster ever recurs; on a mixing chain most clusters of a sample have
been seen before and the arena grows far slower. There is no cap or spill:
every doubling of the table or the arena is logged with the new ``nbytes``.
"""

from __future__ import annotations

import logging

from .pair_table import EMPTY, _pow2_at_least

log = logging.getLogger("dblink_amd.ops")


class ClusterCountTable:
    """Counts the distinct clusters of the samples fed to it.

    Public state: ``keys`` (int64, ``EMPTY`` = free), ``counts``, ``first``,
    ``size`` (int32), ``off`` (int64), ``members`` (int32 arena),
    ``capacity``, ``arena_capacity``, ``occupied``, ``arena_used`` and ``err``
    (host ints, refreshed by every add), ``grow_count`` (table rehashes and
    arena copies so far).
    """

    def __init__(self, initial_capacity=1 << 16, initial_arena=1 << 18, device="cuda"):
        import torch

        from . import native

        self._C = native()
        if not hasattr(self._C, "cluster_table_add"):
            raise RuntimeError("the native extension lacks the cluster-count kernels")
        cap = int(initial_capacity)
        if cap < 2 or cap & (cap - 1):
            raise ValueError("initial_capacity must be a power of two >= 2")
        if int(initial_arena) < 1:
            raise ValueError("initial_arena must be positive")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("ClusterCountTable lives on a GPU device")
        self.keys, self.counts, self.first, self.size, self.off = self._alloc(cap)
        self.members = torch.empty(int(initial_arena), dtype=torch.int32,
                                   device=self.device)
        self._ctr = torch.zeros(2, dtype=torch.int64, device=self.device)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.occupied = 0
        self.arena_used = 0
        self.err = 0
        self.grow_count = 0
        self._l_cnt = self._l_ptr = self._l_codes = None  # add_links scratch

    def _alloc(self, cap):
        import torch

        kw = {"device": self.device}
        return (torch.full((cap,), EMPTY, dtype=torch.int64, **kw),
                torch.zeros(cap, dtype=torch.int32, **kw),
                torch.zeros(cap, dtype=torch.int32, **kw),
                torch.zeros(cap, dtype=torch.int32, **kw),
                torch.zeros(cap, dtype=torch.int64, **kw))

    @property
    def capacity(self):
        return self.keys.numel()

    @property
    def arena_capacity(self):
        return self.members.numel()

    @property
    def nbytes(self):
        return self.capacity * (8 + 4 + 4 + 4 + 8) + self.arena_capacity * 4

    def _check_err(self, what):
        self.err = int(self._err.item())
        if self.err & 4:
            # bad input, not a broken table: nothing was added, and the
            # table stays usable
            self._err.zero_()
            raise RuntimeError(
                f"cluster-count table: {what} raised error flag {self.err} "
                "(4 = a rec_ent outside [0, num_entities) or a rec_gid outside "
                "[0, 2^31)): the sample was not counted")
        if self.err:
            raise RuntimeError(
                f"cluster-count table: {what} raised error flag {self.err} "
                "(1 = no free slot, 2 = inconsistent offsets, 8 = arena "
                "overflow): this is a bug")

    def _read_counters(self):
        self.occupied, self.arena_used = (int(v) for v in self._ctr.tolist())

    def _grow_table(self, cap):
        new = self._alloc(cap)
        self._C.cluster_table_rehash(self.keys, self.counts, self.first, self.size,
                                     self.off, *new, self._err)
        self.keys, self.counts, self.first, self.size, self.off = new
        self.grow_count += 1
        self._check_err("rehash")
        log.info("cluster-count table grown to %d slots (%d bytes with the arena)",
                 cap, self.nbytes)

    def _grow_arena(self, n):
        import torch

        members = torch.empty(n, dtype=torch.int32, device=self.device)
        members[:self.arena_used] = self.members[:self.arena_used]
        self.members = members
        self.grow_count += 1
        log.info("cluster-count arena grown to %d members (%d bytes with the table)",
                 n, self.nbytes)

    def add(self, codes, ent_ptr, iteration):
        """Count the clusters ``codes[ent_ptr[e]:ent_ptr[e + 1]]`` of one
        sample taken at chain iteration ``iteration``; empty ranges are no
        clusters. ``codes`` is int32 and ``ent_ptr`` int64, both on the
        table's device. Iterations must not decrease from add to add, so
        that ``first`` is the first."""
        R, E = int(codes.numel()), int(ent_ptr.numel()) - 1
        if R == 0 or E <= 0:
            return
        new = min(E, R)
        if 2 * (self.occupied + new) > self.capacity:
            self._grow_table(_pow2_at_least(2 * (self.occupied + new)))
        if self.arena_used + R > self.arena_capacity:
            self._grow_arena(_pow2_at_least(self.arena_used + R))
        self._C.cluster_table_add(codes, ent_ptr, int(iteration), self.keys,
                                  self.counts, self.first, self.size, self.off,
                                  self.members, self._ctr, self._err)
        self._check_err("add")
        self._read_counters()

    def _links_scratch(self, E, R):
        """Buffers of ``add_links``, regrown only when E or R outgrows them."""
        import torch

        if self._l_cnt is None or self._l_cnt.numel() < E:
            self._l_cnt = torch.empty(E, dtype=torch.int32, device=self.device)
            self._l_ptr = torch.empty(E + 1, dtype=torch.int64, device=self.device)
        if self._l_codes is None or self._l_codes.numel() < R:
            self._l_codes = torch.empty(R, dtype=torch.int32, device=self.device)
        return self._l_cnt[:E], self._l_ptr[:E + 1], self._l_codes[:R]

    def add_links(self, rec_ent, rec_gid, num_entities, iteration):
        """Count one sample given as links: record r, with the gid
        ``rec_gid[r]``, sits in the cluster of entity ``rec_ent[r]``.

        Both are int64 vectors on the table's device, in any record order;
        ``rec_ent`` lies in ``[0, num_entities)`` and ``rec_gid`` in
        ``[0, 2^31)``. A value outside raises RuntimeError (flag 4) and the
        sample is not counted: the add kernel leaves a launch alone that
        finds the flag set, so the flag is read once, after both."""
        R, E = int(rec_ent.numel()), int(num_entities)
        if R == 0 or E == 0:
            return
        cnt, ptr, codes = self._links_scratch(E, R)
        self._C.pair_links_csr(rec_ent, rec_gid, cnt, ptr, codes, self._err)
        self.add(codes, ptr, iteration)

    def finish(self):
        """``(keys, counts, first, offsets, members)`` of the occupied slots
        as device tensors, sorted by key: int64 except ``members`` (int32);
        cluster i holds ``members[offsets[i]:offsets[i + 1]]``."""
        import torch

        live = torch.nonzero(self.keys != EMPTY).squeeze(1)
        keys, order = torch.sort(self.keys[live])
        live = live[order]
        sizes = self.size[live].to(torch.int64)
        offsets = torch.zeros(live.numel() + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(sizes, 0, out=offsets[1:])
        idx = torch.arange(int(offsets[-1].item()), dtype=torch.int64,
                           device=self.device)
        idx += torch.repeat_interleave(self.off[live] - offsets[:-1], sizes)
        return (keys, self.counts[live].to(torch.int64),
                self.first[live].to(torch.int64), offsets, self.members[idx])
