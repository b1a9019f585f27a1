"""Growable device pair-count hash table (holder for ``pair_counts.hip``).

Open addressing with linear probing over a power-of-two capacity. A key is
``(a << 32) | b`` for rank codes ``a < b < 2^31``; the all-ones pattern marks
an empty slot. The table is grown *before* a chunk is added, so the load
factor never passes 0.5, an insert always finds a slot and a chunk is never
half-applied. The kernels' error flag is read after every add; a set flag is
a bug and raises. ``add`` takes clusters as member codes and offsets;
``add_links`` takes one sample as device-resident links (record -> entity,
record -> code) and groups them on the device first.
"""

from __future__ import annotations

EMPTY = -1  # all-ones uint64, as the int64 the tensors hold


def _pow2_at_least(n):
    return 1 << max(1, int(n - 1).bit_length())


class PairCountTable:
    """Counts unordered pairs of int32 codes that share a cluster.

    Public state: ``keys`` (int64, ``EMPTY`` = free), ``counts`` (int32),
    ``capacity``, ``occupied`` and ``err`` (host ints, refreshed by ``add``),
    ``grow_count`` (number of rehashes so far).
    """

    def __init__(self, initial_capacity=1 << 16, device="cuda"):
        import torch

        from . import native

        self._C = native()
        if not hasattr(self._C, "pair_table_add"):
            raise RuntimeError("the native extension lacks the pair-count kernels")
        cap = int(initial_capacity)
        if cap < 2 or cap & (cap - 1):
            raise ValueError("initial_capacity must be a power of two >= 2")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PairCountTable lives on a GPU device")
        self.keys, self.counts = self._alloc(cap)
        self._occupied = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.occupied = 0
        self.err = 0
        self.grow_count = 0
        self._l_cnt = self._l_ptr = self._l_codes = None  # add_links scratch

    def _alloc(self, cap):
        import torch

        keys = torch.full((cap,), EMPTY, dtype=torch.int64, device=self.device)
        counts = torch.zeros(cap, dtype=torch.int32, device=self.device)
        return keys, counts

    @property
    def capacity(self):
        return self.keys.numel()

    @property
    def nbytes(self):
        return self.capacity * (8 + 4)

    def _check_err(self, what):
        self.err = int(self._err.item())
        if self.err & ~3:
            # bad input, not a broken table: nothing was added, and the
            # table stays usable
            self._err.zero_()
            raise RuntimeError(
                f"pair-count table: {what} raised error flag {self.err} "
                "(4 = a rec_ent outside [0, num_entities) or a rec_gid outside "
                "[0, 2^31)): the sample was not counted")
        if self.err:
            raise RuntimeError(
                f"pair-count table: {what} raised error flag {self.err} "
                "(1 = no free slot, 2 = inconsistent offsets): this is a bug")

    def _grow(self, cap):
        keys, counts = self._alloc(cap)
        self._C.pair_table_rehash(self.keys, self.counts, keys, counts, self._err)
        self.keys, self.counts = keys, counts
        self.grow_count += 1
        self._check_err("rehash")

    def add(self, codes, cluster_offsets, total_pairs=None):
        """Count every member pair of the clusters ``codes[off[c]:off[c+1]]``.

        ``codes`` is int32 and ``cluster_offsets`` int64 (starting at 0),
        both on the table's device. ``total_pairs`` (the sum of s(s-1)/2),
        when the caller knows it, saves one device read."""
        import torch

        sizes = cluster_offsets[1:] - cluster_offsets[:-1]
        pair_ptr = torch.zeros(cluster_offsets.numel(), dtype=torch.int64,
                               device=self.device)
        torch.cumsum(sizes * (sizes - 1) // 2, 0, out=pair_ptr[1:])
        P = int(pair_ptr[-1].item()) if total_pairs is None else int(total_pairs)
        self.occupied = int(self._occupied.item())
        if 2 * (self.occupied + P) > self.capacity:
            self._grow(_pow2_at_least(2 * (self.occupied + P)))
        self._C.pair_table_add(codes, cluster_offsets, pair_ptr, self.keys,
                               self.counts, self._occupied, self._err, P)
        self._check_err("add")
        self.occupied = int(self._occupied.item())

    def _links_scratch(self, E, R):
        """Buffers of ``add_links``, regrown only when E or R outgrows them."""
        import torch

        if self._l_cnt is None or self._l_cnt.numel() < E:
            self._l_cnt = torch.empty(E, dtype=torch.int32, device=self.device)
            self._l_ptr = torch.empty(E + 1, dtype=torch.int64, device=self.device)
        if self._l_codes is None or self._l_codes.numel() < R:
            self._l_codes = torch.empty(R, dtype=torch.int32, device=self.device)
        return self._l_cnt[:E], self._l_ptr[:E + 1], self._l_codes[:R]

    def add_links(self, rec_ent, rec_gid, num_entities):
        """Count one sample given as links: record r sits in the cluster of
        entity ``rec_ent[r]`` and is counted under the code ``rec_gid[r]``.

        Both are int64 vectors on the table's device, in any record order;
        ``rec_ent`` lies in ``[0, num_entities)`` and ``rec_gid`` in
        ``[0, 2^31)``. A value outside raises RuntimeError (flag 4) and the
        sample is not counted."""
        R, E = int(rec_ent.numel()), int(num_entities)
        if R == 0 or E == 0:
            return
        cnt, ptr, codes = self._links_scratch(E, R)
        self._C.pair_links_csr(rec_ent, rec_gid, cnt, ptr, codes, self._err)
        self._check_err("add_links")
        # entities with fewer than two records have an empty pair range
        self.add(codes, ptr)

    def load(self, keys, counts):
        """Add saved ``(keys, counts)``, as ``finish()`` returns them (int64,
        host or device), into the table: the rehash kernel re-inserts them."""
        import torch

        keys = torch.as_tensor(keys, dtype=torch.int64).to(self.device).reshape(-1)
        counts = torch.as_tensor(counts, dtype=torch.int64).to(self.device).reshape(-1)
        n = keys.numel()
        if counts.numel() != n:
            raise ValueError("keys and counts must have one length")
        if n == 0:
            return
        if bool((keys < 0).any()) or bool((counts < 0).any()) or \
                int(counts.max()) >= 2**31:
            raise ValueError("keys must be pair keys and counts fit int32")
        cap = _pow2_at_least(n)
        src_keys, src_counts = self._alloc(cap)
        src_keys[:n] = keys
        src_counts[:n] = counts.to(torch.int32)
        self.occupied = int(self._occupied.item())
        if 2 * (self.occupied + n) > self.capacity:
            self._grow(_pow2_at_least(2 * (self.occupied + n)))
        self._C.pair_table_rehash(src_keys, src_counts, self.keys, self.counts,
                                  self._err)
        self._check_err("load")
        # the rehash kernel does not keep the slot counter
        self._occupied.copy_((self.keys != EMPTY).sum().reshape(1))
        self.occupied = int(self._occupied.item())

    def finish(self):
        """(sorted keys, counts), both int64, of the occupied slots."""
        import torch

        live = self.keys != EMPTY
        keys, order = torch.sort(self.keys[live])
        return keys, self.counts[live][order].to(torch.int64)
