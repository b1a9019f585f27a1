// Pair-count hash table (gfx950): co-clustering counts of record pairs over
// the linkage chain, for the posterior pairwise link probabilities. An
// extension; the reference has no counterpart.
//
// Table: open addressing, linear probing, power-of-two capacity. keys holds
// (uint64(a) << 32) | b with rank codes a < b < 2^31, so the all-ones EMPTY
// marker is unreachable; counts is int32. The host grows the table BEFORE an
// add so that the load factor stays <= 0.5: an insert always finds a slot
// and a chunk is never half-applied. Every probe loop is bounded by the
// capacity; a thread that runs out of slots raises the error flag and goes
// on. No loop here waits on another thread's progress.
//
// The second half of the file is the cluster-count table (how often each
// distinct cluster occurs, for the most probable clusters): the same probing
// over content keys, with per-slot metadata and a member arena.

#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "common.h"

namespace dblink {

// kernels.hip
void scan_excl(torch::Tensor counts, torch::Tensor ptr, torch::Tensor cursor,
               bool clear);

namespace {

constexpr unsigned long long PT_EMPTY = ~0ull;
constexpr int PT_THREADS = 256;
constexpr int PT_ITEMS = 8;  // consecutive pair indices per thread
constexpr int64_t PT_TILE = (int64_t)PT_THREADS * PT_ITEMS;
constexpr int PT_ERR_FULL = 1;    // probed every slot without success
constexpr int PT_ERR_BOUNDS = 2;  // pair_ptr and cluster_offsets disagree
constexpr int PT_ERR_LINKS = 4;   // a link's entity or gid is out of range
constexpr int64_t PT_MAX_CODE = (int64_t)1 << 31;  // codes are < 2^31

DBL_D unsigned long long pt_mix(unsigned long long x) {  // splitmix64 finaliser
  x += 0x9E3779B97F4A7C15ull;
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// Adds `add` to the count of `key`, claiming a slot on first sight. Returns
// 1 when this thread claimed the slot, 0 on a match, -1 when all `cap` slots
// were probed in vain. The plain load ahead of the CAS is a shortcut only: a
// key never changes once written, a stale EMPTY just leads to the CAS, and
// the CAS returns the truth.
DBL_D int pt_insert(unsigned long long* __restrict__ keys, int32_t* __restrict__ counts,
                    unsigned long long cap, unsigned long long key, int32_t add) {
  const unsigned long long mask = cap - 1;
  unsigned long long slot = pt_mix(key) & mask;
  for (unsigned long long n = 0; n < cap; ++n, slot = (slot + 1) & mask) {
    unsigned long long cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
    int claimed = 0;
    if (cur == PT_EMPTY) {
      cur = atomicCAS(&keys[slot], PT_EMPTY, key);
      if (cur == PT_EMPTY) {
        cur = key;
        claimed = 1;
      }
    }
    if (cur == key) {
      atomicAdd(&counts[slot], add);
      return claimed;
    }
  }
  return -1;
}

// First index i in [lo, hi) with arr[i] > key.
DBL_D int64_t pt_upper_bound(const int64_t* __restrict__ arr, int64_t lo, int64_t hi,
                             int64_t key) {
  while (lo < hi) {
    int64_t mid = (lo + hi) >> 1;
    if (arr[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

DBL_D int64_t pt_row_start(int64_t j) { return j * (j - 1) / 2; }

// Cluster-local pair index t -> (i, j), i < j, with t = j (j - 1) / 2 + i.
// The fp64 root is a first guess only; the integer fix-up makes it exact
// for every t (an fp32 root is off from t > 2^24).
DBL_D void pt_decode(int64_t t, int64_t* i, int64_t* j) {
  int64_t r = (int64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
  if (r < 1) r = 1;
  while (pt_row_start(r) > t) --r;
  while (pt_row_start(r + 1) <= t) ++r;
  *j = r;
  *i = t - pt_row_start(r);
}

// Work is split by GLOBAL PAIR INDEX: a block takes tiles of PT_TILE
// consecutive pair indices (grid-stride), a thread PT_ITEMS consecutive
// ones. The tile's cluster range comes from one binary search per tile edge
// in pair_ptr; a thread searches only that range, then walks forward.
__global__ void __launch_bounds__(PT_THREADS)
pair_table_add_kernel(const int32_t* __restrict__ codes, int64_t n_codes,
                      const int64_t* __restrict__ offsets,
                      const int64_t* __restrict__ pair_ptr, int64_t C,
                      int64_t total, unsigned long long* __restrict__ keys,
                      int32_t* __restrict__ counts, unsigned long long cap,
                      unsigned long long* __restrict__ occupied,
                      int32_t* __restrict__ err) {
  __shared__ int64_t edge[2];
  const int64_t n_tiles = (total + PT_TILE - 1) / PT_TILE;
  unsigned int claimed = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t t0 = tile * PT_TILE;
    const int64_t t1 = t0 + PT_TILE < total ? t0 + PT_TILE : total;
    __syncthreads();  // the previous tile's readers are done with edge[]
    if (threadIdx.x < 2) {
      const int64_t p = threadIdx.x == 0 ? t0 : t1 - 1;
      const int64_t e = pt_upper_bound(pair_ptr, 0, C + 1, p) - 1;
      edge[threadIdx.x] = e < 0 ? 0 : (e < C ? e : C - 1);
    }
    __syncthreads();
    int64_t p = t0 + (int64_t)threadIdx.x * PT_ITEMS;
    const int64_t p_end = p + PT_ITEMS < t1 ? p + PT_ITEMS : t1;
    if (p >= p_end) continue;
    // the cluster c with pair_ptr[c] <= p < pair_ptr[c + 1]; clusters
    // without pairs have an empty range and are never landed on
    int64_t c = pt_upper_bound(pair_ptr, edge[0], edge[1] + 1, p) - 1;
    if (c < edge[0]) c = edge[0];
    int64_t c_lo = pair_ptr[c], c_hi = pair_ptr[c + 1], base = offsets[c];
    for (; p < p_end; ++p) {
      while (p >= c_hi && c + 1 < C) {
        ++c;
        c_lo = c_hi;
        c_hi = pair_ptr[c + 1];
        base = offsets[c];
      }
      if (p < c_lo || p >= c_hi) {  // pair_ptr does not cover p
        atomicOr(err, PT_ERR_BOUNDS);
        continue;
      }
      int64_t i, j;
      pt_decode(p - c_lo, &i, &j);
      if (base < 0 || base + j >= n_codes) {
        atomicOr(err, PT_ERR_BOUNDS);
        continue;
      }
      const uint32_t x = (uint32_t)codes[base + i], y = (uint32_t)codes[base + j];
      if (x == y) continue;  // a duplicated member is no pair
      const unsigned long long key =
          ((unsigned long long)(x < y ? x : y) << 32) | (unsigned long long)(x < y ? y : x);
      const int r = pt_insert(keys, counts, cap, key, 1);
      if (r < 0) atomicOr(err, PT_ERR_FULL); else claimed += (unsigned)r;
    }
  }
  // one counter update per wave (every lane gets here: the tile loop's
  // bounds are uniform over the block)
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) claimed += __shfl_down(claimed, off);
  if ((threadIdx.x & (WAVE - 1)) == 0 && claimed)
    atomicAdd(occupied, (unsigned long long)claimed);
}

__global__ void __launch_bounds__(PT_THREADS)
pair_table_rehash_kernel(const unsigned long long* __restrict__ old_keys,
                         const int32_t* __restrict__ old_counts, int64_t old_cap,
                         unsigned long long* __restrict__ keys,
                         int32_t* __restrict__ counts, unsigned long long cap,
                         int32_t* __restrict__ err) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < old_cap;
       s += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = old_keys[s];
    if (key == PT_EMPTY) continue;
    if (pt_insert(keys, counts, cap, key, old_counts[s]) < 0)
      atomicOr(err, PT_ERR_FULL);
  }
}

// ---------------------------------------------------------------------------
// Links -> member lists. A sample held as a link vector (record r belongs to
// entity rec_ent[r] and has the global id rec_gid[r]) becomes the
// (codes, offsets) form pair_table_add_kernel consumes: a counting sort of
// the gids by entity, as count / scan / scatter. The scan is scan_excl
// (kernels.hip). An entity without records, or with one, has an empty pair
// range, so the offsets keep one cluster per entity.
// ---------------------------------------------------------------------------

// A record is counted only when its entity indexes ent_cnt and its gid fits
// the 31 bits of a pair key; both kernels apply this test, before any access
// that depends on e or gid, and skip the same records.
DBL_D bool pl_valid(int64_t e, int64_t gid, int64_t E) {
  return e >= 0 && e < E && gid >= 0 && gid < PT_MAX_CODE;
}

__global__ void __launch_bounds__(PT_THREADS)
pair_links_count_kernel(const int64_t* __restrict__ rec_ent,
                        const int64_t* __restrict__ rec_gid, int64_t R, int64_t E,
                        int32_t* __restrict__ ent_cnt,  // [E], zeroed
                        int32_t* __restrict__ err) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = rec_ent[r];
    if (!pl_valid(e, rec_gid[r], E)) {
      atomicOr(err, PT_ERR_LINKS);
      continue;
    }
    atomicAdd(&ent_cnt[e], 1);
  }
}

// cursor [E] is zero on entry (scan_excl cleared the counters it scanned).
// The slot within the entity's range is whatever the atomic hands out: the
// member order is arbitrary, which the pair counts do not depend on.
__global__ void __launch_bounds__(PT_THREADS)
pair_links_scatter_kernel(const int64_t* __restrict__ rec_ent,
                          const int64_t* __restrict__ rec_gid, int64_t R, int64_t E,
                          const int64_t* __restrict__ ent_ptr,  // [E + 1]
                          int32_t* __restrict__ cursor,
                          int32_t* __restrict__ codes, int64_t n_codes,
                          int32_t* __restrict__ err) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t e = rec_ent[r];
    const int64_t gid = rec_gid[r];
    if (!pl_valid(e, gid, E)) continue;  // flagged by the count pass
    const int64_t lo = ent_ptr[e], hi = ent_ptr[e + 1];
    const int64_t pos = atomicAdd(&cursor[e], 1);
    if (pos < 0 || pos >= hi - lo || lo < 0 || lo + pos >= n_codes) {
      atomicOr(err, PT_ERR_BOUNDS);  // links changed between the two passes
      continue;
    }
    codes[lo + pos] = (int32_t)gid;
  }
}

void check_table(const torch::Tensor& keys, const torch::Tensor& counts,
                 const char* what) {
  TORCH_CHECK(keys.is_cuda() && counts.is_cuda(), what, ": table must be on the GPU");
  TORCH_CHECK(keys.is_contiguous() && counts.is_contiguous(), what,
              ": table must be contiguous");
  TORCH_CHECK(keys.scalar_type() == torch::kInt64 &&
              counts.scalar_type() == torch::kInt32, what,
              ": keys int64, counts int32");
  const int64_t cap = keys.numel();
  TORCH_CHECK(cap >= 2 && (cap & (cap - 1)) == 0, what,
              ": capacity must be a power of two");
  TORCH_CHECK(counts.numel() == cap, what, ": counts must match keys");
}

unsigned grid_for(int64_t work_items) {
  const int64_t cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(work_items, cus * 8));
}

}  // namespace

// Counts every member pair of the chunk's clusters into the table.
// cluster_offsets [C + 1] delimits the clusters in codes; pair_ptr [C + 1]
// is the exclusive int64 scan of s (s - 1) / 2 with the total last.
// total_pairs < 0 reads that total back from the device.
void pair_table_add(torch::Tensor codes, torch::Tensor cluster_offsets,
                    torch::Tensor pair_ptr, torch::Tensor keys,
                    torch::Tensor counts, torch::Tensor occupied,
                    torch::Tensor err, int64_t total_pairs) {
  check_table(keys, counts, "pair_table_add");
  TORCH_CHECK(codes.is_cuda() && cluster_offsets.is_cuda() && pair_ptr.is_cuda() &&
              occupied.is_cuda() && err.is_cuda(),
              "pair_table_add: all tensors must be on the GPU");
  TORCH_CHECK(codes.is_contiguous() && cluster_offsets.is_contiguous() &&
              pair_ptr.is_contiguous(), "pair_table_add: inputs must be contiguous");
  TORCH_CHECK(codes.scalar_type() == torch::kInt32 &&
              cluster_offsets.scalar_type() == torch::kInt64 &&
              pair_ptr.scalar_type() == torch::kInt64,
              "pair_table_add: codes int32, cluster_offsets and pair_ptr int64");
  TORCH_CHECK(occupied.scalar_type() == torch::kInt64 && occupied.numel() == 1 &&
              err.scalar_type() == torch::kInt32 && err.numel() == 1,
              "pair_table_add: occupied int64 [1], err int32 [1]");
  const int64_t C = cluster_offsets.numel() - 1;
  TORCH_CHECK(C >= 0 && pair_ptr.numel() == C + 1,
              "pair_table_add: pair_ptr must hold one entry per offset");
  if (C == 0) return;
  const int64_t total =
      total_pairs >= 0 ? total_pairs : pair_ptr[C].item<int64_t>();
  if (total == 0) return;
  const int64_t n_tiles = (total + PT_TILE - 1) / PT_TILE;
  hipLaunchKernelGGL(
      pair_table_add_kernel, dim3(grid_for(n_tiles)), dim3(PT_THREADS), 0,
      at::cuda::getCurrentCUDAStream(), codes.data_ptr<int32_t>(), codes.numel(),
      cluster_offsets.data_ptr<int64_t>(), pair_ptr.data_ptr<int64_t>(), C, total,
      reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
      counts.data_ptr<int32_t>(), (unsigned long long)keys.numel(),
      reinterpret_cast<unsigned long long*>(occupied.data_ptr<int64_t>()),
      err.data_ptr<int32_t>());
}

// One sample's links -> the member lists pair_table_add takes: codes [R]
// receives the gids grouped by entity (any order inside an entity), ent_ptr
// [E + 1] the offsets. ent_cnt [E] is scratch (zeroed here). A
// record whose entity is outside [0, E) or whose gid is outside [0, 2^31)
// raises PT_ERR_LINKS in err and is left out; ent_ptr[E] then counts the
// records that were taken.
void pair_links_csr(torch::Tensor rec_ent, torch::Tensor rec_gid,
                    torch::Tensor ent_cnt, torch::Tensor ent_ptr,
                    torch::Tensor codes, torch::Tensor err) {
  TORCH_CHECK(rec_ent.is_cuda() && rec_gid.is_cuda() && ent_cnt.is_cuda() &&
              ent_ptr.is_cuda() && codes.is_cuda() && err.is_cuda(),
              "pair_links_csr: all tensors must be on the GPU");
  TORCH_CHECK(rec_ent.is_contiguous() && rec_gid.is_contiguous() &&
              ent_cnt.is_contiguous() && ent_ptr.is_contiguous() &&
              codes.is_contiguous(), "pair_links_csr: tensors must be contiguous");
  TORCH_CHECK(rec_ent.scalar_type() == torch::kInt64 &&
              rec_gid.scalar_type() == torch::kInt64,
              "pair_links_csr: rec_ent and rec_gid int64");
  TORCH_CHECK(ent_cnt.scalar_type() == torch::kInt32 &&
              ent_ptr.scalar_type() == torch::kInt64 &&
              codes.scalar_type() == torch::kInt32,
              "pair_links_csr: ent_cnt and codes int32, ent_ptr int64");
  TORCH_CHECK(err.scalar_type() == torch::kInt32 && err.numel() == 1,
              "pair_links_csr: err int32 [1]");
  const int64_t R = rec_ent.numel(), E = ent_cnt.numel();
  TORCH_CHECK(rec_ent.dim() == 1 && rec_gid.dim() == 1 && rec_gid.numel() == R,
              "pair_links_csr: rec_ent and rec_gid must be vectors of one length");
  TORCH_CHECK(ent_ptr.numel() == E + 1, "pair_links_csr: ent_ptr must hold E + 1 entries");
  TORCH_CHECK(codes.numel() >= R, "pair_links_csr: codes must hold one entry per record");
  TORCH_CHECK(R < ((int64_t)1 << 31), "pair_links_csr: at most 2^31 - 1 records");
  auto stream = at::cuda::getCurrentCUDAStream();
  ent_cnt.zero_();
  if (R == 0 || E == 0) {
    ent_ptr.zero_();
    return;
  }
  const unsigned grid = grid_for((R + PT_THREADS - 1) / PT_THREADS);
  hipLaunchKernelGGL(pair_links_count_kernel, dim3(grid), dim3(PT_THREADS), 0, stream,
                     rec_ent.data_ptr<int64_t>(), rec_gid.data_ptr<int64_t>(), R, E,
                     ent_cnt.data_ptr<int32_t>(), err.data_ptr<int32_t>());
  // offsets, and the counters zeroed again to serve as the scatter's cursor
  scan_excl(ent_cnt, ent_ptr, ent_cnt.narrow(0, 0, 0), true);
  hipLaunchKernelGGL(pair_links_scatter_kernel, dim3(grid), dim3(PT_THREADS), 0, stream,
                     rec_ent.data_ptr<int64_t>(), rec_gid.data_ptr<int64_t>(), R, E,
                     ent_ptr.data_ptr<int64_t>(), ent_cnt.data_ptr<int32_t>(),
                     codes.data_ptr<int32_t>(), codes.numel(), err.data_ptr<int32_t>());
}

// Re-inserts every occupied slot of the old table, with its count, into the
// new (EMPTY-filled, zero-count) one.
void pair_table_rehash(torch::Tensor old_keys, torch::Tensor old_counts,
                       torch::Tensor new_keys, torch::Tensor new_counts,
                       torch::Tensor err) {
  check_table(old_keys, old_counts, "pair_table_rehash (old)");
  check_table(new_keys, new_counts, "pair_table_rehash (new)");
  TORCH_CHECK(err.is_cuda() && err.scalar_type() == torch::kInt32 &&
              err.numel() == 1, "pair_table_rehash: err int32 [1] on the GPU");
  TORCH_CHECK(new_keys.data_ptr() != old_keys.data_ptr(),
              "pair_table_rehash: tables must differ");
  const int64_t old_cap = old_keys.numel();
  hipLaunchKernelGGL(
      pair_table_rehash_kernel, dim3(grid_for((old_cap + PT_THREADS - 1) / PT_THREADS)),
      dim3(PT_THREADS), 0, at::cuda::getCurrentCUDAStream(),
      reinterpret_cast<const unsigned long long*>(old_keys.data_ptr<int64_t>()),
      old_counts.data_ptr<int32_t>(), old_cap,
      reinterpret_cast<unsigned long long*>(new_keys.data_ptr<int64_t>()),
      new_counts.data_ptr<int32_t>(), (unsigned long long)new_keys.numel(),
      err.data_ptr<int32_t>());
}

// ---------------------------------------------------------------------------
// Cluster-count table: how often each distinct cluster (member set) occurs
// over the samples, for the most probable clusters. Same open addressing as
// above, keyed by an order-independent 64-bit content key, with per-slot
// metadata (first iteration, size, start of the member list) and one member
// arena shared by all slots. The host keeps the load <= 0.5 and the arena
// large enough for one whole sample before every add.
//
// Within one sample a record lies in one cluster, so two entities of one
// launch never claim or match the same slot (up to key collisions): the
// claimer's plain stores to first/size/off and the arena are not read in the
// launch that wrote them, only by later launches on the stream.
// ---------------------------------------------------------------------------

namespace {

constexpr int CT_ERR_ARENA = 8;  // the arena cannot take a new cluster's members

// The integers of chain._mpc_keys_numpy over the gids: two splitmix-derived
// hashes per member, each summed mod 2^64, combined with the size. EMPTY is
// remapped so that no cluster looks like a free slot.
DBL_D unsigned long long ct_key(const int32_t* __restrict__ codes, int64_t lo, int64_t hi) {
  unsigned long long s1 = 0, s2 = 0;
  for (int64_t i = lo; i < hi; ++i) {
    const unsigned long long h1 = pt_mix((unsigned long long)(uint32_t)codes[i]);
    unsigned long long h2 = (h1 ^ (h1 >> 29)) * 0xD6E8FEB86659FD93ull;
    h2 ^= h2 >> 32;
    s1 += h1;
    s2 += h2;
  }
  const unsigned long long key =
      (s1 ^ (s2 * 0x9E3779B97F4A7C15ull)) + (unsigned long long)(hi - lo);
  return key == PT_EMPTY ? PT_EMPTY - 1 : key;
}

// The slot of `key`, claimed on first sight (*claimed = 1), or -1 when all
// `cap` slots were probed in vain. Probing as pt_insert.
DBL_D int64_t ct_slot(unsigned long long* __restrict__ keys, unsigned long long cap,
                      unsigned long long key, int* claimed) {
  const unsigned long long mask = cap - 1;
  unsigned long long slot = pt_mix(key) & mask;
  *claimed = 0;
  for (unsigned long long n = 0; n < cap; ++n, slot = (slot + 1) & mask) {
    unsigned long long cur = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
    if (cur == PT_EMPTY) {
      cur = atomicCAS(&keys[slot], PT_EMPTY, key);
      if (cur == PT_EMPTY) {
        *claimed = 1;
        return (int64_t)slot;
      }
    }
    if (cur == key) return (int64_t)slot;
  }
  return -1;
}

// One thread per entity (grid-stride). ctr[0] counts the occupied slots,
// ctr[1] is the arena cursor. A launch that finds err already set (a bad
// link flagged by pair_links_csr) counts nothing.
__global__ void __launch_bounds__(PT_THREADS)
cluster_table_add_kernel(const int32_t* __restrict__ codes, int64_t n_codes,
                         const int64_t* __restrict__ ent_ptr, int64_t E,
                         int32_t iteration, unsigned long long* __restrict__ keys,
                         int32_t* __restrict__ counts, int32_t* __restrict__ first,
                         int32_t* __restrict__ size, int64_t* __restrict__ off,
                         unsigned long long cap, int32_t* __restrict__ members,
                         int64_t arena_cap, unsigned long long* __restrict__ ctr,
                         int32_t* __restrict__ err) {
  __shared__ int skip;
  if (threadIdx.x == 0) skip = __atomic_load_n(err, __ATOMIC_RELAXED) != 0;
  __syncthreads();
  if (skip) return;  // uniform over the block
  unsigned int claimed_n = 0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t lo = ent_ptr[e], hi = ent_ptr[e + 1];
    if (lo == hi) continue;  // an entity without records is no cluster
    if (lo < 0 || hi < lo || hi > n_codes) {
      atomicOr(err, PT_ERR_BOUNDS);
      continue;
    }
    const int64_t n = hi - lo;
    int claimed;
    const int64_t slot = ct_slot(keys, cap, ct_key(codes, lo, hi), &claimed);
    if (slot < 0) {
      atomicOr(err, PT_ERR_FULL);
      continue;
    }
    atomicAdd(&counts[slot], 1);
    if (!claimed) continue;
    ++claimed_n;
    const int64_t o = (int64_t)atomicAdd(&ctr[1], (unsigned long long)n);
    first[slot] = iteration;
    if (o < 0 || o + n > arena_cap) {  // the host sized the arena wrongly
      atomicOr(err, CT_ERR_ARENA);
      size[slot] = 0;
      off[slot] = 0;
      continue;
    }
    size[slot] = (int32_t)n;
    off[slot] = o;
    for (int64_t i = 0; i < n; ++i) members[o + i] = codes[lo + i];
  }
  // one counter update per wave (every lane gets here: no lane leaves the
  // loop early)
#pragma unroll
  for (int s = WAVE / 2; s > 0; s >>= 1) claimed_n += __shfl_down(claimed_n, s);
  if ((threadIdx.x & (WAVE - 1)) == 0 && claimed_n)
    atomicAdd(&ctr[0], (unsigned long long)claimed_n);
}

// Re-inserts the old table's keys and carries count and metadata along; the
// arena stays where it is.
__global__ void __launch_bounds__(PT_THREADS)
cluster_table_rehash_kernel(const unsigned long long* __restrict__ old_keys,
                            const int32_t* __restrict__ old_counts,
                            const int32_t* __restrict__ old_first,
                            const int32_t* __restrict__ old_size,
                            const int64_t* __restrict__ old_off, int64_t old_cap,
                            unsigned long long* __restrict__ keys,
                            int32_t* __restrict__ counts, int32_t* __restrict__ first,
                            int32_t* __restrict__ size, int64_t* __restrict__ off,
                            unsigned long long cap, int32_t* __restrict__ err) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < old_cap;
       s += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long key = old_keys[s];
    if (key == PT_EMPTY) continue;
    int claimed;
    const int64_t slot = ct_slot(keys, cap, key, &claimed);
    if (slot < 0) {
      atomicOr(err, PT_ERR_FULL);
      continue;
    }
    atomicAdd(&counts[slot], old_counts[s]);
    if (claimed) {  // old keys are distinct, so every one claims
      first[slot] = old_first[s];
      size[slot] = old_size[s];
      off[slot] = old_off[s];
    }
  }
}

void check_cluster_table(const torch::Tensor& keys, const torch::Tensor& counts,
                         const torch::Tensor& first, const torch::Tensor& size,
                         const torch::Tensor& off, const char* what) {
  check_table(keys, counts, what);
  const int64_t cap = keys.numel();
  TORCH_CHECK(first.is_cuda() && size.is_cuda() && off.is_cuda(), what,
              ": table must be on the GPU");
  TORCH_CHECK(first.is_contiguous() && size.is_contiguous() && off.is_contiguous(),
              what, ": table must be contiguous");
  TORCH_CHECK(first.scalar_type() == torch::kInt32 &&
              size.scalar_type() == torch::kInt32 &&
              off.scalar_type() == torch::kInt64, what,
              ": first and size int32, off int64");
  TORCH_CHECK(first.numel() == cap && size.numel() == cap && off.numel() == cap,
              what, ": first, size and off must match keys");
}

}  // namespace

// Counts one sample's clusters into the cluster-count table. codes and
// ent_ptr [E + 1] are what pair_links_csr produces: gids grouped by entity.
// ctr is int64 [2]: occupied slots, arena cursor. The caller guarantees
// capacity >= 2 (occupied + min(E, R)) and an arena of cursor + R entries.
void cluster_table_add(torch::Tensor codes, torch::Tensor ent_ptr, int64_t iteration,
                       torch::Tensor keys, torch::Tensor counts, torch::Tensor first,
                       torch::Tensor size, torch::Tensor off, torch::Tensor members,
                       torch::Tensor ctr, torch::Tensor err) {
  check_cluster_table(keys, counts, first, size, off, "cluster_table_add");
  TORCH_CHECK(codes.is_cuda() && ent_ptr.is_cuda() && members.is_cuda() &&
              ctr.is_cuda() && err.is_cuda(),
              "cluster_table_add: all tensors must be on the GPU");
  TORCH_CHECK(codes.is_contiguous() && ent_ptr.is_contiguous() &&
              members.is_contiguous() && ctr.is_contiguous(),
              "cluster_table_add: tensors must be contiguous");
  TORCH_CHECK(codes.scalar_type() == torch::kInt32 &&
              ent_ptr.scalar_type() == torch::kInt64 &&
              members.scalar_type() == torch::kInt32,
              "cluster_table_add: codes and members int32, ent_ptr int64");
  TORCH_CHECK(ctr.scalar_type() == torch::kInt64 && ctr.numel() == 2 &&
              err.scalar_type() == torch::kInt32 && err.numel() == 1,
              "cluster_table_add: ctr int64 [2], err int32 [1]");
  TORCH_CHECK(iteration >= 0 && iteration < PT_MAX_CODE,
              "cluster_table_add: iteration must lie in [0, 2^31)");
  TORCH_CHECK(codes.numel() < PT_MAX_CODE,
              "cluster_table_add: at most 2^31 - 1 records");
  const int64_t E = ent_ptr.numel() - 1;
  TORCH_CHECK(E >= 0, "cluster_table_add: ent_ptr must hold E + 1 entries");
  if (E == 0 || codes.numel() == 0) return;
  hipLaunchKernelGGL(
      cluster_table_add_kernel, dim3(grid_for((E + PT_THREADS - 1) / PT_THREADS)),
      dim3(PT_THREADS), 0, at::cuda::getCurrentCUDAStream(),
      codes.data_ptr<int32_t>(), codes.numel(), ent_ptr.data_ptr<int64_t>(), E,
      (int32_t)iteration,
      reinterpret_cast<unsigned long long*>(keys.data_ptr<int64_t>()),
      counts.data_ptr<int32_t>(), first.data_ptr<int32_t>(),
      size.data_ptr<int32_t>(), off.data_ptr<int64_t>(),
      (unsigned long long)keys.numel(), members.data_ptr<int32_t>(),
      members.numel(),
      reinterpret_cast<unsigned long long*>(ctr.data_ptr<int64_t>()),
      err.data_ptr<int32_t>());
}

// Re-inserts every occupied slot of the old table, with its count and
// metadata, into the new (EMPTY-filled, zero-count) one.
void cluster_table_rehash(torch::Tensor old_keys, torch::Tensor old_counts,
                          torch::Tensor old_first, torch::Tensor old_size,
                          torch::Tensor old_off, torch::Tensor new_keys,
                          torch::Tensor new_counts, torch::Tensor new_first,
                          torch::Tensor new_size, torch::Tensor new_off,
                          torch::Tensor err) {
  check_cluster_table(old_keys, old_counts, old_first, old_size, old_off,
                      "cluster_table_rehash (old)");
  check_cluster_table(new_keys, new_counts, new_first, new_size, new_off,
                      "cluster_table_rehash (new)");
  TORCH_CHECK(err.is_cuda() && err.scalar_type() == torch::kInt32 &&
              err.numel() == 1, "cluster_table_rehash: err int32 [1] on the GPU");
  TORCH_CHECK(new_keys.data_ptr() != old_keys.data_ptr(),
              "cluster_table_rehash: tables must differ");
  const int64_t old_cap = old_keys.numel();
  hipLaunchKernelGGL(
      cluster_table_rehash_kernel,
      dim3(grid_for((old_cap + PT_THREADS - 1) / PT_THREADS)), dim3(PT_THREADS), 0,
      at::cuda::getCurrentCUDAStream(),
      reinterpret_cast<const unsigned long long*>(old_keys.data_ptr<int64_t>()),
      old_counts.data_ptr<int32_t>(), old_first.data_ptr<int32_t>(),
      old_size.data_ptr<int32_t>(), old_off.data_ptr<int64_t>(), old_cap,
      reinterpret_cast<unsigned long long*>(new_keys.data_ptr<int64_t>()),
      new_counts.data_ptr<int32_t>(), new_first.data_ptr<int32_t>(),
      new_size.data_ptr<int32_t>(), new_off.data_ptr<int64_t>(),
      (unsigned long long)new_keys.numel(), err.data_ptr<int32_t>());
}

}  // namespace dblink
