// CDNA4 (gfx950) HIP kernels for the partitioned Gibbs sweep.
//
// Kernel inventory (K-numbers as in STATUS.md "§2.2 / §2.4 kernels"):
//   K4+K5  link_update{,_small,_heavy}_kernel — wave / thread / hierarchical
//              A* link draw, one shared candidate-scoring core (link_* below)
//          link_update_split_kernel — a block per wave-path record whose
//              base list is long, served from a device-side list
//          link_update_dense_kernel — PCG-II / Gibbs-Sequential partition scan
//   K6     value_base_draw (k=0), value_update_k1, _kd1, _kd2,
//              value_update_kernel_t<VMODE> (LDS hash / union merge), _seq
//   K7     distortion_update_kernel — Bernoulli resample, loglik fused in
//   K8     summary_loglik / summary_counts / summary_finalize
//   K3     build_keys, postings_hist / _scatter (counting sort), cand_ranges,
//              build_ekeys_stable (+ rocprim radix sort), classify_modes
//   --     mfma_score / scalar_score — matrix-core scoring experiment
//   K9     kd_descent_kernel — flat KD-tree partition reassignment
//   --     scan_excl, csr_count / _scatter / _order, resort_hist / _scatter /
//              _remap — the integer glue of the sweep (index prefix, entity ->
//              records CSR + kobs, KD descent fused with the stable partition
//              re-sort)
//   K1     sim_pairs_kernel — bit-parallel Levenshtein / OSA domain sweep
//          jaro_pairs_kernel — bit-parallel Jaro(-Winkler) domain sweep
//
// Wave kernels give one wave (64 lanes) a record or an (entity, attribute)
// pair, 4 waves per block; thread kernels give one lane an item. All
// categorical draws use Gumbel-max with Philox counter RNG (common.h), so
// results are independent of scheduling order.

#include <ATen/cuda/CUDAContext.h>
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <torch/extension.h>

#include "common.h"
#include "jaro.h"

namespace dblink {

#define CHECK_GPU(x) TORCH_CHECK(x.is_cuda(), #x " must be a GPU tensor")
#define CHECK_CONTIG(x) TORCH_CHECK(x.is_contiguous(), #x " must be contiguous")

constexpr int MAX_ATTRS = 16;
constexpr uint32_t PH_LINK = 1, PH_DIST = 2, PH_VALG = 3, PH_VALM = 4,
                   PH_LINKH = 7, PH_LINKF = 8;

// ---------------------------------------------------------------------------
// Staged similarity rows. A record's od-attribute CSR sim rows are FIXED for
// the whole candidate scan, yet sim_lookup pays a log2(row)-deep
// dependent-load binary search per (candidate, attr). PMC counters
// (profiles/pmc_r02_1M64.txt) show the link kernels latency-bound
// (SQ_WAIT_ANY >> SQ_ACTIVE_INST), so that chain is the bottleneck: staging
// each row once into a per-wave LDS open-addressing hash turns it into ~1
// LDS probe. Sub-table descriptors are nibble-packed per attr (runtime-
// indexed local arrays would spill to scratch): logpk nibble = log2(slots)
// (0 = not staged -> global binary search, 15 = empty row -> sim 0), offpk
// nibble = offset/32. Load factor <= 1/2; rows that don't fit stay global.
// ---------------------------------------------------------------------------
constexpr int SIMH_CAP = 512;  // staged entries per wave (4 KB key+value)

// NT = threads that fill one table together: WAVE (a wave, lane = its lane id)
// or a whole block (lane = threadIdx.x; the caller adds a __syncthreads()
// before the first lookup). Every branch below is uniform across the NT
// threads, so the block form's barrier is reached by all of them.
template <int NT>
__device__ inline void simh_stage(
    int32_t* kh, float* vh, int lane, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const int64_t* __restrict__ voff, const int32_t* __restrict__ rec_values,
    int64_t r, int A, uint32_t od_mask, uint64_t& logpk, uint64_t& offpk) {
  logpk = 0;
  offpk = 0;
  int cursor = 0;
  for (uint32_t m = od_mask; m;) {
    const int a = __ffs(m) - 1;
    m &= m - 1;
    const int64_t row = voff[a] + rec_values[r * A + a];
    const int64_t lo = csr_row_ptr[row];
    const int len = (int)(csr_row_ptr[row + 1] - lo);
    if (len == 0) {
      logpk |= 15ull << (4 * a);
      continue;
    }
    int lg = 5;  // >= 32 slots keeps offsets on /32 nibble boundaries
    while ((1 << lg) < 2 * len) ++lg;
    if (lg > 9 || cursor + (1 << lg) > SIMH_CAP) continue;  // stays global
    const int sz = 1 << lg, base = cursor;
    for (int i = lane; i < sz; i += NT) kh[base + i] = -1;
    // wave-lockstep: the CAS claims below see the -1 fill of this wave
    if (NT > WAVE) __syncthreads();
    for (int i = lane; i < len; i += NT) {
      const int32_t y = csr_col[lo + i];
      int h = (int)(((uint32_t)y * 2654435761u) >> (32 - lg));
      for (;;) {
        const int32_t prev = atomicCAS(&kh[base + h], -1, y);
        if (prev == -1) {
          vh[base + h] = csr_sim[lo + i];
          break;
        }
        h = (h + 1) & (sz - 1);
      }
    }
    logpk |= (uint64_t)lg << (4 * a);
    offpk |= (uint64_t)(base >> 5) << (4 * a);
    cursor += sz;
  }
}

__device__ inline float simh_lookup(const int32_t* kh, const float* vh,
                                    uint64_t logpk, uint64_t offpk, int a,
                                    const int64_t* __restrict__ csr_row_ptr,
                                    const int32_t* __restrict__ csr_col,
                                    const float* __restrict__ csr_sim,
                                    int64_t row, int32_t y) {
  const int lg = (int)((logpk >> (4 * a)) & 15ull);
  if (lg == 15) return 0.0f;  // empty sim row
  if (lg == 0)                // row not staged
    return sim_lookup(csr_row_ptr, csr_col, csr_sim, row, y);
  const int base = (int)(((offpk >> (4 * a)) & 15ull) << 5);
  int h = (int)(((uint32_t)y * 2654435761u) >> (32 - lg));
  const int msk = (1 << lg) - 1;
  for (;;) {
    const int32_t k = kh[base + h];
    if (k == y) return vh[base + h];
    if (k == -1) return 0.0f;  // staged table holds the FULL row
    h = (h + 1) & msk;
  }
}

// ---------------------------------------------------------------------------
// Candidate-scoring core shared by the link kernels. The wave, thread and
// heavy paths must draw the SAME entity for a record (routing between them
// is a performance decision), so classification, base selection, the
// equality check and the f32 log-weight each exist once, here.
// ---------------------------------------------------------------------------

// Device-side {seed, iteration} override: graph replays read both from ctrl.
DBL_D void ctrl_override(const int64_t* __restrict__ ctrl, uint64_t& seed,
                         uint32_t& iteration) {
  if (ctrl != nullptr) { seed = (uint64_t)ctrl[0]; iteration = (uint32_t)ctrl[1]; }
}

// Attribute classification as BITMASKS, not arrays: runtime-indexed local
// arrays spill to scratch (measured 208 B/lane = a scratch round-trip per
// membership probe), and so do reference out-parameters here. nd = observed
// non-distorted, od = observed distorted and non-constant (constant od attrs
// scale all weights equally and cancel under normalization).
struct LinkMasks { uint32_t nd, od; };

DBL_D LinkMasks link_classify(const int32_t* __restrict__ rec_values,
                              const uint8_t* __restrict__ rec_dist,
                              const uint8_t* __restrict__ attr_const,
                              int64_t r, int A) {
  uint32_t nd_mask = 0, od_mask = 0;
  for (int a = 0; a < A; ++a) {
    const int32_t x = rec_values[r * A + a];
    if (x < 0) continue;
    if (!rec_dist[r * A + a]) nd_mask |= 1u << a;
    else if (!attr_const[a]) od_mask |= 1u << a;
  }
  return {nd_mask, od_mask};
}

struct LinkBase {
  int64_t lo, n;        // candidate range to enumerate
  uint32_t check_mask;  // nd attrs every candidate must still be checked on
  bool postings;        // range indexes postings[]; else it is entity ids
};

// base = smallest candidate list among nd attrs and (optional) const-pair
// pseudo slots; a pair base implies both constituents match, but every nd
// single must still be value-checked (check_mask keeps them all). Without
// any nd attr the base is the record's whole partition.
//
// range(t) gives slot t's candidate range of record r: the stored cand_lo/hi
// for the link kernels, the key prefix itself where the ranges are being
// written in the same launch.
struct CandRange { int64_t lo, hi; };

template <class Range>
DBL_D LinkBase link_select_base_from(const Range& range,
                                     const int32_t* __restrict__ pair_a1,
                                     const int32_t* __restrict__ pair_a2, int NP,
                                     const int32_t* __restrict__ rec_part,
                                     const int64_t* __restrict__ ent_ptr,
                                     int64_t r, int A, uint32_t nd_mask) {
  int base_attr = -1;
  LinkBase b{0, INT64_MAX, 0, true};
  for (uint32_t m = nd_mask; m;) {
    const int a = __ffs(m) - 1;
    m &= m - 1;
    const CandRange c = range(a);
    const int64_t lo = c.lo, n = c.hi - lo;
    if (n < b.n) { b.n = n; b.lo = lo; base_attr = a; }
  }
  for (int t = 0; t < NP; ++t) {
    const int a1 = pair_a1[t], a2 = pair_a2[t];
    if (((nd_mask >> a1) & 1u) == 0 || ((nd_mask >> a2) & 1u) == 0) continue;
    const CandRange c = range(A + t);
    const int64_t lo = c.lo, n = c.hi - lo;
    if (n < b.n) { b.n = n; b.lo = lo; base_attr = -1; }
  }
  if (nd_mask == 0) {
    const int32_t p = rec_part[r];
    b.lo = ent_ptr[p];
    b.n = ent_ptr[p + 1] - b.lo;
    b.postings = false;
  }
  b.check_mask = base_attr >= 0 ? (nd_mask & ~(1u << base_attr)) : nd_mask;
  return b;
}

DBL_D LinkBase link_select_base(const int64_t* __restrict__ cand_lo,
                                const int64_t* __restrict__ cand_hi,
                                const int32_t* __restrict__ pair_a1,
                                const int32_t* __restrict__ pair_a2, int NP,
                                const int32_t* __restrict__ rec_part,
                                const int64_t* __restrict__ ent_ptr,
                                int64_t r, int A, uint32_t nd_mask) {
  const int T = A + NP;
  return link_select_base_from(
      [&](int t) { return CandRange{cand_lo[r * T + t], cand_hi[r * T + t]}; },
      pair_a1, pair_a2, NP, rec_part, ent_ptr, r, A, nd_mask);
}

// Entity e equals record r on every attribute in mask.
DBL_D bool link_matches(const int32_t* __restrict__ ent_values,
                        const int32_t* __restrict__ rec_values, int64_t e,
                        int64_t r, int A, uint32_t mask) {
  for (uint32_t m = mask; m;) {
    const int a = __ffs(m) - 1;
    m &= m - 1;
    if (ent_values[e * A + a] != rec_values[r * A + a]) return false;
  }
  return true;
}

// f32 observed-distorted log-weight of entity e for record r:
// sum over od attrs (ascending) of log_norm(y) + sim(x, y), each term added
// as one f32 sum — the order every path must share to stay bitwise equal.
// sim(a, row, y) is the lookup (staged or global); attribute a_given, if
// any, takes sim_given instead (the heavy S_r scan enumerates by sim row).
template <class Sim>
DBL_D float link_logw(const int32_t* __restrict__ ent_values,
                      const int32_t* __restrict__ rec_values,
                      const float* __restrict__ log_norm,
                      const int64_t* __restrict__ voff, int64_t e, int64_t r,
                      int A, uint32_t od_mask, const Sim& sim,
                      int a_given = -1, float sim_given = 0.0f) {
  float logw = 0.0f;
  for (uint32_t m = od_mask; m;) {
    const int a = __ffs(m) - 1;
    m &= m - 1;
    const int32_t y = ent_values[e * A + a];
    logw += log_norm[voff[a] + y] +
            (a == a_given ? sim_given
                          : sim(a, voff[a] + rec_values[r * A + a], y));
  }
  return logw;
}

// Empty candidate set (state invariant violated): count it, keep the link.
DBL_D long long link_winner_or_keep(long long best_e,
                                    const int64_t* __restrict__ rec_ent_in,
                                    int64_t r, int* __restrict__ error_count) {
  if (best_e >= 0) return best_e;
  atomicAdd(error_count, 1);
  return rec_ent_in[r];
}

// ---------------------------------------------------------------------------
// K3+K4+K5: link update (PCG-I / Gibbs indexed path)
//
// Posting lists are used ONLY to enumerate the smallest candidate set;
// membership in every other non-distorted attribute's posting list is
// equivalent to a direct entity-value comparison (the posting list of
// (partition, attr, v) is exactly the entities whose attr equals v), so no
// binary search / bitmap is needed and posting order is irrelevant — which
// is what lets the index build be an unstable counting sort.
// ---------------------------------------------------------------------------

// One wave scans record r's base list (the body of link_update_kernel and of
// the wave blocks of link_update_merged_kernel).
DBL_D void link_wave_record(
    const int32_t* __restrict__ rec_values,  // [R, A]
    const uint8_t* __restrict__ rec_dist,    // [R, A]
    const int64_t* __restrict__ rec_gid,     // [R]
    const int32_t* __restrict__ rec_part,    // [R]
    const int64_t* __restrict__ cand_lo,     // [R, A]
    const int64_t* __restrict__ cand_hi,     // [R, A]
    const int32_t* __restrict__ postings,    // [E*A]
    const int32_t* __restrict__ ent_values,  // [E, A]
    const int64_t* __restrict__ ent_ptr,     // [P+1]
    const float* __restrict__ log_norm,      // [Vtot]
    const int64_t* __restrict__ voff,        // [A+1]
    const int64_t* __restrict__ csr_row_ptr, // [Vtot+1]
    const int32_t* __restrict__ csr_col,
    const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const,  // [A]
    const int32_t* __restrict__ pair_a1,     // [NP] const-pair pseudo slots
    const int32_t* __restrict__ pair_a2, int NP,
    const uint8_t* __restrict__ small_mask,  // [R] 1 = handled by small kernel (or null)
    int64_t R, int A,
    uint64_t seed, uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out,       // [R]
    const int64_t* __restrict__ rec_ent_in,  // [R]
    int* __restrict__ error_count, int simh_on,
    int64_t split_len,                       // 0 = no split path
    int32_t* __restrict__ split_list,        // [R] records left to the split kernel
    int* __restrict__ split_count,           // null: the list was built earlier
    int32_t* simh_k, float* simh_v,          // this wave's SIMH_CAP-entry LDS tables
    int64_t r) {
  const int lane = threadIdx.x & (WAVE - 1);
  if (r >= R) return;
  if (small_mask != nullptr && small_mask[r]) return;
  ctrl_override(ctrl, seed, iteration);

  // All rec_values/voff reads below are wave-uniform, so they compile to
  // scalar-cache loads and cost nothing per candidate.
  const auto [nd_mask, od_mask] =
      link_classify(rec_values, rec_dist, attr_const, r, A);
  const LinkBase base = link_select_base(cand_lo, cand_hi, pair_a1, pair_a2,
                                         NP, rec_part, ent_ptr, r, A, nd_mask);
  // a list longer than split_len is not scanned by one wave: the record goes
  // on the list that link_update_split_kernel serves in the next launch
  if (split_len > 0 && base.n > split_len) {
    if (lane == 0 && split_count != nullptr)
      split_list[atomicAdd(split_count, 1)] = (int32_t)r;
    return;
  }

  const uint64_t gid = (uint64_t)rec_gid[r];
  // stage this record's od-attr sim rows into LDS when the scan is long
  // enough to amortize the fill (short scans: the binary search is cheaper)
  uint64_t logpk = 0, offpk = 0;
  if (simh_on && od_mask && base.n * __popc(od_mask) >= 32)
    simh_stage<WAVE>(simh_k, simh_v, lane, csr_row_ptr, csr_col, csr_sim, voff,
               rec_values, r, A, od_mask, logpk, offpk);
  const auto sim = [&](int a, int64_t row, int32_t y) {
    return simh_lookup(simh_k, simh_v, logpk, offpk, a, csr_row_ptr, csr_col,
                       csr_sim, row, y);
  };
  float best_score = -INFINITY;
  long long best_e = -1;
  for (int64_t i = lane; i < base.n; i += WAVE) {
    int32_t e = base.postings ? postings[base.lo + i] : (int32_t)(base.lo + i);
    if (!link_matches(ent_values, rec_values, e, r, A, base.check_mask)) continue;
    const float logw =
        link_logw(ent_values, rec_values, log_norm, voff, e, r, A, od_mask, sim);
    const float g = gumbel_from_uniform(
        philox_uniform(seed, iteration, PH_LINK, gid, (uint32_t)e));
    if (logw + g > best_score) { best_score = logw + g; best_e = e; }
  }
  wave_argmax(best_score, best_e);
  if (lane == 0)
    rec_ent_out[r] = link_winner_or_keep(best_e, rec_ent_in, r, error_count);
}

__global__ void link_update_kernel(
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    const int32_t* __restrict__ postings, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ ent_ptr, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, const int32_t* __restrict__ pair_a1,
    const int32_t* __restrict__ pair_a2, int NP,
    const uint8_t* __restrict__ small_mask, int64_t R, int A, uint64_t seed,
    uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count, int simh_on, int64_t split_len,
    int32_t* __restrict__ split_list, int* __restrict__ split_count) {
  __shared__ int32_t simh_k_s[4][SIMH_CAP];  // launcher uses WPB == 4
  __shared__ float simh_v_s[4][SIMH_CAP];
  const int wid = threadIdx.x / WAVE;
  link_wave_record(rec_values, rec_dist, rec_gid, rec_part, cand_lo, cand_hi, postings,
                   ent_values, ent_ptr, log_norm, voff, csr_row_ptr, csr_col, csr_sim,
                   attr_const, pair_a1, pair_a2, NP, small_mask, R, A, seed, iteration,
                   ctrl, rec_ent_out, rec_ent_in, error_count, simh_on, split_len,
                   split_list, split_count, simh_k_s[wid], simh_v_s[wid],
                   (int64_t)blockIdx.x * (blockDim.x / WAVE) + wid);
}

// Thread-per-record link update for records whose smallest candidate list is
// short (the common case once clusters localize): one thread walks the
// intersection serially — 64x fewer wave slots than the wave path. Same
// core as the wave kernel, sim rows read from global memory (no LDS).
__global__ void link_update_small_kernel(
    const uint8_t* __restrict__ small_mask, int64_t n_recs,
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    const int32_t* __restrict__ postings, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ ent_ptr, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, const int32_t* __restrict__ pair_a1,
    const int32_t* __restrict__ pair_a2, int NP, int A, uint64_t seed,
    uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_recs || small_mask[r] != 1) return;
  ctrl_override(ctrl, seed, iteration);

  const auto [nd_mask, od_mask] =
      link_classify(rec_values, rec_dist, attr_const, r, A);
  const LinkBase base = link_select_base(cand_lo, cand_hi, pair_a1, pair_a2,
                                         NP, rec_part, ent_ptr, r, A, nd_mask);
  const auto sim = [&](int, int64_t row, int32_t y) {
    return sim_lookup(csr_row_ptr, csr_col, csr_sim, row, y);
  };
  const uint64_t gid = (uint64_t)rec_gid[r];
  float best_score = -INFINITY;
  long long best_e = -1;
  for (int64_t i = base.lo; i < base.lo + base.n; ++i) {
    const int32_t e = base.postings ? postings[i] : (int32_t)i;
    if (!link_matches(ent_values, rec_values, e, r, A, base.check_mask)) continue;
    const float logw =
        link_logw(ent_values, rec_values, log_norm, voff, e, r, A, od_mask, sim);
    const float g = gumbel_from_uniform(
        philox_uniform(seed, iteration, PH_LINK, gid, (uint32_t)e));
    if (logw + g > best_score) { best_score = logw + g; best_e = e; }
  }
  rec_ent_out[r] = link_winner_or_keep(best_e, rec_ent_in, r, error_count);
}

// Block-per-record link update for the few records whose base list is long
// (a partition-sized scan, or a low-cardinality posting range). On the wave
// kernel such a record is ~40 dependent rounds of gathers on one wave while
// the chip idles; here LINK_SPLIT_WAVES waves stride the same list, the od
// sim rows are staged once per block, and the argmax is combined in LDS.
//
// The winner must be the wave kernel's, f32 ties included (two candidates
// of equal log-weight tie whenever their uniforms round to the same float,
// which happens at partition-sized lists). There, with i the position in the
// base list, lane i % 64 keeps the first maximum it meets under strict '>',
// i.e. the lowest i / 64, and wave_argmax's shuffle tree keeps, among equal
// scores, the lane whose id is lowest read with its 6 bits REVERSED (the
// last step pits even lanes against odd ones and the even side stays, the
// step before decides bit 1, ...). So the total order is: higher score, then
// lower bit-reversed i % 64, then lower i / 64. Thread t scans positions
// t, t + 1024, ... in ascending order (same i % 64, ascending i / 64), and
// link_split_better() below carries the position through both reductions.
constexpr int LINK_SPLIT_WAVES = 16;
constexpr int LINK_SPLIT_THREADS = LINK_SPLIT_WAVES * WAVE;

DBL_D bool link_split_better(float s_a, int64_t i_a, float s_b, int64_t i_b) {
  if (s_a != s_b) return s_a > s_b;
  const uint32_t la = __brev((uint32_t)(i_a & 63)) >> 26;
  const uint32_t lb = __brev((uint32_t)(i_b & 63)) >> 26;
  if (la != lb) return la < lb;
  return i_a < i_b;
}

// The block serves entries first, first + stride, ... of the list (the body
// of link_update_split_kernel and of the split blocks of
// link_update_merged_kernel). simh_k/simh_v: SIMH_CAP entries; red_*: one
// slot per wave.
DBL_D void link_split_block(
    const int32_t* __restrict__ split_list, const int* __restrict__ split_count,
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    const int32_t* __restrict__ postings, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ ent_ptr, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, const int32_t* __restrict__ pair_a1,
    const int32_t* __restrict__ pair_a2, int NP, int A, uint64_t seed,
    uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count, int simh_on, int32_t* simh_k, float* simh_v,
    float* red_s, int64_t* red_i, long long* red_e, int first, int stride) {
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wid = tid / WAVE;
  ctrl_override(ctrl, seed, iteration);
  // the list was completed by the previous launch; a list longer than the
  // (static) grid is served by the stride
  const int n_listed = *split_count;
  for (int j = first; j < n_listed; j += stride) {
    const int64_t r = split_list[j];
    const auto [nd_mask, od_mask] =
        link_classify(rec_values, rec_dist, attr_const, r, A);
    const LinkBase base = link_select_base(cand_lo, cand_hi, pair_a1, pair_a2,
                                           NP, rec_part, ent_ptr, r, A, nd_mask);
    const uint64_t gid = (uint64_t)rec_gid[r];
    uint64_t logpk = 0, offpk = 0;
    if (simh_on && od_mask)
      simh_stage<LINK_SPLIT_THREADS>(simh_k, simh_v, tid, csr_row_ptr, csr_col,
                                     csr_sim, voff, rec_values, r, A, od_mask,
                                     logpk, offpk);
    __syncthreads();  // table complete (and red_* of the last record read)
    const auto sim = [&](int a, int64_t row, int32_t y) {
      return simh_lookup(simh_k, simh_v, logpk, offpk, a, csr_row_ptr, csr_col,
                         csr_sim, row, y);
    };
    float best_score = -INFINITY;
    long long best_e = -1;
    int64_t best_i = INT64_MAX;
    for (int64_t i = tid; i < base.n; i += LINK_SPLIT_THREADS) {
      int32_t e = base.postings ? postings[base.lo + i] : (int32_t)(base.lo + i);
      if (!link_matches(ent_values, rec_values, e, r, A, base.check_mask)) continue;
      const float logw =
          link_logw(ent_values, rec_values, log_norm, voff, e, r, A, od_mask, sim);
      const float g = gumbel_from_uniform(
          philox_uniform(seed, iteration, PH_LINK, gid, (uint32_t)e));
      if (logw + g > best_score) { best_score = logw + g; best_e = e; best_i = i; }
    }
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
      const float other_s = __shfl_down(best_score, off);
      const long long other_e = __shfl_down(best_e, off);
      const int64_t other_i = __shfl_down(best_i, off);
      if (lane + off < WAVE && other_e >= 0 &&
          (best_e < 0 || link_split_better(other_s, other_i, best_score, best_i))) {
        best_score = other_s; best_e = other_e; best_i = other_i;
      }
    }
    if (lane == 0) { red_s[wid] = best_score; red_i[wid] = best_i; red_e[wid] = best_e; }
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < LINK_SPLIT_WAVES; ++w)
        if (red_e[w] >= 0 &&
            (best_e < 0 || link_split_better(red_s[w], red_i[w], best_score, best_i))) {
          best_score = red_s[w]; best_i = red_i[w]; best_e = red_e[w];
        }
      rec_ent_out[r] = link_winner_or_keep(best_e, rec_ent_in, r, error_count);
    }
    // no barrier here: the next record's staging touches simh_* only, which
    // every wave has finished probing, and red_* is rewritten behind the
    // barrier above, which thread 0 reaches after this combine
  }
}

__global__ void __launch_bounds__(LINK_SPLIT_THREADS) link_update_split_kernel(
    const int32_t* __restrict__ split_list, const int* __restrict__ split_count,
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    const int32_t* __restrict__ postings, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ ent_ptr, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, const int32_t* __restrict__ pair_a1,
    const int32_t* __restrict__ pair_a2, int NP, int A, uint64_t seed,
    uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count, int simh_on) {
  __shared__ int32_t simh_k[SIMH_CAP];
  __shared__ float simh_v[SIMH_CAP];
  __shared__ float red_s[LINK_SPLIT_WAVES];
  __shared__ int64_t red_i[LINK_SPLIT_WAVES];
  __shared__ long long red_e[LINK_SPLIT_WAVES];
  link_split_block(split_list, split_count, rec_values, rec_dist, rec_gid, rec_part,
                   cand_lo, cand_hi, postings, ent_values, ent_ptr, log_norm, voff,
                   csr_row_ptr, csr_col, csr_sim, attr_const, pair_a1, pair_a2, NP, A,
                   seed, iteration, ctrl, rec_ent_out, rec_ent_in, error_count, simh_on,
                   simh_k, simh_v, red_s, red_i, red_e, (int)blockIdx.x,
                   (int)gridDim.x);
}

// Link phase in one launch, once the split list exists before it (built with
// the candidate ranges): blocks [0, n_split) serve the list, the blocks after
// them are wave blocks of LINK_SPLIT_WAVES records each, which skip a listed
// record. The two kinds share no data. The per-wave tables fill the 64 KiB of
// static LDS; a split block uses wave 0's tables and keeps its reduction
// slots in wave 1's key table.
__global__ void __launch_bounds__(LINK_SPLIT_THREADS) link_update_merged_kernel(
    const int32_t* __restrict__ split_list, const int* __restrict__ split_count,
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    const int32_t* __restrict__ postings, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ ent_ptr, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, const int32_t* __restrict__ pair_a1,
    const int32_t* __restrict__ pair_a2, int NP, int64_t R, int A, uint64_t seed,
    uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count, int simh_on, int64_t split_len, unsigned n_split) {
  __shared__ __attribute__((aligned(16))) int32_t simh_k_s[LINK_SPLIT_WAVES][SIMH_CAP];
  __shared__ __attribute__((aligned(16))) float simh_v_s[LINK_SPLIT_WAVES][SIMH_CAP];
  static_assert(SIMH_CAP * sizeof(int32_t) >=
                    LINK_SPLIT_WAVES * (sizeof(float) + 2 * sizeof(int64_t)),
                "reduction slots must fit one wave's key table");
  if (blockIdx.x < n_split) {
    int64_t* red_i = reinterpret_cast<int64_t*>(simh_k_s[1]);
    long long* red_e = reinterpret_cast<long long*>(red_i + LINK_SPLIT_WAVES);
    float* red_s = reinterpret_cast<float*>(red_e + LINK_SPLIT_WAVES);
    link_split_block(split_list, split_count, rec_values, rec_dist, rec_gid, rec_part,
                     cand_lo, cand_hi, postings, ent_values, ent_ptr, log_norm, voff,
                     csr_row_ptr, csr_col, csr_sim, attr_const, pair_a1, pair_a2, NP,
                     A, seed, iteration, ctrl, rec_ent_out, rec_ent_in, error_count,
                     simh_on, simh_k_s[0], simh_v_s[0], red_s, red_i, red_e,
                     (int)blockIdx.x, (int)n_split);
  } else {
    const int wid = threadIdx.x / WAVE;
    link_wave_record(rec_values, rec_dist, rec_gid, rec_part, cand_lo, cand_hi,
                     postings, ent_values, ent_ptr, log_norm, voff, csr_row_ptr,
                     csr_col, csr_sim, attr_const, pair_a1, pair_a2, NP, nullptr, R, A,
                     seed, iteration, ctrl, rec_ent_out, rec_ent_in, error_count,
                     simh_on, split_len, nullptr, nullptr, simh_k_s[wid],
                     simh_v_s[wid],
                     (int64_t)(blockIdx.x - n_split) * LINK_SPLIT_WAVES + wid);
  }
}

// ---------------------------------------------------------------------------
// Heavy link update: hierarchical (A*) Gumbel-max sampler.
//
// In the model's stationary regime the distortion probabilities are large
// (~0.2-0.6 under the shipped demo priors, measured on real RLdata10000), so
// many records have few observed NON-distorted attributes: their candidate
// set is a whole low-cardinality posting range (thousands of entities) or
// the entire partition (GibbsUpdates.scala:398-430 with an empty
// obsNonDistorted set). Scanning those ranges is what made sweeps grow
// ~100x between burn-in and stationarity. This kernel draws the SAME
// categorical (exactly — validated statistically against the scan path)
// in O(|similar set| + tens) per record:
//
//   score(e) = t(e) + sim(e) + gumbel_e,   t(e) = sum_od lognorm(y_e,a) <= 0
//
//   1. exact Gumbel-max over S_r = entities similar to any observed-distorted
//      record value (enumerated via the sim-row's posting segments) that pass
//      the non-distorted equality checks; per-entity keyed gumbels.
//   2. the complement (sim == 0) via A* sampling with a UNIFORM proposal
//      (q = 0 >= t since every log-normalizer is <= 0): successive maxima
//      G_1 > G_2 > ... of the pool's gumbels via truncated-Gumbel draws;
//      each drawn entity is excluded (Z -= 1) and, if it passes the checks
//      and is not similar, scores t(e) + G_k. Stop when G <= current best
//      (no remaining candidate can win: t <= 0).
//   3. winner = argmax of the two halves. Independent keyed RNG streams per
//      half keep the combined draw an exact categorical sample.
//
// All draws are keyed by (seed, iteration, record gid, counter), so results
// are deterministic and independent of posting order. If the A* loop hits
// its exclusion cap (rare; counted in stats[1]), the record falls back to a
// deterministic full scan with a FRESH key stream (PH_LINKF) — exact
// regardless of what the truncated chain did.
// ---------------------------------------------------------------------------

constexpr int HEAVY_EXC_CAP = 512;   // A* exclusions per record before fallback
constexpr int HEAVY_HASH = 1024;     // LDS exclusion hash slots per wave
constexpr int HEAVY_WAVES = 4;

__global__ void link_update_heavy_kernel(
    const uint8_t* __restrict__ mode,        // [R] 2 = heavy
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int32_t* __restrict__ ent_values, const int64_t* __restrict__ ent_ptr,
    const float* __restrict__ log_norm, const int64_t* __restrict__ voff,
    const int64_t* __restrict__ csr_row_ptr, const int32_t* __restrict__ csr_col,
    const float* __restrict__ csr_sim, const uint8_t* __restrict__ attr_const,
    const int64_t* __restrict__ csr_row_ptr_big,
    const int32_t* __restrict__ csr_col_big, const float* __restrict__ csr_sim_big,
    float tau,
    const int32_t* __restrict__ postings, const int64_t* __restrict__ idx_ptr,
    int64_t Vmax, int NP, int64_t R, int A,
    uint64_t seed, uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, const int64_t* __restrict__ rec_ent_in,
    int* __restrict__ error_count,
    unsigned long long* __restrict__ stats, int simh_on) {
  // stats[4] (or null): {A* iterations, fallbacks, S_r visits, heavy records}
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  __shared__ int32_t simh_k_s[HEAVY_WAVES][SIMH_CAP];
  __shared__ float simh_v_s[HEAVY_WAVES][SIMH_CAP];
  const int64_t r = (int64_t)blockIdx.x * HEAVY_WAVES + wid;
  if (r >= R || mode[r] != 2) return;
  ctrl_override(ctrl, seed, iteration);

  const int T = A + NP;
  const auto [nd_mask, od_mask] =
      link_classify(rec_values, rec_dist, attr_const, r, A);
  const int32_t p = rec_part[r];
  const int64_t e0 = ent_ptr[p], e1 = ent_ptr[p + 1];
  const uint64_t gid = (uint64_t)rec_gid[r];

  // proposal pool: the whole partition (no nd attr) or the base posting
  // segment of the single nd attr (postings are stable-sorted when this
  // kernel is active, so indexed draws are deterministic)
  const bool seg_pool = nd_mask != 0;
  int64_t plo, pn;
  if (seg_pool) {
    const int a = __ffs(nd_mask) - 1;
    const int64_t key = ((int64_t)p * T + a) * Vmax + rec_values[r * A + a];
    plo = idx_ptr[key];
    pn = idx_ptr[key + 1] - plo;
  } else {
    plo = e0;
    pn = e1 - e0;
  }

  // heavy scans are always long: stage the record's od-attr sim rows in LDS
  uint64_t logpk = 0, offpk = 0;
  int32_t* simh_k = simh_k_s[wid];
  float* simh_v = simh_v_s[wid];
  if (simh_on && od_mask)
    simh_stage<WAVE>(simh_k, simh_v, lane, csr_row_ptr, csr_col, csr_sim, voff,
               rec_values, r, A, od_mask, logpk, offpk);
  const auto sim = [&](int a, int64_t row, int32_t y) {
    return simh_lookup(simh_k, simh_v, logpk, offpk, a, csr_row_ptr, csr_col,
                       csr_sim, row, y);
  };

  // ---- 1. exact scan over the similar set S_r ----------------------------
  // The sim-row's posting segments average only a few entries, so a
  // segment-at-a-time wave loop would idle ~60 of 64 lanes. Instead each
  // 64-column chunk is flattened warp-cooperatively: a register prefix scan
  // of the segment lengths, then lanes stride the flat space and locate
  // their owning column by a shuffle-based binary search.
  float best_f = -INFINITY;
  long long best_e = -1;
  for (uint32_t m = od_mask; m;) {
    const int a = __ffs(m) - 1;
    m &= m - 1;
    const int64_t row = voff[a] + rec_values[r * A + a];
    const int64_t j0 = csr_row_ptr_big[row], j1 = csr_row_ptr_big[row + 1];
    for (int64_t cbase = j0; cbase < j1; cbase += WAVE) {
      const int64_t myj = cbase + lane;
      long long lo = 0;
      int n = 0;
      float simv = 0.0f;
      if (myj < j1) {
        const int64_t key = ((int64_t)p * T + a) * Vmax + csr_col_big[myj];
        lo = idx_ptr[key];
        n = (int)(idx_ptr[key + 1] - lo);
        simv = csr_sim_big[myj];
      }
      int pre = n;  // inclusive prefix of segment lengths across lanes
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const int v = __shfl_up(pre, off);
        if (lane >= off) pre += v;
      }
      const int total = __shfl(pre, WAVE - 1);
      const int excl = pre - n;
      for (int sb = 0; sb < total; sb += WAVE) {
        const int s = sb + lane;
        // owning lane = last lane with excl <= s (shuffle binary search);
        // every lane participates in the shuffles (uniform loop bound)
        int fl = 0;
#pragma unroll
        for (int step = WAVE / 2; step; step >>= 1) {
          const int cand = fl + step;
          const int ce = __shfl(excl, cand < WAVE ? cand : WAVE - 1);
          if (cand < WAVE && ce <= s) fl = cand;
        }
        const int64_t i = __shfl(lo, fl) + (s - __shfl(excl, fl));
        const float dsim = __shfl(simv, fl);  // sim of the enumerated attr
        if (s >= total) continue;
        const int32_t e = postings[i];
        if (!link_matches(ent_values, rec_values, e, r, A, nd_mask)) continue;
        const float logw = link_logw(ent_values, rec_values, log_norm, voff, e,
                                     r, A, od_mask, sim, a, dsim);
        const float g = gumbel_from_uniform(
            philox_uniform(seed, iteration, PH_LINK, gid, (uint32_t)e));
        if (logw + g > best_f) { best_f = logw + g; best_e = e; }
      }
      if (lane == 0 && stats != nullptr)
        atomicAdd(&stats[2], (unsigned long long)total);
    }
  }
  wave_argmax(best_f, best_e);

  // ---- 2. A* over the complement (lane 0 serial) -------------------------
  // Proposal: uniform with constant shift q = |od| * tau — every pool entity
  // (all big-sims excluded) has score t + sum(small sims) + g <= q + g, so
  // the successive proposal maxima q + G_k bound the remaining candidates.
  __shared__ int32_t exclh_s[HEAVY_WAVES][HEAVY_HASH];
  __shared__ long long winner_s[HEAVY_WAVES];
  __shared__ int fell_back_s[HEAVY_WAVES];
  int32_t* exclh = exclh_s[wid];
  for (int i = lane; i < HEAVY_HASH; i += WAVE) exclh[i] = -1;
  // wave-lockstep: lane 0 reads below see these LDS writes
  if (lane == 0) {
    const double q_shift = (double)tau * (double)__popc(od_mask);
    double best = (best_e >= 0) ? (double)best_f : -INFINITY;
    long long bE = best_e;
    double Z = (double)pn;
    double b = 0.0;
    bool first = true;
    uint32_t ctr = 0;
    int n_exc = 0;
    bool fell_back = false;
    unsigned long long iters = 0;
    while (Z > 0.5) {
      const double logZ = log(Z);
      double G;
      {
        const double u = (double)philox_uniform(seed, iteration, PH_LINKH, gid, ctr++);
        G = first ? logZ - log(-log(u)) : logZ - log(exp(logZ - b) - log(u));
        first = false;
      }
      b = G;
      if (G + q_shift <= best) break;
      // categorical (uniform) draw over pool \ excluded, by pool index;
      // the single-writer LDS hash both tests and records exclusions
      int64_t ci = -1;
      for (int tries = 0; tries < 4 * HEAVY_EXC_CAP; ++tries) {
        const float u = philox_uniform(seed, iteration, PH_LINKH, gid, ctr++);
        int64_t cand = (int64_t)(u * (float)pn);
        if (cand >= pn) cand = pn - 1;
        int h = (int)(((uint32_t)cand * 2654435761u) >> 16) & (HEAVY_HASH - 1);
        bool fresh = false;
        for (;;) {
          const int32_t cur = exclh[h];
          if (cur == (int32_t)cand) break;          // already excluded
          if (cur == -1) { exclh[h] = (int32_t)cand; fresh = true; break; }
          h = (h + 1) & (HEAVY_HASH - 1);
        }
        if (fresh) { ci = cand; break; }
      }
      if (ci < 0 || ++n_exc > HEAVY_EXC_CAP) { fell_back = true; break; }
      Z -= 1.0;
      ++iters;
      const int32_t e = seg_pool ? postings[plo + ci] : (int32_t)(plo + ci);
      if (!link_matches(ent_values, rec_values, e, r, A, nd_mask)) continue;
      // f64 log-weight with the tau early exit: not link_logw (that one is
      // f32 and has no exit), and must stay in step with it by hand
      double t = 0.0;
      bool in_big = false;
      for (uint32_t mo = od_mask; mo;) {
        const int ao = __ffs(mo) - 1;
        mo &= mo - 1;
        const int32_t y = ent_values[(int64_t)e * A + ao];
        const float s = sim(ao, voff[ao] + rec_values[r * A + ao], y);
        if (s >= tau) { in_big = true; break; }  // scored exactly in S_r
        t += (double)(log_norm[voff[ao] + y] + s);
      }
      if (in_big) continue;
      const double s_true = t + G;  // gumbel realization of this draw == G
      if (s_true > best) { best = s_true; bE = e; }
    }
    winner_s[wid] = bE;
    fell_back_s[wid] = fell_back ? 1 : 0;
    if (stats != nullptr) {
      atomicAdd(&stats[0], iters);
      if (fell_back) atomicAdd(&stats[1], 1ull);
      atomicAdd(&stats[3], 1ull);  // heavy records processed
    }
  }
  __syncthreads();

  // ---- 3. rare fallback: deterministic full scan, fresh key stream -------
  if (fell_back_s[wid]) {
    float bf = -INFINITY;
    long long be = -1;
    for (int64_t e = e0 + lane; e < e1; e += WAVE) {
      if (!link_matches(ent_values, rec_values, e, r, A, nd_mask)) continue;
      const float logw = link_logw(ent_values, rec_values, log_norm, voff, e,
                                   r, A, od_mask, sim);
      const float g = gumbel_from_uniform(
          philox_uniform(seed, iteration, PH_LINKF, gid, (uint32_t)(e - e0)));
      if (logw + g > bf) { bf = logw + g; be = e; }
    }
    wave_argmax(bf, be);
    if (lane == 0) winner_s[wid] = be;
  }
  if (lane == 0)
    rec_ent_out[r] =
        link_winner_or_keep(winner_s[wid], rec_ent_in, r, error_count);
}

// ---------------------------------------------------------------------------
// Dense link update: PCG-II (collapsed) and Gibbs-Sequential
// ---------------------------------------------------------------------------

__global__ void link_update_dense_kernel(
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int64_t* __restrict__ rec_gid, const int32_t* __restrict__ rec_part,
    const int32_t* __restrict__ rec_file,
    const int32_t* __restrict__ ent_values, const int64_t* __restrict__ ent_ptr,
    const float* __restrict__ theta,       // [A, F]
    const float* __restrict__ phi,         // [Vtot] linear probability
    const float* __restrict__ norm_lin,    // [Vtot] linear 1/normalizer
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, int64_t R, int A, int F,
    int collapsed,  // 1 = PCG-II weights, 0 = Gibbs-Sequential weights
    uint64_t seed, uint32_t iteration, const int64_t* __restrict__ ctrl,
    int64_t* __restrict__ rec_ent_out, int simh_on) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wid = threadIdx.x / WAVE;
  __shared__ int32_t simh_k_s[4][SIMH_CAP];  // launcher uses WPB == 4
  __shared__ float simh_v_s[4][SIMH_CAP];
  const int64_t r = (int64_t)blockIdx.x * (blockDim.x / WAVE) + wid;
  if (r >= R) return;
  ctrl_override(ctrl, seed, iteration);
  const int32_t p = rec_part[r];
  const int64_t e0 = ent_ptr[p], e1 = ent_ptr[p + 1];
  const int f = rec_file[r];
  const uint64_t gid = (uint64_t)rec_gid[r];

  // stage the record's sim rows once per wave: the dense scan pays a
  // sim_lookup per (entity, attr), all against rows fixed for this record
  uint32_t st_mask = 0;
  for (int a = 0; a < A; ++a) {
    if (rec_values[r * A + a] < 0 || attr_const[a]) continue;
    if (collapsed || rec_dist[r * A + a]) st_mask |= 1u << a;
  }
  uint64_t logpk = 0, offpk = 0;
  int32_t* simh_k = simh_k_s[wid];
  float* simh_v = simh_v_s[wid];
  if (simh_on && st_mask && (e1 - e0) * __popc(st_mask) >= 32)
    simh_stage<WAVE>(simh_k, simh_v, lane, csr_row_ptr, csr_col, csr_sim, voff,
               rec_values, r, A, st_mask, logpk, offpk);

  float best_score = -INFINITY;
  long long best_e = -1;
  for (int64_t e = e0 + lane; e < e1; e += WAVE) {
    float logw = 0.0f;
    for (int a = 0; a < A; ++a) {
      const int32_t x = rec_values[r * A + a];
      if (x < 0) continue;
      const int32_t y = ent_values[e * A + a];
      if (collapsed) {
        const float th = theta[a * F + f];
        float like = phi[voff[a] + x];
        if (!attr_const[a]) {
          float s = simh_lookup(simh_k, simh_v, logpk, offpk, a, csr_row_ptr,
                                csr_col, csr_sim, voff[a] + x, y);
          like *= norm_lin[voff[a] + y] * __expf(s);
        }
        float w = (y == x ? 1.0f - th : 0.0f) + th * like;
        logw += __logf(w);
      } else {
        // Gibbs-Sequential: non-distorted must match exactly
        if (!rec_dist[r * A + a]) {
          if (x != y) { logw = -INFINITY; break; }
        } else if (!attr_const[a]) {
          float s = simh_lookup(simh_k, simh_v, logpk, offpk, a, csr_row_ptr,
                                csr_col, csr_sim, voff[a] + x, y);
          logw += __logf(norm_lin[voff[a] + y]) + s;  // phi(x) constant: cancels
        }
      }
    }
    if (logw == -INFINITY) continue;
    float g = gumbel_from_uniform(
        philox_uniform(seed, iteration, PH_LINK, gid, (uint32_t)(e - e0)));
    float score = logw + g;
    if (score > best_score) { best_score = score; best_e = e; }
  }
  wave_argmax(best_score, best_e);
  if (lane == 0) rec_ent_out[r] = best_e;  // weights always > 0 when collapsed
}

// ---------------------------------------------------------------------------
// K6: value update
// ---------------------------------------------------------------------------

// LDS hash table per wave for sparse perturbation weights.
constexpr int HASH_CAP = 1024;            // slots per wave
constexpr int WAVES_PER_BLOCK_VAL = 4;    // 256 threads
constexpr int VAL_DMAX = 16;              // distinct (value, file) groups per pair

struct ValueArgs {
  const int64_t* ctrl;         // [2] = {seed, iteration} device override (or null)
  const int64_t* pair_list;    // [n_pairs] flattened (e*A + a) (or null)
  const int32_t* kobs;         // [E*A] observed-linked counts for self-selection (or null)
  int64_t n_pairs;
  const double* csr_excl;      // [nnz] exclusive row prefix of raw k=1 weights
  const double* csr_rawsum;    // [Vtot] row totals of raw k=1 weights
  const double* z1;            // [A] power-1 normalizer Z_1
  // k >= 2 single-distinct-value tables (set_value_ktables): level k-2
  const double* tab_excl;      // [(kmax-1) * nnz] exclusive row prefixes
  const double* tab_rawsum;    // [(kmax-1) * Vtot] row totals
  const float* self_expsim;    // [Vtot]
  int ktab_max;                // largest k covered (0 = disabled)
  int64_t nnz;
  // 2-distinct-value (k, m) tables: level (k-2)(k-1)/2 + m - 1
  const double* tab2_excl;
  const double* tab2_rawsum;
  int k2tab_max;
  const int32_t* rec_values;
  const uint8_t* rec_dist;
  const int32_t* rec_file;
  const int64_t* ent_rec_ptr;  // [E+1]
  const int64_t* ent_rec_idx;  // [R] record rows grouped by entity
  int32_t* ent_values;         // [E, A] in/out
  const float* theta;          // [A, F]
  const float* phi;            // [Vtot]
  const float* log_phi;        // [Vtot]
  const float* norm_lin;       // [Vtot]
  const float* log_norm;       // [Vtot]
  const int64_t* voff;         // [A+1]
  const int64_t* csr_row_ptr;
  const int32_t* csr_col;
  const float* csr_sim;
  const float* phi_prob;       // [Vtot] alias prob for phi
  const int32_t* phi_alias;    // [Vtot]
  const float* pow_prob;       // power-dist alias tables, concatenated
  const int32_t* pow_alias;
  const int64_t* pow_off;      // [A] offset into pow_* for k=1 (or -1)
  const float* log_pow_total;  // [A * (Kc+1)] log Z_k (index a*(Kc+1)+k)
  const uint8_t* attr_const;
  int Kc;
  int64_t E;
  int A, F;
  int collapsed;
  uint64_t seed;
  uint32_t iteration;
  uint64_t ent_id_base;
  int* error_count;
  // optional [8]: {k2_pairs, hash_pairs, merge_pairs, sum_entries,
  //                sum_units, sum_kobs, rare_pairs, merge_entries}
  unsigned long long* stats;
  int vchunk;  // 1 = chunked hash-accumulate dense path (DBLINK_VCHUNK)
  // list mode (kobs mode only, or null): the k >= 2 pairs of the hash and the
  // merge kernel, classified once per sweep by value_update_kd1_kernel. One
  // [E*A] buffer holds both lists: hash pairs fill it from the front, merge
  // pairs from the back (a pair is on at most one list).
  int32_t* pair_lists;
  int* list_count;  // [2] = {hash pairs, merge pairs}, zeroed by the caller
};

// --- shared draw core --------------------------------------------------------
// Every value kernel below is built from these pieces. Which kernel (and
// which k >= 2 path inside it) handles a pair is a performance decision; the
// distribution drawn from must not depend on it, so the pieces exist once.

struct ValuePair {
  int64_t e;
  int a;
  int64_t v0;     // attribute a's offset into the value-indexed tables
  int V;          // attribute a's domain size
  uint64_t elem;  // Philox element id of the pair
  bool is_const;
};

DBL_D ValuePair value_pair_of(const ValueArgs& args, int64_t pair) {
  const int64_t e = pair / args.A;
  const int a = (int)(pair % args.A);
  const bool is_const = args.attr_const[a];
  const int64_t v0 = args.voff[a];
  const int V = (int)(args.voff[a + 1] - v0);
  const uint64_t elem = (args.ent_id_base + (uint64_t)e) * 32u + (uint64_t)a;
  return {e, a, v0, V, elem, is_const};
}

// --- which kernel owns a k >= 2 pair ----------------------------------------
// Exactly one kernel writes each pair. The predicates exist once, here: the
// wave kernels apply them inside value_update_pair, and list mode applies
// them once per pair and sweep in value_route (thread-per-pair), so that the
// wave kernels only ever see their own pairs.
constexpr int VOWN_HASH = 0, VOWN_MERGE = 1, VOWN_KD1 = 2, VOWN_KD2 = 3;

// Settled without perturbation weights: the non-collapsed copy of a held
// (non-distorted) value, or a constant attribute's non-collapsed base draw.
DBL_D bool value_settles_early(const ValueArgs& args, bool is_const, bool has_nondist) {
  return !args.collapsed && (has_nondist || is_const);
}

// The sim rows of the pair's units overflow the per-wave LDS hash.
DBL_D bool value_is_dense(int64_t total_entries) {
  return total_entries > (HASH_CAP * 3) / 4;
}

// One (value, file) group with cached k-tables: value_update_kd1_kernel's.
DBL_D bool value_goes_kd1(const ValueArgs& args, bool is_const, bool gover, int d,
                          int k_obs) {
  return args.kobs != nullptr && args.tab_excl != nullptr && !is_const && !gover &&
         d == 1 && k_obs <= args.ktab_max && k_obs <= args.Kc;
}

// Two distinct VALUES with cached (k, m) tables: value_update_kd2_kernel's.
DBL_D bool value_goes_kd2(const ValueArgs& args, bool is_const, bool gover, int d,
                          int k_obs, int32_t x0, int32_t x1) {
  return args.kobs != nullptr && args.tab2_excl != nullptr && !is_const && !gover &&
         d == 2 && k_obs <= args.k2tab_max && x0 != x1;
}

DBL_D int64_t value_row_entries(const ValueArgs& args, const ValuePair& p, int32_t x) {
  return p.is_const ? 1
                    : args.csr_row_ptr[p.v0 + x + 1] - args.csr_row_ptr[p.v0 + x];
}

// The owner of pair p (k_obs >= 2) and its first group, by one thread. Groups
// are the distinct (value, file) of the observed records in record order, as
// value_update_pair collects them into gbuf: a record opens a group unless an
// earlier record holds its (value, file), found by re-scanning (k is a
// handful, so no per-thread array). A new group beyond VAL_DMAX sets gover,
// and the units become the k_obs records themselves.
struct ValueRoute { int owner; int32_t x, f; };

DBL_D ValueRoute value_route(const ValueArgs& args, const ValuePair& p, int k_obs) {
  const int a = p.a;
  const int64_t r_lo = args.ent_rec_ptr[p.e], r_hi = args.ent_rec_ptr[p.e + 1];
  bool has_nondist = false, gover = false;
  int d = 0;
  int32_t x0 = -1, f0 = -1, x1 = -1;
  int64_t group_entries = 0, record_entries = 0;
  for (int64_t i = r_lo; i < r_hi; ++i) {
    const int64_t r = args.ent_rec_idx[i];
    const int32_t x = args.rec_values[r * args.A + a];
    if (x < 0) continue;
    if (!args.collapsed && !args.rec_dist[r * args.A + a]) has_nondist = true;
    const int32_t f = args.collapsed ? args.rec_file[r] : 0;
    const int64_t len = value_row_entries(args, p, x);
    record_entries += len;
    if (gover) continue;
    bool seen = false;
    for (int64_t j = r_lo; j < i && !seen; ++j) {
      const int64_t rr = args.ent_rec_idx[j];
      seen = args.rec_values[rr * args.A + a] == x &&
             (args.collapsed ? args.rec_file[rr] : 0) == f;
    }
    if (seen) continue;
    if (d == VAL_DMAX) { gover = true; continue; }
    if (d == 0) { x0 = x; f0 = f; }
    if (d == 1) x1 = x;
    ++d;
    group_entries += len;
  }
  if (value_settles_early(args, p.is_const, has_nondist)) return {VOWN_HASH, x0, f0};
  if (value_goes_kd1(args, p.is_const, gover, d, k_obs)) return {VOWN_KD1, x0, f0};
  if (value_goes_kd2(args, p.is_const, gover, d, k_obs, x0, x1)) return {VOWN_KD2, x0, f0};
  return {value_is_dense(gover ? record_entries : group_entries) ? VOWN_MERGE : VOWN_HASH,
          x0, f0};
}

// The table kernels' four uniforms: mixture test, CDF target (both f64: the
// prefix tables are f64) and the two alias-draw uniforms.
struct ValueUniforms { double u_mix, u_sel; float u_a1, u_a2; };

DBL_D ValueUniforms value_uniforms(const ValueArgs& args, uint64_t elem) {
  const u32x4 rnd = philox4x32(args.seed, (uint32_t)elem, (uint32_t)(elem >> 32),
                               args.iteration ^ (PH_VALM << 24), 0xFFFF0000u);
  return {((double)rnd.x + 0.5) * 2.3283064365386963e-10,
          ((double)rnd.y + 0.5) * 2.3283064365386963e-10,
          u32_to_uniform(rnd.z), u32_to_uniform(rnd.w)};
}

// Value at the last row entry whose exclusive prefix is <= t: first entry
// whose prefix exceeds t, minus one, clamped to the row.
DBL_D int32_t prefix_pick(const double* excl, const int32_t* col, int64_t row_lo,
                          int64_t row_hi, double t) {
  int64_t lo = row_lo, hi = row_hi;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (excl[mid] <= t) lo = mid + 1; else hi = mid;
  }
  int64_t jidx = lo - 1;
  if (jidx < row_lo) jidx = row_lo;
  if (jidx >= row_hi) jidx = row_hi - 1;
  return col[jidx];
}

// Base draw from a cached alias table: phi for const attributes or k == 0
// (GibbsUpdates.scala:584-588), else the power distribution phi norm^k
// (1 <= k <= Kc).
DBL_D int value_base_alias(const ValueArgs& args, const ValuePair& p, int k,
                           float u1, float u2) {
  if (p.is_const || k == 0)
    return alias_draw(args.phi_prob + p.v0, args.phi_alias + p.v0, p.V, u1, u2);
  const int64_t off = args.pow_off[p.a] + (int64_t)(k - 1) * p.V;
  return alias_draw(args.pow_prob + off, args.pow_alias + off, p.V, u1, u2);
}

// Collapsed self term of a record with value x from file f: phi*norm*se
// collapses to (1/theta - 1). The wave paths work in f32 and the table
// kernels in f64; the two are not interchangeable bit for bit.
DBL_D float value_self_f32(const ValueArgs& args, const ValuePair& p, int32_t x,
                           int32_t f) {
  if (!args.collapsed) return 0.0f;
  const float th = args.theta[p.a * args.F + f];
  const float px = args.phi[p.v0 + x];
  return (1.0f / th - 1.0f) / (p.is_const ? px : px * args.norm_lin[p.v0 + x]);
}

DBL_D double value_self_f64(const ValueArgs& args, const ValuePair& p, int32_t x,
                            int32_t f) {
  if (!args.collapsed) return 0.0;
  const double th = (double)args.theta[p.a * args.F + f];
  return (1.0 / th - 1.0) /
         ((double)args.phi[p.v0 + x] * (double)args.norm_lin[p.v0 + x]);
}

// Per-wave LDS open-addressing table (mask = size - 1): vals[slot of v] += x.
DBL_D void lds_hash_add(int32_t* keys, float* vals, uint32_t mask, int32_t v,
                        float x) {
  uint32_t h = ((uint32_t)v * 2654435761u) & mask;
  while (true) {
    const int32_t prev = atomicCAS(&keys[h], -1, v);
    if (prev == -1 || prev == v) { atomicAdd(&vals[h], x); break; }
    h = (h + 1) & mask;
  }
}

DBL_D void lds_hash_clear(int32_t* keys, float* vals, int size, int lane) {
  for (int i = lane; i < size; i += WAVE) { keys[i] = -1; vals[i] = 0.0f; }
  // drain LDS writes before other lanes' atomics may touch the slots
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// Log factor one row entry (value v, log-sim s) of a unit (value ux,
// multiplicity fm) contributes: the self point carries the self term.
DBL_D float row_factor_log(int32_t v, int32_t ux, float s, float fm,
                           float self_extra) {
  return (v == ux && self_extra > 0.0f) ? fm * __logf(__expf(s) + self_extra)
                                        : fm * s;
}

// One support value with summed log factor L > 0 and log base probability
// log_base: weight base * (e^L - 1) into W, keyed Gumbel into the running
// best. log(exp(L) - 1) = L + log1p(-exp(-L)), stable for L > 0.
DBL_D void value_accum(const ValueArgs& args, uint64_t elem, int32_t v, float L,
                       float log_base, double& W, float& best, long long& best_v) {
  const float log_expm1 = L + __logf(1.0f - __expf(-L));
  const float logw = log_base + log_expm1;
  W += (logw < 80.0f) ? (double)__expf(logw) : exp((double)logw);
  const float g = gumbel_from_uniform(
      philox_uniform(args.seed, args.iteration, PH_VALG, elem, (uint32_t)v));
  if (logw + g > best) { best = logw + g; best_v = v; }
}

// Drain the table's atomics, then value_accum every occupied slot.
template <class LogBase>
DBL_D void lds_hash_reduce(const ValueArgs& args, uint64_t elem,
                           const int32_t* keys, const float* vals, int size,
                           int lane, const LogBase& log_base, double& W,
                           float& best, long long& best_v) {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  for (int i = lane; i < size; i += WAVE) {
    const int32_t v = keys[i];
    if (v < 0) continue;
    value_accum(args, elem, v, vals[i], log_base(v), W, best, best_v);
  }
}

// Draw from p(v) ~ phi(v)*norm(v)^k by a dense Gumbel scan (rare path for
// k > Kc where no alias table is cached). Also returns log Z_k via wave sum.
__device__ int dense_power_draw(const ValueArgs& args, int a, int k, uint64_t elem,
                                int lane, float* out_log_total) {
  const int64_t v0 = args.voff[a], v1 = args.voff[a + 1];
  float best = -INFINITY;
  long long best_v = 0;
  double total = 0.0;
  for (int64_t v = v0 + lane; v < v1; v += WAVE) {
    float lw = args.log_phi[v] + (float)k * args.log_norm[v];
    total += exp((double)lw);
    float g = gumbel_from_uniform(philox_uniform(args.seed, args.iteration, PH_VALG,
                                                 elem, (uint32_t)(v - v0) | 0x40000000u));
    if (lw + g > best) { best = lw + g; best_v = v - v0; }
  }
  total = wave_sum(total);
  wave_argmax(best, best_v);
  *out_log_total = (float)log(total);
  return (int)best_v;
}

// Thread-per-pair base draws for empty clusters (k_obs == 0): the base
// distribution is phi for every variant (GibbsUpdates.scala:584-588).
DBL_D void value_base_draw_pair(const ValueArgs& args, int64_t pair) {
  const ValuePair p = value_pair_of(args, pair);
  float u1, u2;
  philox_uniform2(args.seed, args.iteration, PH_VALM, p.elem, 0xFFFF0000u, &u1, &u2);
  args.ent_values[p.e * args.A + p.a] = (int32_t)value_base_alias(args, p, 0, u1, u2);
}

__global__ void value_base_draw_kernel(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= args.n_pairs) return;
  const int64_t pair = args.pair_list ? args.pair_list[i] : i;
  if (args.kobs && args.kobs[pair] != 0) return;
  value_base_draw_pair(args, pair);
}

// Thread-per-pair value update for single-record clusters (k_obs == 1).
// The perturbation distribution for one linked record with value x is STATIC
// per (attribute, x) up to the self-term correction, which is exactly
// (1/theta - 1) of extra raw mass on x. Using the precomputed raw row weights
// raw_w1[j] = phi(col)*norm(col)*(expsim-1), their exclusive row prefix and
// row totals, a draw is: one Philox call, a mixture test, and one binary
// search over the row prefix — O(log row) regardless of row size.
DBL_D void value_update_k1_pair(const ValueArgs& args, int64_t pair) {
  const ValuePair p = value_pair_of(args, pair);
  const int64_t e = p.e, v0 = p.v0;
  const int a = p.a;
  const bool is_const = p.is_const;

  // locate the single observed linked record
  const int64_t r_lo = args.ent_rec_ptr[e], r_hi = args.ent_rec_ptr[e + 1];
  int64_t r = -1;
  int32_t x = -1;
  for (int64_t j = r_lo; j < r_hi; ++j) {
    const int64_t rr = args.ent_rec_idx[j];
    const int32_t xx = args.rec_values[rr * args.A + a];
    if (xx >= 0) { r = rr; x = xx; break; }
  }

  // non-collapsed deterministic copy
  if (!args.collapsed && !args.rec_dist[r * args.A + a]) {
    args.ent_values[e * args.A + a] = x;
    return;
  }

  const ValueUniforms u = value_uniforms(args, p.elem);
  auto base_draw = [&]() -> int {
    return value_base_alias(args, p, 1, u.u_a1, u.u_a2);
  };
  if (!args.collapsed && is_const) {
    args.ent_values[e * args.A + a] = (int32_t)base_draw();
    return;
  }

  // raw perturbation mass (in Z-scaled units): row total + self correction
  double extra = 0.0;
  if (args.collapsed) {
    const float th = args.theta[a * args.F + args.rec_file[r]];
    extra = 1.0 / (double)th - 1.0;  // phi*norm*se collapses to (1/theta - 1)
  }
  double raw_total, Wnorm;
  if (is_const) {
    // row is {x}: raw weight = phi(x)*(factor-1) = phi(x)*se = (1/theta-1)
    raw_total = extra;
    Wnorm = extra <= 0.0 ? 0.0 : extra;  // base = phi (Z = 1), raw already phi-scaled
  } else {
    raw_total = args.csr_rawsum[v0 + x] + extra;
    Wnorm = raw_total / args.z1[a];
  }

  int v_new;
  if (u.u_mix < 1.0 / (1.0 + Wnorm) || raw_total <= 0.0) {
    v_new = base_draw();
  } else if (is_const) {
    v_new = x;  // the only support value
  } else {
    const double t = u.u_sel * raw_total;
    if (t >= args.csr_rawsum[v0 + x])
      v_new = x;  // self-correction mass
    else
      v_new = prefix_pick(args.csr_excl, args.csr_col, args.csr_row_ptr[v0 + x],
                          args.csr_row_ptr[v0 + x + 1], t);
  }
  args.ent_values[e * args.A + a] = (int32_t)v_new;
}

__global__ void value_update_k1_kernel(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= args.n_pairs) return;
  const int64_t pair = args.pair_list ? args.pair_list[i] : i;
  if (args.kobs && args.kobs[pair] != 1) return;
  value_update_k1_pair(args, pair);
}

// Thread-per-pair value update for clusters whose observed linked records
// all share ONE (value, file) — the dominant k >= 2 class (measured d~1.1-1.6
// mean distinct values per pair at 1M/10M stationarity). The perturbation
// weights phi(v) norm(v)^k (e^{k s(x,v)} - 1) are PRECOMPUTED per (value, k)
// (set_value_ktables), so a draw is one Philox call, the theta-dependent
// self-power correction, a mixture test and one binary search — O(log row)
// like the k = 1 kernel, replacing an O(k row) wave merge.
DBL_D void value_update_kd1_pair(const ValueArgs& args, int64_t pair, int k) {
  const ValuePair p = value_pair_of(args, pair);
  const int64_t e = p.e, v0 = p.v0;
  const int a = p.a;
  int32_t x = -1, f = -1;
  if (args.list_count != nullptr) {
    // list mode: this thread already has to scan the pair's records, so it
    // is where every k >= 2 pair is classified, once per sweep. Pairs of
    // the wave kernels go on their lists (order arbitrary: each pair reads
    // records and writes its own ent_values slot only); kd2 self-selects.
    const ValueRoute rt = value_route(args, p, k);
    if (rt.owner == VOWN_HASH)
      args.pair_lists[atomicAdd(&args.list_count[0], 1)] = (int32_t)pair;
    else if (rt.owner == VOWN_MERGE)
      args.pair_lists[args.n_pairs - 1 - atomicAdd(&args.list_count[1], 1)] =
          (int32_t)pair;
    if (rt.owner != VOWN_KD1) return;
    x = rt.x;
    f = rt.f;
  } else {
    if (k > args.ktab_max || p.is_const) return;
    // all observed linked records must share one (value, file); any
    // non-distorted observed record (non-collapsed) defers to the wave path
    const int64_t r_lo = args.ent_rec_ptr[e], r_hi = args.ent_rec_ptr[e + 1];
    for (int64_t j = r_lo; j < r_hi; ++j) {
      const int64_t r = args.ent_rec_idx[j];
      const int32_t xx = args.rec_values[r * args.A + a];
      if (xx < 0) continue;
      if (!args.collapsed && !args.rec_dist[r * args.A + a]) return;
      const int32_t ff = args.collapsed ? args.rec_file[r] : 0;
      if (x < 0) { x = xx; f = ff; }
      else if (xx != x || ff != f) return;  // multi-group: wave path
    }
    if (x < 0) return;
    if (k > args.Kc) return;  // no cached power dist (rare path stays on wave)
  }

  const ValueUniforms u = value_uniforms(args, p.elem);

  const int lvl = k - 2;
  // theta-dependent self correction: the table carries the plain self
  // factor e^{k s(x,x)}; collapsed adds ((e^s + se)^k - e^{ks}) phi norm^k
  double extra = 0.0;
  if (args.collapsed) {
    const double se = value_self_f64(args, p, x, f);
    const double es = (double)args.self_expsim[v0 + x];
    double plain = 1.0, boosted = 1.0;
    for (int t = 0; t < k; ++t) { plain *= es; boosted *= es + se; }
    extra = (boosted - plain) *
            exp((double)args.log_phi[v0 + x] + (double)k * (double)args.log_norm[v0 + x]);
  }
  const double row_total = args.tab_rawsum[(int64_t)lvl * (args.voff[args.A]) + v0 + x];
  const double raw_total = row_total + extra;
  const double Zk = exp((double)args.log_pow_total[a * (args.Kc + 1) + k]);
  const double W = raw_total / Zk;

  int v_new;
  if (u.u_mix < 1.0 / (1.0 + W) || raw_total <= 0.0) {
    v_new = value_base_alias(args, p, k, u.u_a1, u.u_a2);
  } else {
    const double t = u.u_sel * raw_total;
    if (t >= row_total)
      v_new = x;  // the self-correction mass
    else
      v_new = prefix_pick(args.tab_excl + (int64_t)lvl * args.nnz, args.csr_col,
                          args.csr_row_ptr[v0 + x], args.csr_row_ptr[v0 + x + 1], t);
  }
  args.ent_values[e * args.A + a] = (int32_t)v_new;
}

__global__ void value_update_kd1_kernel(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= args.n_pairs) return;
  const int k = args.kobs[i];
  if (k < 2) return;
  value_update_kd1_pair(args, i, k);
}

// The three thread-per-pair kernels above as one launch in kobs mode: they
// cover the same pairs and act on disjoint classes (k = 0, k = 1, k >= 2),
// each writing only its own pair's ent_values word, so one thread reads
// kobs[pair] once and takes its class's branch. `kd1` carries the launcher's
// condition for the k >= 2 kernel.
__global__ void value_update_thread_kernel(ValueArgs args, bool kd1) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int64_t pair = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= args.n_pairs) return;
  const int k = args.kobs[pair];
  if (k == 0) {
    value_base_draw_pair(args, pair);
  } else if (k == 1) {
    value_update_k1_pair(args, pair);
  } else if (k >= 2 && kd1) {
    value_update_kd1_pair(args, pair, k);
  }
}

// Wave-per-pair value update for clusters spanning exactly TWO distinct
// values of an attribute (the remaining k >= 2 mass after kd1): the
// perturbation decomposes into two PRECOMPUTED single-row measures
// phi norm^k (e^{m_i s_i} - 1) (set_value_k2tables, level (k-2)(k-1)/2+m-1)
// plus an exact non-negative residual supported on the two self points and
// the row intersection:
//   w(v) = base_k(v)(F1 F2 - 1)
//        = plain1(v) + plain2(v) + base_k(v)(F1-1)(F2-1) [+ self-se boosts]
// Component sampling: two table CDF binary searches, or a residual re-walk.
// The residual walk strides the SHORTER row across the wave's 64 lanes with
// an ordered f64 prefix scan (identical op order in the total and selection
// passes), so it is deterministic and exact.

__device__ void value_update_kd2_pair(const ValueArgs& args, int64_t pair,
                                      int lane) {
  const int k = args.kobs[pair];
  if (k < 2 || k > args.k2tab_max) return;
  const ValuePair p = value_pair_of(args, pair);
  if (p.is_const) return;
  const int64_t e = p.e, v0 = p.v0;
  const int a = p.a;
  const int64_t Vtot = args.voff[args.A];

  // exactly two first-seen (value, file) groups with DISTINCT values
  // (wave-uniform scalar loads; every lane runs the same scan)
  const int64_t r_lo = args.ent_rec_ptr[e], r_hi = args.ent_rec_ptr[e + 1];
  int32_t x1 = -1, f1 = -1, x2 = -1, f2 = -1;
  int m1 = 0, m2 = 0;
  for (int64_t j = r_lo; j < r_hi; ++j) {
    const int64_t r = args.ent_rec_idx[j];
    const int32_t x = args.rec_values[r * args.A + a];
    if (x < 0) continue;
    if (!args.collapsed && !args.rec_dist[r * args.A + a]) return;
    const int32_t ff = args.collapsed ? args.rec_file[r] : 0;
    if (x1 < 0 || (x == x1 && ff == f1)) { x1 = x; f1 = ff; ++m1; }
    else if (x2 < 0 || (x == x2 && ff == f2)) { x2 = x; f2 = ff; ++m2; }
    else return;  // three or more groups: wave merge path
  }
  if (x2 < 0 || x1 == x2) return;  // d != 2 distinct values

  const int lb = (k - 2) * (k - 1) / 2 - 1;
  const double T1 = args.tab2_rawsum[(int64_t)(lb + m1) * Vtot + v0 + x1];
  const double T2 = args.tab2_rawsum[(int64_t)(lb + m2) * Vtot + v0 + x2];

  auto braw = [&](int32_t v) -> double {
    return exp((double)args.log_phi[v0 + v] +
               (double)k * (double)args.log_norm[v0 + v]);
  };
  const double se1 = value_self_f64(args, p, x1, f1);
  const double se2 = value_self_f64(args, p, x2, f2);

  auto resid_self = [&](int32_t xs, double ses, int ms, int32_t xo,
                        int mo) -> double {
    const double es = (double)args.self_expsim[v0 + xs];
    const float so = sim_lookup(args.csr_row_ptr, args.csr_col, args.csr_sim,
                                v0 + xo, xs);
    const double Fs = pow(es + ses, (double)ms);
    const double Fo = exp((double)so * (double)mo);
    double r = (Fs * Fo - 1.0) - (pow(es, (double)ms) - 1.0);
    if (so != 0.0f) r -= Fo - 1.0;
    r *= braw(xs);
    return r > 0.0 ? r : 0.0;
  };

  const int64_t lo1 = args.csr_row_ptr[v0 + x1], hi1 = args.csr_row_ptr[v0 + x1 + 1];
  const int64_t lo2 = args.csr_row_ptr[v0 + x2], hi2 = args.csr_row_ptr[v0 + x2 + 1];
  const bool first_shorter = (hi1 - lo1) <= (hi2 - lo2);
  const int64_t wlo = first_shorter ? lo1 : lo2;
  const int64_t whi = first_shorter ? hi1 : hi2;
  const int64_t olo = first_shorter ? lo2 : lo1;
  const int64_t ohi = first_shorter ? hi2 : hi1;
  const int mw = first_shorter ? m1 : m2;
  const int mo = first_shorter ? m2 : m1;

  // one lane's residual contribution for walk element j (0 if not in the
  // other row or a self point)
  auto walk_elem = [&](int64_t j) -> double {
    const int32_t v = args.csr_col[j];
    if (v == x1 || v == x2) return 0.0;
    const int64_t p = lower_bound_i32(args.csr_col, olo, ohi, v);
    if (p >= ohi || args.csr_col[p] != v) return 0.0;
    const double Fw = exp((double)args.csr_sim[j] * (double)mw) - 1.0;
    const double Fo = exp((double)args.csr_sim[p] * (double)mo) - 1.0;
    return braw(v) * Fw * Fo;
  };

  const double r_self1 = resid_self(x1, se1, m1, x2, m2);
  const double r_self2 = resid_self(x2, se2, m2, x1, m1);

  // residual pass: lanes stride 64-wide chunks with an ordered inclusive
  // f64 prefix (carry chained across chunks). When target >= 0 the pass
  // selects the first element whose running total crosses it.
  auto residual_pass = [&](double target, int32_t* out_v) -> double {
    double run = r_self1 + r_self2;
    if (out_v != nullptr) {
      if (r_self1 >= target && r_self1 > 0.0) { *out_v = x1; return run; }
      if (run >= target) { *out_v = x2; return run; }
    }
    for (int64_t cb = wlo; cb < whi; cb += WAVE) {
      const int64_t j = cb + lane;
      double mine = (j < whi) ? walk_elem(j) : 0.0;
      // inclusive prefix across lanes (deterministic shfl ladder)
      double pre = mine;
#pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        const double v = __shfl_up(pre, off);
        if (lane >= off) pre += v;
      }
      const double chunk_total = __shfl(pre, WAVE - 1);
      if (out_v != nullptr && run + chunk_total >= target) {
        // first lane whose running total crosses the target
        const bool crossed = (run + pre >= target) && j < whi;
        const unsigned long long mask = __ballot(crossed);
        if (mask != 0ull) {
          const int fl = __ffsll((long long)mask) - 1;
          const int32_t v = args.csr_col[cb + fl];
          *out_v = v;
          return run + chunk_total;
        }
      }
      run += chunk_total;
    }
    return run;
  };
  const double R = residual_pass(-1.0, nullptr);

  const double W = T1 + T2 + R;
  const double Zk = exp((double)args.log_pow_total[a * (args.Kc + 1) + k]);
  const double Wn = W / Zk;

  const ValueUniforms u = value_uniforms(args, p.elem);

  int v_new;
  if (u.u_mix < 1.0 / (1.0 + Wn) || W <= 0.0) {
    v_new = value_base_alias(args, p, k, u.u_a1, u.u_a2);
  } else {
    const double t = u.u_sel * W;
    if (t < T1) {
      v_new = prefix_pick(args.tab2_excl + (int64_t)(lb + m1) * args.nnz,
                          args.csr_col, lo1, hi1, t);
    } else if (t < T1 + T2) {
      v_new = prefix_pick(args.tab2_excl + (int64_t)(lb + m2) * args.nnz,
                          args.csr_col, lo2, hi2, t - T1);
    } else {
      int32_t sel = x1;
      residual_pass(t - T1 - T2, &sel);
      v_new = sel;
    }
  }
  if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)v_new;
}

__global__ void __launch_bounds__(WAVES_PER_BLOCK_VAL * WAVE)
value_update_kd2_kernel(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t widx = (int64_t)blockIdx.x * WAVES_PER_BLOCK_VAL + wave;
  const int64_t p0 = widx * 8;
  for (int64_t pair = p0; pair < p0 + 8 && pair < args.n_pairs; ++pair) {
    if (args.kobs[pair] >= 2) value_update_kd2_pair(args, pair, lane);
  }
}

constexpr int VAL_STRIDE = 8;  // pairs examined per wave in kobs mode

// One factor of a pair's perturbation: a distinct (value, file) group of
// observed records with its multiplicity, or a single record.
struct ValueUnit { int32_t x, m, f; };

// VMODE selects which k >= 2 perturbation path a kernel instantiation
// carries: 0 = both (explicit pair lists / tests), 1 = LDS-hash only,
// 2 = union-merge only. The split halves the register pressure of the hot
// kobs-mode kernels (the monolithic kernel sat at 118 VGPRs = 4 waves/SIMD).
template <int VMODE>
__device__ void value_update_pair(const ValueArgs& args, int64_t pair, int lane,
                                  int32_t* keys, float* vals, int32_t* gbuf,
                                  int64_t* glo, int32_t* gn, float* gse) {
  const ValuePair p = value_pair_of(args, pair);
  const int64_t e = p.e, v0 = p.v0;
  const int a = p.a, V = p.V;
  const bool is_const = p.is_const;
  const uint64_t elem = p.elem;

  // ---- gather observed linked records -------------------------------------
  const int64_t r_lo = args.ent_rec_ptr[e], r_hi = args.ent_rec_ptr[e + 1];
  int k_obs = 0;
  int64_t first_obs_r = -1;
  int32_t first_nondist = -1;  // first observed non-distorted value (record order)
  for (int64_t i = r_lo; i < r_hi; ++i) {
    const int64_t r = args.ent_rec_idx[i];
    const int32_t x = args.rec_values[r * args.A + a];
    if (x < 0) continue;
    if (k_obs == 0) first_obs_r = r;
    ++k_obs;
    if (!args.collapsed && first_nondist < 0 && !args.rec_dist[r * args.A + a])
      first_nondist = x;
  }

  // base distribution: cached alias tables, or the dense scan for k_obs > Kc
  auto base_draw = [&](uint32_t draw_tag) -> int {
    float u1, u2;
    philox_uniform2(args.seed, args.iteration, PH_VALM, elem, draw_tag, &u1, &u2);
    if (is_const || k_obs == 0 || k_obs <= args.Kc)
      return value_base_alias(args, p, k_obs, u1, u2);
    float dummy;
    return dense_power_draw(args, a, k_obs, elem, lane, &dummy);
  };

  // non-collapsed deterministic copy (GibbsUpdates.scala:619-630)
  if (value_settles_early(args, false, first_nondist >= 0)) {
    if (lane == 0) args.ent_values[e * args.A + a] = first_nondist;
    return;
  }

  if (k_obs == 0) {
    int v = base_draw(0xFFFF0000u);
    if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)v;
    return;
  }

  if (value_settles_early(args, is_const, false)) {  // no perturbation for const non-collapsed
    int v = base_draw(0xFFFF0000u);
    if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)v;
    return;
  }

  // log of normalized base probability of value v (local id); log Z for the
  // rare k > Kc case is computed on demand by a wave reduction.
  float log_z_rare = 0.0f;
  if (!is_const && k_obs > args.Kc) {
    double tot = 0.0;
    for (int64_t v = v0 + lane; v < v0 + V; v += WAVE)
      tot += exp((double)(args.log_phi[v] + (float)k_obs * args.log_norm[v]));
    log_z_rare = (float)log(wave_sum(tot));
  }
  const float log_z =
      is_const ? 0.0f
               : (k_obs <= args.Kc ? args.log_pow_total[a * (args.Kc + 1) + k_obs]
                                   : log_z_rare);
  auto log_base_prob = [&](int v_local) -> float {
    const int64_t v = v0 + v_local;
    if (is_const) return args.log_phi[v];
    return args.log_phi[v] + (float)k_obs * args.log_norm[v] - log_z;
  };
  auto finish = [&](double W, float best, long long best_v) {
    const float u = philox_uniform(args.seed, args.iteration, PH_VALM, elem, 0xFFFF0001u);
    int v_new;
    if ((double)u < 1.0 / (1.0 + W) || best_v < 0) {
      v_new = base_draw(0xFFFF0002u);
    } else {
      v_new = (int)best_v;
    }
    if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)v_new;
  };

  // ---- k == 1 fast path: the perturbation support is one sim row ----------
  // Its accumulation stays separate from value_accum: k = 1 log-weights are
  // bounded (~35), so it sums W with the f32 exp alone (~20x cheaper than
  // the software double exp) and takes log(e^s + se) without a multiplicity.
  if (k_obs == 1) {
    const int64_t r = first_obs_r;
    const int32_t x = args.rec_values[r * args.A + a];
    const float se =
        value_self_f32(args, p, x, args.collapsed ? args.rec_file[r] : 0);
    double W = 0.0;
    float best = -INFINITY;
    long long best_v = -1;
    if (is_const) {  // single support value {x}, factor = 1 + se
      if (lane == 0 && se > 0.0f) {
        const float L = __logf(1.0f + se);
        const float logw = log_base_prob(x) + L + __logf(1.0f - __expf(-L));
        W = (double)__expf(logw);
        best = 0.0f;
        best_v = x;
      }
      W = wave_sum(W);
      best_v = __shfl(best_v, 0);
    } else {
      const int64_t row_lo = args.csr_row_ptr[v0 + x], row_hi = args.csr_row_ptr[v0 + x + 1];
      for (int64_t jj = row_lo + lane; jj < row_hi; jj += WAVE) {
        const int32_t v = args.csr_col[jj];
        const float s = args.csr_sim[jj];
        const float L = (v == x && se > 0.0f) ? __logf(__expf(s) + se) : s;
        const float logw = log_base_prob(v) + L + __logf(1.0f - __expf(-L));
        W += (double)__expf(logw);
        const float g = gumbel_from_uniform(
            philox_uniform(args.seed, args.iteration, PH_VALG, elem, (uint32_t)v));
        if (logw + g > best) { best = logw + g; best_v = v; }
      }
      W = wave_sum(W);
      wave_argmax(best, best_v);
    }
    finish(W, best, best_v);
    return;
  }

  // ---- perturbation weights (k >= 2): grouped by distinct value ----------
  // A cluster's linked records mostly agree, so group them by distinct
  // (value, file): m records sharing x contribute the factor (e^s + se)^m,
  // i.e. one row pass with a multiplier instead of m passes — the union
  // support is sum of DISTINCT rows, not k rows. L_v = sum_g m_g log f_g(v);
  // final weight = base_prob(v) * (exp(L_v) - 1). More than VAL_DMAX
  // distinct groups (rare) falls back to per-record units.
  int d = 0;
  bool gover = false;
  if (lane == 0) {
    for (int64_t i = r_lo; i < r_hi; ++i) {
      const int64_t r = args.ent_rec_idx[i];
      const int32_t x = args.rec_values[r * args.A + a];
      if (x < 0) continue;
      const int32_t f = args.collapsed ? args.rec_file[r] : 0;
      int g = 0;
      for (; g < d; ++g)
        if (gbuf[g] == x && gbuf[VAL_DMAX + g] == f) break;
      if (g < d) {
        gbuf[2 * VAL_DMAX + g] += 1;
      } else if (d < VAL_DMAX) {
        gbuf[d] = x;
        gbuf[VAL_DMAX + d] = f;
        gbuf[2 * VAL_DMAX + d] = 1;
        ++d;
      } else {
        gover = true;
        break;
      }
    }
    gbuf[3 * VAL_DMAX] = gover ? -1 : d;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  gover = gbuf[3 * VAL_DMAX] < 0;
  d = gover ? 0 : gbuf[3 * VAL_DMAX];

  const int n_units = gover ? k_obs : d;
  // unit u: group u of gbuf, or (gover) the u-th observed record of the list
  auto unit_of = [&](int u) -> ValueUnit {
    if (!gover) return {gbuf[u], gbuf[2 * VAL_DMAX + u], gbuf[VAL_DMAX + u]};
    int seen = 0;
    for (int64_t i = r_lo; i < r_hi; ++i) {
      const int64_t r = args.ent_rec_idx[i];
      const int32_t xx = args.rec_values[r * args.A + a];
      if (xx < 0) continue;
      if (seen++ == u) return {xx, 1, args.collapsed ? args.rec_file[r] : 0};
    }
    return {0, 0, 0};  // not reached: u < k_obs
  };

  // size the table (and its clear/scan cost) to the actual support
  int64_t total_entries = 0;
  for (int u = 0; u < n_units; ++u) {
    total_entries += value_row_entries(args, p, unit_of(u).x);
  }
  const bool dense = value_is_dense(total_entries);
  if (VMODE == 1 && dense) return;   // the merge kernel's pair
  if (VMODE == 2 && !dense) return;  // the hash kernel's pair
  int tsize = 64;
  while (tsize < 2 * (int)total_entries && tsize < HASH_CAP) tsize <<= 1;
  if (args.stats != nullptr && lane == 0) {
    atomicAdd(&args.stats[0], 1ull);
    atomicAdd(&args.stats[dense ? 2 : 1], 1ull);
    atomicAdd(&args.stats[3], (unsigned long long)total_entries);
    atomicAdd(&args.stats[4], (unsigned long long)n_units);
    atomicAdd(&args.stats[5], (unsigned long long)k_obs);
    if (!is_const && k_obs > args.Kc) atomicAdd(&args.stats[6], 1ull);
    if (dense)
      atomicAdd(&args.stats[7], (unsigned long long)total_entries);
  }

  // single-(value, file) pairs with cached k-tables are the kd1 kernel's
  // (kobs mode only; explicit pair lists keep the full path)
  if (value_goes_kd1(args, is_const, gover, d, k_obs)) return;
  // two distinct VALUES with cached (k, m) tables: the kd2 kernel's
  if (d >= 2 && value_goes_kd2(args, is_const, gover, d, k_obs, gbuf[0], gbuf[1]))
    return;

  double W = 0.0;            // total perturbation weight
  float best = -INFINITY;    // gumbel-max over perturbation weights
  long long best_v = -1;

  if (VMODE != 2 && !dense) {
    lds_hash_clear(keys, vals, tsize, lane);
    const uint32_t mask = (uint32_t)(tsize - 1);
    // hash-accumulate log factors per unit
    for (int u = 0; u < n_units; ++u) {
      const ValueUnit un = unit_of(u);
      const float self_extra = value_self_f32(args, p, un.x, un.f);
      const float fm = (float)un.m;
      if (is_const) {
        // single-entry row {x}: factor = (1 + self_extra)^m
        if (lane == 0)
          lds_hash_add(keys, vals, mask, un.x, fm * __logf(1.0f + self_extra));
      } else {
        const int64_t row_lo = args.csr_row_ptr[v0 + un.x];
        const int64_t row_hi = args.csr_row_ptr[v0 + un.x + 1];
        for (int64_t j = row_lo + lane; j < row_hi; j += WAVE) {
          const int32_t v = args.csr_col[j];
          lds_hash_add(keys, vals, mask, v,
                       row_factor_log(v, un.x, args.csr_sim[j], fm, self_extra));
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    lds_hash_reduce(args, elem, keys, vals, tsize, lane, log_base_prob, W, best,
                    best_v);
  } else if (VMODE != 1 && !gover && !is_const && args.vchunk) {
    // chunked hash-accumulate (union too big for one LDS table): sweep the
    // d rows in ascending value-range chunks sized so each chunk's entries
    // fit the table, then run the same clear/insert/reduce as the small
    // path per chunk. Replaces the union-merge path's (d-1) dependent-load
    // binary searches PER ENTRY with one binary search per unit PER CHUNK.
    // L_v accumulation order per value (ascending unit) matches the small
    // path, so replay stays deterministic. Cursor = row_end - remaining:
    // glo holds the fixed row end, gn the mutable remaining count.
    if (lane == 0) {
      for (int u = 0; u < n_units; ++u) {
        const int32_t x2 = gbuf[u];
        const int64_t lo2 = args.csr_row_ptr[v0 + x2];
        glo[u] = args.csr_row_ptr[v0 + x2 + 1];
        gn[u] = (int32_t)(glo[u] - lo2);
        gse[u] = value_self_f32(args, p, x2, gbuf[VAL_DMAX + u]);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
    const int ccap = (HASH_CAP * 3) / 4;
    const int per_u = ccap / n_units > 0 ? ccap / n_units : 1;
    for (;;) {
      // chunk bound (exclusive): min over units of the value per_u entries
      // ahead of the cursor; every per-unit segment is then <= per_u
      int32_t vhi = INT32_MAX;
      bool any = false;
      for (int u = 0; u < n_units; ++u) {
        const int64_t end2 = glo[u];
        const int64_t cu = end2 - gn[u];
        if (cu < end2) any = true;
        if (cu + per_u < end2) {
          const int32_t cv = args.csr_col[cu + per_u];
          if (cv < vhi) vhi = cv;
        }
      }
      if (!any) break;
      lds_hash_clear(keys, vals, HASH_CAP, lane);
      for (int u = 0; u < n_units; ++u) {
        const int64_t end2 = glo[u];
        const int64_t cu = end2 - gn[u];
        const int64_t seg_end =
            (vhi == INT32_MAX) ? end2
                               : lower_bound_i32(args.csr_col, cu, end2, vhi);
        const int32_t ux = gbuf[u];
        const float self_extra = gse[u];
        const float fm = (float)gbuf[2 * VAL_DMAX + u];
        for (int64_t j = cu + lane; j < seg_end; j += WAVE) {
          const int32_t v = args.csr_col[j];
          lds_hash_add(keys, vals, HASH_CAP - 1, v,
                       row_factor_log(v, ux, args.csr_sim[j], fm, self_extra));
        }
        if (lane == 0) gn[u] = (int32_t)(end2 - seg_end);
        __builtin_amdgcn_wave_barrier();
      }
      lds_hash_reduce(args, elem, keys, vals, HASH_CAP, lane, log_base_prob, W,
                      best, best_v);
      // reads of this chunk's table must drain before the next chunk's clear
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_wave_barrier();
    }
  } else if (VMODE != 1) {
    // union-merge path (gover / const attrs): iterate every entry of every
    // DISTINCT row, but process a value only from the FIRST unit containing
    // it; full L_v comes from binary searches in the other units' rows.
    // Per-unit metadata (row bounds, the theta-dependent self term) is
    // hoisted into LDS once per pair — the entry loop touches ~10^2-10^3
    // values per unit and must not recompute it per (entry, unit).
    const bool hoist = !gover && !is_const;
    if (hoist && lane == 0) {
      for (int u = 0; u < n_units; ++u) {
        const int32_t x2 = gbuf[u];
        glo[u] = args.csr_row_ptr[v0 + x2];
        gn[u] = (int32_t)(args.csr_row_ptr[v0 + x2 + 1] - glo[u]);
        gse[u] = value_self_f32(args, p, x2, gbuf[VAL_DMAX + u]);
      }
    }
    // unit u2 as the entry loop needs it: the hoisted LDS copy, or (gover)
    // rebuilt from the record scan
    struct MergeUnit { int32_t x, m; float se; int64_t lo, hi; };
    auto merge_unit = [&](int u2) -> MergeUnit {
      if (hoist) {
        const int64_t lo2 = glo[u2];
        return {gbuf[u2], gbuf[2 * VAL_DMAX + u2], gse[u2], lo2, lo2 + gn[u2]};
      }
      const ValueUnit un = unit_of(u2);
      return {un.x, un.m, value_self_f32(args, p, un.x, un.f),
              args.csr_row_ptr[v0 + un.x], args.csr_row_ptr[v0 + un.x + 1]};
    };
    for (int u = 0; u < n_units; ++u) {
      const ValueUnit un = unit_of(u);
      const int32_t ux = un.x;
      if (is_const) {
        if (lane == 0) {
          bool first = true;
          for (int u2 = 0; u2 < u && first; ++u2)
            if (unit_of(u2).x == ux) first = false;  // only possible when gover
          if (first) {
            float L = 0.0f;
            for (int u2 = u; u2 < n_units; ++u2) {
              const ValueUnit o = unit_of(u2);
              if (o.x != ux) continue;
              L += (float)o.m * __logf(1.0f + value_self_f32(args, p, o.x, o.f));
            }
            if (L > 0.0f)
              value_accum(args, elem, ux, L, log_base_prob(ux), W, best, best_v);
          }
        }
        continue;
      }
      const int64_t row_lo = args.csr_row_ptr[v0 + ux];
      const int64_t row_hi = args.csr_row_ptr[v0 + ux + 1];
      for (int64_t j = row_lo + lane; j < row_hi; j += WAVE) {
        const int32_t v = args.csr_col[j];
        // one ascending pass fuses the dedupe test (an EARLIER unit's row
        // containing v means that unit owns the value) with the log-factor
        // accumulation: one binary search per (entry, unit) instead of two
        bool first = true;
        float L = 0.0f;
        for (int u2 = 0; u2 < n_units; ++u2) {
          const MergeUnit o = merge_unit(u2);
          float s2;
          if (u2 == u) {
            s2 = args.csr_sim[j];
          } else {
            const int64_t p2 = lower_bound_i32(args.csr_col, o.lo, o.hi, v);
            const bool found = p2 < o.hi && args.csr_col[p2] == v;
            if (found && u2 < u) { first = false; break; }
            s2 = found ? args.csr_sim[p2] : 0.0f;
          }
          // row_factor_log's two cases, each added to L in its own statement:
          // the compiler may contract either product with the sum, which
          // one shared select-then-add need not reproduce bit for bit
          if (v == o.x && o.se > 0.0f)
            L += (float)o.m * __logf(__expf(s2) + o.se);
          else if (s2 != 0.0f)
            L += (float)o.m * s2;
        }
        if (!first) continue;
        value_accum(args, elem, v, L, log_base_prob(v), W, best, best_v);
      }
    }
  }
  W = wave_sum(W);
  wave_argmax(best, best_v);

  // mixture between base and perturbation (GibbsUpdates.scala:593-597)
  finish(W, best, best_v);
}

template <int VMODE>
__global__ void __launch_bounds__(WAVES_PER_BLOCK_VAL * WAVE)
value_update_kernel_t(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  __shared__ int32_t h_key[WAVES_PER_BLOCK_VAL][HASH_CAP];
  __shared__ float h_val[WAVES_PER_BLOCK_VAL][HASH_CAP];
  __shared__ int32_t g_buf[WAVES_PER_BLOCK_VAL][3 * VAL_DMAX + 1];
  // merge-path per-unit hoists: (row_lo, row_len, se) per distinct group
  __shared__ int64_t g_lo[WAVES_PER_BLOCK_VAL][VAL_DMAX];
  __shared__ int32_t g_n[WAVES_PER_BLOCK_VAL][VAL_DMAX];
  __shared__ float g_se[WAVES_PER_BLOCK_VAL][VAL_DMAX];

  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t widx = (int64_t)blockIdx.x * WAVES_PER_BLOCK_VAL + wave;
  if (args.pair_list != nullptr) {
    if (widx >= args.n_pairs) return;
    value_update_pair<VMODE>(args, args.pair_list[widx], lane, h_key[wave],
                             h_val[wave], g_buf[wave], g_lo[wave], g_n[wave],
                             g_se[wave]);
  } else if (args.list_count != nullptr) {
    // list mode (VMODE 1 or 2): one wave per listed pair of this kernel, a
    // static grid striding over a list whose length is read from the device
    const bool merge = VMODE == 2;
    const int64_t n = args.list_count[merge ? 1 : 0];
    const int64_t n_waves = (int64_t)gridDim.x * WAVES_PER_BLOCK_VAL;
    for (int64_t j = widx; j < n; j += n_waves) {
      const int64_t pair = args.pair_lists[merge ? args.n_pairs - 1 - j : j];
      value_update_pair<VMODE>(args, pair, lane, h_key[wave], h_val[wave],
                               g_buf[wave], g_lo[wave], g_n[wave], g_se[wave]);
    }
  } else {
    // kobs self-selection: each wave examines VAL_STRIDE consecutive pairs
    // and runs the (rare) k >= 2 ones serially
    const int64_t p0 = widx * VAL_STRIDE;
    for (int64_t pair = p0; pair < p0 + VAL_STRIDE && pair < args.n_pairs; ++pair) {
      if (args.kobs[pair] >= 2)
        value_update_pair<VMODE>(args, pair, lane, h_key[wave], h_val[wave],
                                 g_buf[wave], g_lo[wave], g_n[wave], g_se[wave]);
    }
  }
}

// Brute-force dense value update (Gibbs-Sequential, GibbsUpdates.scala:652-698)
__global__ void value_update_seq_kernel(ValueArgs args) {
  ctrl_override(args.ctrl, args.seed, args.iteration);
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t pair = (int64_t)blockIdx.x * (blockDim.x / WAVE) + wave;
  if (pair >= args.n_pairs) return;
  const ValuePair p = value_pair_of(args, pair);
  const int64_t e = p.e, v0 = p.v0;
  const int a = p.a, V = p.V;
  const bool is_const = p.is_const;
  const uint64_t elem = p.elem;

  const int64_t r_lo = args.ent_rec_ptr[e], r_hi = args.ent_rec_ptr[e + 1];
  int k_obs = 0;
  int32_t first_nondist = -1;
  for (int64_t i = r_lo; i < r_hi; ++i) {
    const int64_t r = args.ent_rec_idx[i];
    const int32_t x = args.rec_values[r * args.A + a];
    if (x < 0) continue;
    ++k_obs;
    if (first_nondist < 0 && !args.rec_dist[r * args.A + a]) first_nondist = x;
  }
  if (first_nondist >= 0 && k_obs > 0) {
    if (lane == 0) args.ent_values[e * args.A + a] = first_nondist;
    return;
  }
  if (k_obs == 0 || is_const) {
    float u1, u2;
    philox_uniform2(args.seed, args.iteration, PH_VALM, elem, 0xFFFF0000u, &u1, &u2);
    int v = value_base_alias(args, p, 0, u1, u2);
    if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)v;
    return;
  }
  // dense scan: w(v) = phi(v) * prod_r [expsim(x_r, v) * norm(v) * phi(x_r)]
  float best = -INFINITY;
  long long best_v = 0;
  for (int v_local = lane; v_local < V; v_local += WAVE) {
    float lw = args.log_phi[v0 + v_local];
    for (int64_t i = r_lo; i < r_hi; ++i) {
      const int64_t r = args.ent_rec_idx[i];
      const int32_t x = args.rec_values[r * args.A + a];
      if (x < 0) continue;
      lw += sim_lookup(args.csr_row_ptr, args.csr_col, args.csr_sim, v0 + x, v_local) +
            args.log_norm[v0 + v_local] + args.log_phi[v0 + x];
    }
    const float g = gumbel_from_uniform(
        philox_uniform(args.seed, args.iteration, PH_VALG, elem, (uint32_t)v_local));
    if (lw + g > best) { best = lw + g; best_v = v_local; }
  }
  wave_argmax(best, best_v);
  if (lane == 0) args.ent_values[e * args.A + a] = (int32_t)best_v;
}

// ---------------------------------------------------------------------------
// K7 (+K8): distortion update, with the log-likelihood reduction fused in.
// The distorted-record likelihood terms depend on exactly the data this
// kernel just touched (x, y, z), and the entity prior terms ride along as
// extra leading indices — fusing removes a second full pass over the state
// (summary_loglik_kernel remains for the standalone initial summary).
// ---------------------------------------------------------------------------

__global__ void distortion_update_kernel(
    const int32_t* __restrict__ rec_values, uint8_t* __restrict__ rec_dist,
    const int32_t* __restrict__ rec_file, const int64_t* __restrict__ rec_gid,
    const int64_t* __restrict__ rec_ent, const int32_t* __restrict__ ent_values,
    const float* __restrict__ theta, const float* __restrict__ phi,
    const float* __restrict__ norm_lin, const float* __restrict__ self_expsim,
    const int64_t* __restrict__ voff, const uint8_t* __restrict__ attr_const,
    int64_t R, int A, int F, uint64_t seed, uint32_t iteration,
    const int64_t* __restrict__ ctrl,
    const float* __restrict__ log_phi, const float* __restrict__ log_norm,
    const int64_t* __restrict__ csr_row_ptr, const int32_t* __restrict__ csr_col,
    const float* __restrict__ csr_sim,
    int64_t E,                      // entity prior rows (0 when not fusing)
    double* __restrict__ loglik) {  // nullptr = distortion only
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  ctrl_override(ctrl, seed, iteration);
  double contrib = 0.0;
  if (idx < E * A) {
    const int64_t e = idx / A;
    const int a = (int)(idx % A);
    contrib = (double)log_phi[voff[a] + ent_values[e * A + a]];
  } else if (idx < (E + R) * A) {
    const int64_t j = idx - E * A;
    const int64_t r = j / A;
    const int a = (int)(j % A);
    const int32_t x = rec_values[j];
    const float th = theta[a * F + rec_file[r]];
    const float u = philox_uniform(seed, iteration, PH_DIST,
                                   (uint64_t)rec_gid[r] * 32u + (uint64_t)a, 0);
    uint8_t z;
    if (x < 0) {
      z = u < th;
    } else {
      const int32_t y = ent_values[rec_ent[r] * A + a];
      if (x == y) {
        float pr1 = th * phi[voff[a] + x];
        if (!attr_const[a]) pr1 *= norm_lin[voff[a] + x] * self_expsim[voff[a] + x];
        const float pr0 = 1.0f - th;
        const float psum = pr0 + pr1;
        const float pz = psum != 0.0f ? pr1 / psum : 0.0f;
        z = u < pz;
      } else {
        z = 1;
      }
    }
    rec_dist[j] = z;
    if (loglik != nullptr && z && x >= 0) {
      float lp = log_phi[voff[a] + x];
      if (!attr_const[a]) {
        const int32_t y = ent_values[rec_ent[r] * A + a];
        lp += log_norm[voff[a] + y] +
              sim_lookup(csr_row_ptr, csr_col, csr_sim, voff[a] + x, y);
      }
      contrib = (double)lp;
    }
  }
  if (loglik == nullptr) return;
  // wave shuffle reduce, then cross-wave LDS, one atomic per block
  for (int off = WAVE / 2; off > 0; off >>= 1)
    contrib += __shfl_down(contrib, off, WAVE);
  __shared__ double wsum[256 / WAVE];
  const int wid = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) wsum[wid] = contrib;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    const int nw = (int)(blockDim.x / WAVE);
    for (int i = 0; i < nw; ++i) s += wsum[i];
    // spread over 256 slots: every block adding one global f64 serializes
    // (~10 ns per same-address atomic x tens of thousands of blocks)
    if (s != 0.0) atomicAdd(&loglik[blockIdx.x & 255], s);
  }
}

// ---------------------------------------------------------------------------
// K8: log-likelihood reduction (entity priors + distorted record terms)
// ---------------------------------------------------------------------------

__global__ void summary_loglik_kernel(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ rec_values,
    const uint8_t* __restrict__ rec_dist, const int64_t* __restrict__ rec_ent,
    const float* __restrict__ log_phi, const float* __restrict__ log_norm,
    const int64_t* __restrict__ voff, const int64_t* __restrict__ csr_row_ptr,
    const int32_t* __restrict__ csr_col, const float* __restrict__ csr_sim,
    const uint8_t* __restrict__ attr_const, int64_t E, int64_t R, int A,
    double* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t total = (E + R) * A;
  double contrib = 0.0;
  if (idx < E * A) {
    const int64_t e = idx / A;
    const int a = (int)(idx % A);
    contrib = (double)log_phi[voff[a] + ent_values[e * A + a]];
  } else if (idx < total) {
    const int64_t j = idx - E * A;
    const int64_t r = j / A;
    const int a = (int)(j % A);
    if (rec_dist[r * A + a]) {
      const int32_t x = rec_values[r * A + a];
      if (x >= 0) {
        float lp = log_phi[voff[a] + x];
        if (!attr_const[a]) {
          const int32_t y = ent_values[rec_ent[r] * A + a];
          lp += log_norm[voff[a] + y] +
                sim_lookup(csr_row_ptr, csr_col, csr_sim, voff[a] + x, y);
        }
        contrib = (double)lp;
      }
    }
  }
  // block reduce then one atomic per block
  __shared__ double partial[256];
  partial[threadIdx.x] = contrib;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) partial[threadIdx.x] += partial[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(&out[blockIdx.x & 255], partial[0]);
}

// ---------------------------------------------------------------------------
// Fused support kernels (small-problem launch-count reduction)
// ---------------------------------------------------------------------------

// Build inverted-index sort keys for entities and query keys for records in
// one launch: key = (part * A + a) * Vmax + value (a-major for entities).
__global__ void build_keys_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1,   // [NP] first attr of pseudo slot
    const int32_t* __restrict__ pair_a2,   // [NP] second attr
    const int32_t* __restrict__ pair_v2,   // [NP] domain size of second attr
    int64_t E, int64_t R, int A, int NP, int64_t Vmax,
    int64_t* __restrict__ ekeys,   // [(A+NP) * E] slot-major
    int64_t* __restrict__ qkeys) { // [R * (A+NP)]
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int T = A + NP;
  if (idx < E * T) {
    const int t = (int)(idx / E);
    const int64_t e = idx % E;
    int64_t v;
    if (t < A) {
      v = ent_values[e * A + t];
    } else {
      // composite value of a constant-attribute pair
      v = (int64_t)ent_values[e * A + pair_a1[t - A]] * pair_v2[t - A]
          + ent_values[e * A + pair_a2[t - A]];
    }
    ekeys[idx] = ((int64_t)ent_part[e] * T + t) * Vmax + v;
  } else if (idx < E * T + R * T) {
    const int64_t j = idx - E * T;
    const int64_t r = j / T;
    const int t = (int)(j % T);
    int64_t v;
    if (t < A) {
      const int32_t x = rec_values[r * A + t];
      v = x < 0 ? 0 : x;
    } else {
      const int32_t x1 = rec_values[r * A + pair_a1[t - A]];
      const int32_t x2 = rec_values[r * A + pair_a2[t - A]];
      v = (x1 < 0 || x2 < 0) ? 0 : (int64_t)x1 * pair_v2[t - A] + x2;
    }
    qkeys[j] = ((int64_t)rec_part[r] * T + t) * Vmax + v;
  }
}

// ---------------------------------------------------------------------------
// Counting-sort inverted index (replaces radix sort + batched searchsorted):
//   1. postings_hist_kernel:    counts[key] += 1 over all (entity, slot)
//   2. exclusive prefix (torch.cumsum, host-issued) -> dense ptr over keys
//   3. postings_scatter_kernel: postings[cursor[key]++] = entity
//   4. cand_ranges_kernel:      per (record, slot) lo = ptr[key], hi = ptr[key+1]
// Posting order within one key is arbitrary (atomic cursors): the link
// kernels only ENUMERATE a posting range — membership tests are direct
// entity-value comparisons and the Gumbel-max draw is keyed by entity id,
// so the sampled distribution is order-independent.
// Key layout matches build_keys_kernel: (part * T + t) * Vmax + v.
// ---------------------------------------------------------------------------

DBL_D int64_t posting_slot_value(const int32_t* vals, int64_t row, int A, int t,
                                 const int32_t* pair_a1, const int32_t* pair_a2,
                                 const int32_t* pair_v2) {
  if (t < A) return vals[row * A + t];
  return (int64_t)vals[row * A + pair_a1[t - A]] * pair_v2[t - A]
         + vals[row * A + pair_a2[t - A]];
}

// Popular values (low-cardinality constant attributes) would serialize tens
// of thousands of same-address global atomics, so both passes pre-aggregate
// duplicate keys in an LDS open-addressing hash per block: one global atomic
// per DISTINCT key per block. Keys fit int32 (the dense path is capped at
// 2^28 counters), so the table uses 32-bit LDS CAS.
constexpr int PB_THREADS = 1024;  // items per block == threads
constexpr int PB_TBL = 2048;      // >= 2x max distinct keys per block

DBL_D int pb_hash(int32_t key) {
  return (int)(((uint32_t)key * 2654435761u) >> 16) & (PB_TBL - 1);
}

// Histogram of block blockIdx.x's PB_THREADS (slot, entity) items.
DBL_D void postings_hist_block(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int32_t* __restrict__ counts) {
  __shared__ int32_t h_key[PB_TBL];
  __shared__ int32_t h_cnt[PB_TBL];
  for (int i = threadIdx.x; i < PB_TBL; i += blockDim.x) {
    h_key[i] = -1;
    h_cnt[i] = 0;
  }
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int T = A + NP;
  if (idx < E * T) {
    const int t = (int)(idx / E);
    const int64_t e = idx % E;
    const int64_t v = posting_slot_value(ent_values, e, A, t, pair_a1, pair_a2, pair_v2);
    const int32_t key = (int32_t)(((int64_t)ent_part[e] * T + t) * Vmax + v);
    int slot = pb_hash(key);
    for (;;) {
      const int32_t prev = atomicCAS(&h_key[slot], -1, key);
      if (prev == -1 || prev == key) {
        atomicAdd(&h_cnt[slot], 1);
        break;
      }
      slot = (slot + 1) & (PB_TBL - 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PB_TBL; i += blockDim.x)
    if (h_key[i] >= 0) atomicAdd(&counts[h_key[i]], h_cnt[i]);
}

__global__ __launch_bounds__(PB_THREADS) void postings_hist_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int32_t* __restrict__ counts) {
  postings_hist_block(ent_part, ent_values, pair_a1, pair_a2, pair_v2, E, A, NP, Vmax,
                      counts);
}

// Scatter of block blockIdx.x's PB_THREADS (slot, entity) items.
DBL_D void postings_scatter_block(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int32_t* __restrict__ cursor,        // [NK] initialized to exclusive prefix
    int32_t* __restrict__ postings) {    // [E * T]
  __shared__ int32_t h_key[PB_TBL];
  __shared__ int32_t h_cnt[PB_TBL];
  __shared__ int32_t h_base[PB_TBL];
  for (int i = threadIdx.x; i < PB_TBL; i += blockDim.x) {
    h_key[i] = -1;
    h_cnt[i] = 0;
  }
  __syncthreads();
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int T = A + NP;
  int my_slot = -1;
  int32_t my_rank = 0;
  int32_t e_out = 0;
  if (idx < E * T) {
    const int t = (int)(idx / E);
    const int64_t e = idx % E;
    e_out = (int32_t)e;
    const int64_t v = posting_slot_value(ent_values, e, A, t, pair_a1, pair_a2, pair_v2);
    const int32_t key = (int32_t)(((int64_t)ent_part[e] * T + t) * Vmax + v);
    int slot = pb_hash(key);
    for (;;) {
      const int32_t prev = atomicCAS(&h_key[slot], -1, key);
      if (prev == -1 || prev == key) {
        my_rank = atomicAdd(&h_cnt[slot], 1);
        my_slot = slot;
        break;
      }
      slot = (slot + 1) & (PB_TBL - 1);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < PB_TBL; i += blockDim.x)
    if (h_key[i] >= 0) h_base[i] = atomicAdd(&cursor[h_key[i]], h_cnt[i]);
  __syncthreads();
  if (my_slot >= 0) postings[h_base[my_slot] + my_rank] = e_out;
}

__global__ __launch_bounds__(PB_THREADS) void postings_scatter_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int32_t* __restrict__ cursor, int32_t* __restrict__ postings) {
  postings_scatter_block(ent_part, ent_values, pair_a1, pair_a2, pair_v2, E, A, NP,
                         Vmax, cursor, postings);
}

// One thread per record: route each record to one of three link paths.
//   mode 0 = wave scan (link_update_kernel)
//   mode 1 = thread scan (link_update_small_kernel, short candidate list)
//   mode 2 = hierarchical sampler (link_update_heavy_kernel): records whose
//            candidate set is a large partition slice — no observed
//            non-distorted attribute (pool = whole partition), or exactly one
//            with a big posting range (pool = that stable posting segment) —
//            where an exact scan would touch thousands of entities.
__global__ void classify_modes_kernel(
    const int32_t* __restrict__ rec_values, const uint8_t* __restrict__ rec_dist,
    const int32_t* __restrict__ rec_part, const int64_t* __restrict__ ent_ptr,
    const int64_t* __restrict__ cand_lo, const int64_t* __restrict__ cand_hi,
    int64_t R, int A, int NP, int64_t small_threshold, int64_t heavy_threshold,
    uint8_t* __restrict__ mode) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int T = A + NP;
  int64_t best = INT64_MAX;
  int nd_count = 0;
  for (int a = 0; a < A; ++a) {
    if (rec_values[r * A + a] < 0 || rec_dist[r * A + a]) continue;
    ++nd_count;
    const int64_t n = cand_hi[r * T + a] - cand_lo[r * T + a];
    if (n < best) best = n;
  }
  uint8_t m = 0;
  if (heavy_threshold > 0) {
    const int32_t p = rec_part[r];
    const int64_t pool = ent_ptr[p + 1] - ent_ptr[p];
    if (nd_count == 0 && pool > heavy_threshold) m = 2;
    else if (nd_count == 1 && best > heavy_threshold) m = 2;
  }
  if (m == 0 && best != INT64_MAX && best <= small_threshold) m = 1;
  mode[r] = m;
}

// Candidate range of record r's slot t off the dense key prefix.
DBL_D CandRange cand_range_of(
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, const int64_t* __restrict__ ptr,
    int A, int NP, int64_t Vmax, int64_t r, int t) {
  int64_t v;
  if (t < A) {
    v = rec_values[r * A + t];
  } else {
    const int32_t x1 = rec_values[r * A + pair_a1[t - A]];
    const int32_t x2 = rec_values[r * A + pair_a2[t - A]];
    v = (x1 < 0 || x2 < 0) ? -1 : (int64_t)x1 * pair_v2[t - A] + x2;
  }
  // missing value: empty range (never consulted as a constraint)
  if (v < 0) return {0, 0};
  const int64_t key = ((int64_t)rec_part[r] * (A + NP) + t) * Vmax + v;
  return {ptr[key], ptr[key + 1]};
}

// The same for (record, slot) item idx, stored.
DBL_D void cand_range_item(
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, const int64_t* __restrict__ ptr,
    int64_t R, int A, int NP, int64_t Vmax,
    int64_t* __restrict__ cand_lo, int64_t* __restrict__ cand_hi,  // [R * T]
    int64_t idx) {
  const int T = A + NP;
  if (idx >= R * T) return;
  const CandRange c = cand_range_of(rec_part, rec_values, pair_a1, pair_a2, pair_v2,
                                    ptr, A, NP, Vmax, idx / T, (int)(idx % T));
  cand_lo[idx] = c.lo;
  cand_hi[idx] = c.hi;
}

__global__ void cand_ranges_kernel(
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, const int64_t* __restrict__ ptr,
    int64_t R, int A, int NP, int64_t Vmax,
    int64_t* __restrict__ cand_lo, int64_t* __restrict__ cand_hi) {
  cand_range_item(rec_part, rec_values, pair_a1, pair_a2, pair_v2, ptr, R, A, NP,
                  Vmax, cand_lo, cand_hi,
                  (int64_t)blockIdx.x * blockDim.x + threadIdx.x);
}

// The posting scatter and the candidate ranges both need only the scanned
// prefix, so they share a launch: the first n_scatter blocks scatter, the
// rest take PB_THREADS (record, slot) items each. No block waits for another.
__global__ __launch_bounds__(PB_THREADS) void postings_scatter_ranges_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, const int64_t* __restrict__ ptr,
    int64_t E, int64_t R, int A, int NP, int64_t Vmax, unsigned n_scatter,
    int32_t* __restrict__ cursor, int32_t* __restrict__ postings,
    int64_t* __restrict__ cand_lo, int64_t* __restrict__ cand_hi) {
  if (blockIdx.x < n_scatter) {
    postings_scatter_block(ent_part, ent_values, pair_a1, pair_a2, pair_v2, E, A,
                           NP, Vmax, cursor, postings);
  } else {
    cand_range_item(rec_part, rec_values, pair_a1, pair_a2, pair_v2, ptr, R, A, NP,
                    Vmax, cand_lo, cand_hi,
                    (int64_t)(blockIdx.x - n_scatter) * PB_THREADS + threadIdx.x);
  }
}

// The same launch with the link phase's split list built in it: a range block
// takes one thread per record, writes the record's T ranges and appends the
// record to split_list when its base list (the one the link kernels will
// select) is longer than split_len. split_count must be zero on entry; the
// order within the list is arbitrary.
__global__ __launch_bounds__(PB_THREADS) void postings_scatter_ranges_split_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ rec_part, const int32_t* __restrict__ rec_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, const int64_t* __restrict__ ptr,
    int64_t E, int64_t R, int A, int NP, int64_t Vmax, unsigned n_scatter,
    int32_t* __restrict__ cursor, int32_t* __restrict__ postings,
    int64_t* __restrict__ cand_lo, int64_t* __restrict__ cand_hi,
    const uint8_t* __restrict__ rec_dist, const uint8_t* __restrict__ attr_const,
    const int64_t* __restrict__ ent_ptr, int64_t split_len,
    int32_t* __restrict__ split_list, int* __restrict__ split_count) {
  if (blockIdx.x < n_scatter) {
    postings_scatter_block(ent_part, ent_values, pair_a1, pair_a2, pair_v2, E, A,
                           NP, Vmax, cursor, postings);
    return;
  }
  const int64_t r = (int64_t)(blockIdx.x - n_scatter) * PB_THREADS + threadIdx.x;
  if (r >= R) return;
  const int T = A + NP;
  const auto range = [&](int t) {
    return cand_range_of(rec_part, rec_values, pair_a1, pair_a2, pair_v2, ptr, A, NP,
                         Vmax, r, t);
  };
  for (int t = 0; t < T; ++t) {
    const CandRange c = range(t);
    cand_lo[r * T + t] = c.lo;
    cand_hi[r * T + t] = c.hi;
  }
  const LinkMasks m = link_classify(rec_values, rec_dist, attr_const, r, A);
  const LinkBase base = link_select_base_from(range, pair_a1, pair_a2, NP, rec_part,
                                              ent_ptr, r, A, m.nd);
  if (base.n > split_len) split_list[atomicAdd(split_count, 1)] = (int32_t)r;
}

// Summary counts in one pass: per-record distortion histogram + per
// (attr, file) aggregates + isolate count (from the entity->record CSR).
// Item block `block` of blockDim.x entities-then-records; block_counts is the
// block's LDS staging of the n_counts counters.
DBL_D void summary_counts_block(
    const uint8_t* __restrict__ rec_dist, const int32_t* __restrict__ rec_file,
    const int64_t* __restrict__ ent_rec_ptr, int64_t E, int64_t R, int A, int F,
    int n_counts, int64_t block, unsigned int* block_counts,
    unsigned long long* __restrict__ counts) {  // [1 + A*F + A+1]: iso, agg, hist
  // stage all counters in LDS: one global atomic per counter per BLOCK
  // (per-element global atomics on ~12 counters serialize at ~11 ns each)
  for (int i = threadIdx.x; i < n_counts; i += blockDim.x) block_counts[i] = 0u;
  __syncthreads();

  const int64_t idx = block * blockDim.x + threadIdx.x;
  if (idx < E) {
    if (ent_rec_ptr[idx + 1] == ent_rec_ptr[idx]) atomicAdd(&block_counts[0], 1u);
  } else if (idx < E + R) {
    const int64_t r = idx - E;
    int nd = 0;
    const int f = rec_file[r];
    for (int a = 0; a < A; ++a) {
      if (rec_dist[r * A + a]) {
        ++nd;
        atomicAdd(&block_counts[1 + a * F + f], 1u);
      }
    }
    atomicAdd(&block_counts[1 + A * F + nd], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_counts; i += blockDim.x) {
    if (block_counts[i]) atomicAdd(&counts[i], (unsigned long long)block_counts[i]);
  }
}

__global__ void summary_counts_kernel(
    const uint8_t* __restrict__ rec_dist, const int32_t* __restrict__ rec_file,
    const int64_t* __restrict__ ent_rec_ptr, int64_t E, int64_t R, int A, int F,
    int n_counts, unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned int block_counts[];
  summary_counts_block(rec_dist, rec_file, ent_rec_ptr, E, R, A, F, n_counts,
                       blockIdx.x, block_counts, counts);
}

// Pack loglik + counts (+ the sweep's error count, so the host reads one
// buffer) into the f64 summary buffer. Item i of `stride` items in all; item
// 0 sums the 256 log-likelihood slots in index order (the sum is bitwise the
// same whoever runs it).
DBL_D void summary_finalize_items(
    const double* __restrict__ loglik, const unsigned long long* __restrict__ counts,
    int n_counts, const int* __restrict__ err,  // [1] or null
    int i, int stride,
    double* __restrict__ packed) {              // [1 + n_counts (+ 1 with err)]
  if (i == 0) {
    double s = 0.0;
    for (int j = 0; j < 256; ++j) s += loglik[j];
    packed[0] = s;
    if (err) packed[1 + n_counts] = (double)err[0];
  }
  for (int k = i; k < n_counts; k += stride) packed[1 + k] = (double)counts[k];
}

// (one tiny launch)
__global__ void summary_finalize_kernel(
    const double* __restrict__ loglik, const unsigned long long* __restrict__ counts,
    int n_counts, const int* __restrict__ err, double* __restrict__ packed) {
  summary_finalize_items(loglik, counts, n_counts, err,
                         (int)(blockIdx.x * blockDim.x + threadIdx.x),
                         (int)(gridDim.x * blockDim.x), packed);
}

// ---------------------------------------------------------------------------
// MFMA experiment: the most matrix-shaped hot computation is
// the dense categorical-agreement block of the PCG-II link weights —
// score[r, e] = sum_a bonus_a(x_{r,a}) * 1{x_{r,a} == y_{e,a}} over the
// constant attributes. Two implementations of the same R x E scorer:
//   scalar_score_bench: LDS-staged entity codes, wave-per-record compare/add
//   mfma_score_bench:   one-hot formulation U[r,k] * H[k,e] on the bf16
//                       matrix cores (mfma_f32_16x16x32_bf16, K padded to a
//                       multiple of 32), fragments synthesized on the fly
//                       from the compact codes (no dense one-hot in memory)
// The measured comparison lives in profiles/README.md.
// ---------------------------------------------------------------------------

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

DBL_D short f32_to_bf16(float f) {
  union { float f; uint32_t u; } c = {f};
  return (short)(c.u >> 16);  // truncate (bench precision is bf16 anyway)
}

// score tile per WAVE: 16 records x 16 entities, K-loop over one-hot domain
__global__ void mfma_score_kernel(
    const int32_t* __restrict__ rcode,   // [R, 3] concatenated-domain codes
    const float* __restrict__ rbonus,    // [R, 3] per-record attr bonuses
    const int32_t* __restrict__ ecode,   // [E, 3]
    int R, int E, int K,                 // K = padded one-hot width
    float* __restrict__ score) {         // [R, E]
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int tiles_e = E / 16;
  const int tile = blockIdx.x * (blockDim.x / WAVE) + wave;
  const int tr = tile / tiles_e, te = tile % tiles_e;
  if (tr * 16 >= R) return;

  // A: row i = lane & 15 (record), 8 elements at k = k0 + (lane>>4)*8 + j
  // B: col j = lane & 15 (entity), same k layout
  // C/D: col = lane & 15, row = (lane>>4)*4 + reg
  const int r = tr * 16 + (lane & 15);
  const int e = te * 16 + (lane & 15);
  int32_t rc0 = rcode[r * 3], rc1 = rcode[r * 3 + 1], rc2 = rcode[r * 3 + 2];
  float rb0 = rbonus[r * 3], rb1 = rbonus[r * 3 + 1], rb2 = rbonus[r * 3 + 2];
  int32_t ec0 = ecode[e * 3], ec1 = ecode[e * 3 + 1], ec2 = ecode[e * 3 + 2];

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32) {
    bf16x8 fa, fb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = k0 + (lane >> 4) * 8 + j;
      float av = (k == rc0) ? rb0 : (k == rc1) ? rb1 : (k == rc2) ? rb2 : 0.0f;
      fa[j] = f32_to_bf16(av);
      fb[j] = f32_to_bf16((k == ec0 || k == ec1 || k == ec2) ? 1.0f : 0.0f);
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
  }
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int row = (lane >> 4) * 4 + reg;
    score[(int64_t)(tr * 16 + row) * E + te * 16 + (lane & 15)] = acc[reg];
  }
}

// Wave-per-record scalar scorer over LDS-staged packed entity codes.
constexpr int SCALAR_ETILE = 1024;

__global__ void scalar_score_kernel(
    const int32_t* __restrict__ rcode, const float* __restrict__ rbonus,
    const int32_t* __restrict__ ecode, int R, int E,
    float* __restrict__ score) {
  __shared__ uint32_t epack[SCALAR_ETILE];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int r = blockIdx.x * (blockDim.x / WAVE) + wave;
  const uint32_t rc = r < R ? (uint32_t)(rcode[r * 3] | (rcode[r * 3 + 1] << 10)
                                         | (rcode[r * 3 + 2] << 20)) : 0u;
  const float b0 = r < R ? rbonus[r * 3] : 0.f;
  const float b1 = r < R ? rbonus[r * 3 + 1] : 0.f;
  const float b2 = r < R ? rbonus[r * 3 + 2] : 0.f;
  for (int e0 = 0; e0 < E; e0 += SCALAR_ETILE) {
    __syncthreads();
    for (int i = threadIdx.x; i < SCALAR_ETILE && e0 + i < E; i += blockDim.x)
      epack[i] = (uint32_t)(ecode[(e0 + i) * 3] | (ecode[(e0 + i) * 3 + 1] << 10)
                            | (ecode[(e0 + i) * 3 + 2] << 20));
    __syncthreads();
    if (r >= R) continue;
    for (int i = lane; i < SCALAR_ETILE && e0 + i < E; i += WAVE) {
      const uint32_t ec = epack[i];
      const uint32_t x = rc ^ ec;
      float s = 0.0f;
      if ((x & 0x3FFu) == 0) s += b0;
      if ((x & 0xFFC00u) == 0) s += b1;
      if ((x & 0x3FF00000u) == 0) s += b2;
      score[(int64_t)r * E + e0 + i] = s;
    }
  }
}

void mfma_score_bench(torch::Tensor rcode, torch::Tensor rbonus,
                      torch::Tensor ecode, int64_t K, torch::Tensor score) {
  const int R = (int)rcode.size(0), E = (int)ecode.size(0);
  const int tiles = (R / 16) * (E / 16);
  hipLaunchKernelGGL(mfma_score_kernel, dim3((tiles + 3) / 4), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     rcode.data_ptr<int32_t>(), rbonus.data_ptr<float>(),
                     ecode.data_ptr<int32_t>(), R, E, (int)K,
                     score.data_ptr<float>());
}

void scalar_score_bench(torch::Tensor rcode, torch::Tensor rbonus,
                        torch::Tensor ecode, torch::Tensor score) {
  const int R = (int)rcode.size(0), E = (int)ecode.size(0);
  hipLaunchKernelGGL(scalar_score_kernel, dim3((R + 3) / 4), dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     rcode.data_ptr<int32_t>(), rbonus.data_ptr<float>(),
                     ecode.data_ptr<int32_t>(), R, E, score.data_ptr<float>());
}

// ---------------------------------------------------------------------------
// K9a: KD-tree descent (flat tree, partitioning.py as_flat layout)
// ---------------------------------------------------------------------------

// Leaf partition id of entity e.
DBL_D int32_t kd_leaf(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ node_kind,
    const int32_t* __restrict__ node_attr, const int32_t* __restrict__ node_a,
    const int32_t* __restrict__ node_b, const int32_t* __restrict__ rset,
    int64_t e, int A) {
  int nid = 0;
  while (node_kind[nid] != 0) {
    const int a = node_attr[nid];
    const int32_t v = ent_values[e * A + a];
    bool right;
    if (node_kind[nid] == 1) {
      right = v > node_a[nid];
    } else {
      const int lo = node_a[nid], n = node_b[nid];
      right = contains_i32(rset, lo, lo + n, v);
    }
    nid = 2 * nid + (right ? 2 : 1);
  }
  return node_a[nid];
}

__global__ void kd_descent_kernel(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ node_kind,
    const int32_t* __restrict__ node_attr, const int32_t* __restrict__ node_a,
    const int32_t* __restrict__ node_b, const int32_t* __restrict__ rset,
    int64_t E, int A, int32_t* __restrict__ ent_part_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  ent_part_out[e] =
      kd_leaf(ent_values, node_kind, node_attr, node_a, node_b, rset, e, A);
}

// ---------------------------------------------------------------------------
// Sweep glue: the integer bookkeeping between the sampling kernels, as plain
// launches over persistent buffers (no allocation, no stream workspace, so
// all of it is hipGraph-safe). Every output equals, element for element, the
// torch expression it stands in for (gpu_engine.py keeps those as the
// DBLINK_FUSED_GLUE=0 arm):
//   scan_excl_kernel     exclusive prefix of int32 counts -> int64 ptr[n+1]
//                        (+ an int32 cursor copy), one block
//   csr_count / _scatter / _order
//                        entity -> records CSR in stable order (= stable sort
//                        of rec_ent) with the kobs counts taken in the count
//                        pass
//   resort_hist / _scatter / _remap
//                        KD descent + stable counting sort of the entities by
//                        partition id (= stable argsort of ent_part), and the
//                        record remap through the inverse permutation
// Launches that read nothing of each other share a launch on the single-rank
// path, whole blocks routed by block index (no block waits for another):
//   sweep_begin_kernel   posting histogram + counter-block fill + staging copy
//   resort_hist_counts / resort_scan_scatter / resort_remap_finalize
//                        the re-sort with the summary counts and pack riding
//                        in its first and last launch, and the scan of the
//                        tile histograms in the scatter's prologue
// ---------------------------------------------------------------------------
constexpr int GL_THREADS = 1024;  // block (= entity tile) of the scan and re-sort
constexpr int GL_WAVES = GL_THREADS / WAVE;
// partitions the re-sort ranks in LDS (GL_WAVES * 256 * 4 B = 16 KiB); above
// it the engine keeps the torch argsort path
constexpr int RESORT_MAX_PARTS = 256;
// single-block scans stay cheaper than the two-kernel device scan up to about
// this many counters (32 tiles of 4096); above it launchers call cumsum
constexpr int64_t SCAN_SINGLE_MAX = 1 << 17;
constexpr int CSR_SERIAL_SEG = 32;  // longest segment one thread orders alone

// One thread's four consecutive counters of a tile. All of the scan's traffic
// goes through ONE compute unit, so it has to be coalesced: with 16-byte
// aligned buffers (vec) a thread moves its four counters as one 16-byte load
// and its results as 16-byte stores; otherwise element by element.
DBL_D void scan_load4(const int32_t* __restrict__ counts, int64_t i0, int64_t n,
                      bool vec, int32_t (&c)[4]) {
  if (vec && i0 + 4 <= n) {
    const int4 v = *reinterpret_cast<const int4*>(counts + i0);
    c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = (i0 + j < n) ? counts[i0 + j] : 0;
  }
}

// Zeros over one thread's four counters (same access shape as scan_load4).
DBL_D void scan_clear4(int32_t* __restrict__ counts, int64_t i0, int64_t n, bool vec) {
  if (vec && i0 + 4 <= n) {
    *reinterpret_cast<int4*>(counts + i0) = make_int4(0, 0, 0, 0);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i0 + j < n) counts[i0 + j] = 0;
  }
}

// With `clear` the counters are zeroed once they have been scanned: the next
// histogram accumulates into a clean buffer without a fill launch of its own.
__global__ __launch_bounds__(GL_THREADS) void scan_excl_kernel(
    int32_t* __restrict__ counts, int64_t n,
    int64_t* __restrict__ ptr,       // [n + 1]
    int32_t* __restrict__ cursor,    // [n] copy of ptr[:n], or null
    bool vec,                        // all three buffers 16-byte aligned
    bool clear) {                    // store zeros back over counts
  __shared__ int64_t wave_tot[GL_WAVES];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  constexpr int64_t TILE = GL_THREADS * 4;
  int64_t carry = 0;
  int32_t c[4], c_next[4];
  scan_load4(counts, (int64_t)threadIdx.x * 4, n, vec, c_next);
  for (int64_t base = 0; base < n; base += TILE) {
    const int64_t i0 = base + (int64_t)threadIdx.x * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = c_next[j];
    // the next tile's loads fly while this one is scanned
    if (base + TILE < n) scan_load4(counts, i0 + TILE, n, vec, c_next);
    const int64_t mine = (int64_t)c[0] + c[1] + c[2] + c[3];
    int64_t inc = mine;  // inclusive scan across the wave
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const int64_t o = __shfl_up(inc, off);
      if (lane >= off) inc += o;
    }
    if (lane == WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    int64_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < GL_WAVES; ++w) {
      const int64_t t = wave_tot[w];
      if (w < wave) before += t;
      total += t;
    }
    const int64_t x0 = carry + before + inc - mine;
    const int64_t x1 = x0 + c[0], x2 = x1 + c[1], x3 = x2 + c[2];
    if (vec && i0 + 4 <= n) {
      longlong2* p2 = reinterpret_cast<longlong2*>(ptr + i0);
      p2[0] = make_longlong2(x0, x1);
      p2[1] = make_longlong2(x2, x3);
      if (cursor)
        *reinterpret_cast<int4*>(cursor + i0) =
            make_int4((int32_t)x0, (int32_t)x1, (int32_t)x2, (int32_t)x3);
    } else {
      const int64_t x[4] = {x0, x1, x2, x3};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (i0 + j < n) {
          ptr[i0 + j] = x[j];
          if (cursor) cursor[i0 + j] = (int32_t)x[j];
        }
      }
    }
    carry += total;
    __syncthreads();  // wave_tot is rewritten by the next tile
  }
  if (threadIdx.x == 0) ptr[n] = carry;
  // every thread zeroes exactly the counters it loaded, after the last wait
  // of the scan, so the stores only have to drain by the kernel's end
  if (clear)
    for (int64_t base = 0; base < n; base += TILE)
      scan_clear4(counts, base + (int64_t)threadIdx.x * 4, n, vec);
}

// Sweep head: three jobs that read nothing of each other, routed by block
// index. Blocks [0, n_hist) build the posting histogram; block n_hist copies
// the sweep's host inputs ({seed, iteration} and theta) from their pinned
// host staging words, which the device reads through the same pointer; the
// blocks after it zero the sweep's counter block, four words a thread.
__global__ __launch_bounds__(PB_THREADS) void sweep_begin_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int32_t* __restrict__ counts, unsigned n_hist,
    int32_t* __restrict__ zero_blk, int64_t zero_n, bool zero_vec,
    const uint32_t* __restrict__ stage_pin, uint32_t* __restrict__ stage,
    int stage_words) {
  if (blockIdx.x < n_hist) {
    postings_hist_block(ent_part, ent_values, pair_a1, pair_a2, pair_v2, E, A, NP,
                        Vmax, counts);
  } else if (blockIdx.x == n_hist) {
    for (int i = threadIdx.x; i < stage_words; i += PB_THREADS) stage[i] = stage_pin[i];
  } else {
    scan_clear4(zero_blk,
                ((int64_t)(blockIdx.x - n_hist - 1) * PB_THREADS + threadIdx.x) * 4,
                zero_n, zero_vec);
  }
}

// Count pass: records per entity, observed values per (entity, attribute),
// and the store of the new links into the state's rec_ent.
__global__ void csr_count_kernel(
    const int64_t* __restrict__ rec_ent_new, const int32_t* __restrict__ rec_values,
    int64_t R, int A,
    int64_t* __restrict__ rec_ent,    // [R] state copy of the links, or null
    int32_t* __restrict__ ent_cnt,    // [E] zeroed
    int32_t* __restrict__ kobs) {     // [E * A] zeroed
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t e = rec_ent_new[r];
  if (rec_ent) rec_ent[r] = e;
  atomicAdd(&ent_cnt[e], 1);
  for (int a = 0; a < A; ++a)
    if (rec_values[r * A + a] >= 0) atomicAdd(&kobs[e * A + a], 1);
}

// Scatter pass: each record takes a slot of its entity's segment by counting
// ent_cnt back down (order within a segment is arbitrary until csr_order).
// Leaves ent_cnt all zero.
__global__ void csr_scatter_kernel(
    const int64_t* __restrict__ rec_ent, const int64_t* __restrict__ ent_rec_ptr,
    int64_t R, int32_t* __restrict__ ent_cnt, int64_t* __restrict__ ent_rec_idx) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int64_t e = rec_ent[r];
  const int32_t k = atomicSub(&ent_cnt[e], 1);
  ent_rec_idx[ent_rec_ptr[e] + k - 1] = r;
}

// Order pass: ascending record index within every segment. One thread sorts
// a short segment in place; a segment longer than CSR_SERIAL_SEG is rebuilt
// by its block as an ordered compaction over all records (O(R) per such
// entity: correct at any length, meant for the rare oversized cluster).
constexpr int CSR_ORDER_THREADS = 256;

__global__ __launch_bounds__(CSR_ORDER_THREADS) void csr_order_kernel(
    const int64_t* __restrict__ rec_ent, const int64_t* __restrict__ ent_rec_ptr,
    int64_t E, int64_t R, int64_t* ent_rec_idx) {
  __shared__ int32_t n_long;
  __shared__ int64_t long_ent[CSR_ORDER_THREADS];
  __shared__ int32_t wave_cnt[CSR_ORDER_THREADS / WAVE];
  if (threadIdx.x == 0) n_long = 0;
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < E) {
    const int64_t lo = ent_rec_ptr[e];
    const int64_t len = ent_rec_ptr[e + 1] - lo;
    if (len > CSR_SERIAL_SEG) {
      long_ent[atomicAdd(&n_long, 1)] = e;
    } else {
      for (int64_t i = 1; i < len; ++i) {  // insertion sort
        const int64_t v = ent_rec_idx[lo + i];
        int64_t j = i;
        while (j > 0 && ent_rec_idx[lo + j - 1] > v) {
          ent_rec_idx[lo + j] = ent_rec_idx[lo + j - 1];
          --j;
        }
        ent_rec_idx[lo + j] = v;
      }
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int nl = n_long;
  for (int k = 0; k < nl; ++k) {
    const int64_t le = long_ent[k];
    int64_t out = ent_rec_ptr[le];
    for (int64_t base = 0; base < R; base += CSR_ORDER_THREADS) {
      const int64_t r = base + threadIdx.x;
      const bool hit = r < R && rec_ent[r] == le;
      const unsigned long long m = __ballot(hit);
      if (lane == 0) wave_cnt[wave] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w = 0; w < CSR_ORDER_THREADS / WAVE; ++w) {
        const int t = wave_cnt[w];
        if (w < wave) before += t;
        total += t;
      }
      if (hit)
        ent_rec_idx[out + before + __popcll(m & ((1ull << lane) - 1ull))] = r;
      out += total;
      __syncthreads();  // wave_cnt is rewritten by the next tile
    }
  }
}

// Re-sort pass 1: KD descent of one tile of GL_THREADS entities and the
// tile's partition histogram, stored partition-major so one flat exclusive
// scan gives every (partition, tile) its first output slot.
// Tile blockIdx.x; h is the block's LDS table of P counters.
DBL_D void resort_hist_block(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ node_kind,
    const int32_t* __restrict__ node_attr, const int32_t* __restrict__ node_a,
    const int32_t* __restrict__ node_b, const int32_t* __restrict__ rset,
    int64_t E, int A, int P, int64_t n_tiles, int32_t* h,
    int32_t* __restrict__ ent_part_new,  // [E] unsorted new partition ids
    int32_t* __restrict__ hist) {        // [P * n_tiles]
  for (int i = threadIdx.x; i < P; i += GL_THREADS) h[i] = 0;
  __syncthreads();
  const int64_t e = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x;
  if (e < E) {
    const int32_t p =
        kd_leaf(ent_values, node_kind, node_attr, node_a, node_b, rset, e, A);
    ent_part_new[e] = p;
    // the launcher's caller checks every leaf id against P; the guard keeps
    // a bad tree from writing outside the table
    if ((uint32_t)p < (uint32_t)P) atomicAdd(&h[p], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < P; i += GL_THREADS)
    hist[(int64_t)i * n_tiles + blockIdx.x] = h[i];
}

__global__ __launch_bounds__(GL_THREADS) void resort_hist_kernel(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ node_kind,
    const int32_t* __restrict__ node_attr, const int32_t* __restrict__ node_a,
    const int32_t* __restrict__ node_b, const int32_t* __restrict__ rset,
    int64_t E, int A, int P, int64_t n_tiles,
    int32_t* __restrict__ ent_part_new, int32_t* __restrict__ hist) {
  __shared__ int32_t h[RESORT_MAX_PARTS];
  resort_hist_block(ent_values, node_kind, node_attr, node_a, node_b, rset, E, A, P,
                    n_tiles, h, ent_part_new, hist);
}

// Sweep tail, launch 1: the re-sort's tile histograms (blocks [0, n_tiles))
// and the summary counts (the blocks after them), which read nothing the
// re-sort writes. The two bodies share the block's LDS table.
__global__ __launch_bounds__(GL_THREADS) void resort_hist_counts_kernel(
    const int32_t* __restrict__ ent_values, const int32_t* __restrict__ node_kind,
    const int32_t* __restrict__ node_attr, const int32_t* __restrict__ node_a,
    const int32_t* __restrict__ node_b, const int32_t* __restrict__ rset,
    int64_t E, int A, int P, int64_t n_tiles,
    int32_t* __restrict__ ent_part_new, int32_t* __restrict__ hist,
    const uint8_t* __restrict__ rec_dist, const int32_t* __restrict__ rec_file,
    const int64_t* __restrict__ ent_rec_ptr, int64_t R, int F, int n_counts,
    unsigned long long* __restrict__ counts) {
  extern __shared__ unsigned int tail_lds[];  // max(P, n_counts) words
  if ((int64_t)blockIdx.x < n_tiles) {
    resort_hist_block(ent_values, node_kind, node_attr, node_a, node_b, rset, E, A, P,
                      n_tiles, reinterpret_cast<int32_t*>(tail_lds), ent_part_new,
                      hist);
  } else {
    summary_counts_block(rec_dist, rec_file, ent_rec_ptr, E, R, A, F, n_counts,
                         (int64_t)blockIdx.x - n_tiles, tail_lds, counts);
  }
}

// The scatter computes the scan of hist itself while it fits one tile of the
// scan (RESORT_SCAN_MAX counters): every block repeats the few-KiB prefix in
// LDS instead of waiting on a one-block launch for it.
constexpr int RESORT_SCAN_MAX = GL_THREADS * 4;

// Re-sort pass 2 (after the scan of hist, or with PROLOGUE doing that scan):
// stable scatter. An entity's slot is its (partition, tile) base +
// same-partition entities of earlier waves in the tile + earlier lanes of its
// wave, i.e. entity order within a partition is kept. Also emits the next
// sweep's partition offsets. With PROLOGUE tile_base is an output, stored by
// block 0 exactly as scan_excl would (the counters sum to at most E, so the
// prefix is exact in int32).
template <bool PROLOGUE>
DBL_D void resort_scatter_block(
    const int32_t* __restrict__ ent_part_new, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ hist,  // [P * n_tiles] (PROLOGUE only)
    bool vec,                          // hist 16-byte aligned
    int64_t* tile_base,                // [P * n_tiles + 1] scanned hist
    int64_t E, int A, int P, int64_t n_tiles,
    int32_t* __restrict__ out_part,     // [E]
    int32_t* __restrict__ out_values,   // [E, A]
    int32_t* __restrict__ inv,          // [E] old index -> new index
    int64_t* __restrict__ ent_ptr) {    // [P + 1]
  __shared__ int32_t wave_cnt[GL_WAVES * RESORT_MAX_PARTS];
  __shared__ int32_t base[PROLOGUE ? RESORT_SCAN_MAX : 1];
  __shared__ int32_t wave_tot[GL_WAVES];
  for (int i = threadIdx.x; i < GL_WAVES * P; i += GL_THREADS) wave_cnt[i] = 0;
  if (PROLOGUE) {
    const int64_t n = (int64_t)P * n_tiles;  // <= RESORT_SCAN_MAX
    const int64_t i0 = (int64_t)threadIdx.x * 4;
    int32_t c[4];
    scan_load4(hist, i0, n, vec, c);
    const int32_t mine = c[0] + c[1] + c[2] + c[3];
    int32_t inc = mine;  // inclusive scan across the wave
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      const int32_t o = __shfl_up(inc, off);
      if ((int)(threadIdx.x & (WAVE - 1)) >= off) inc += o;
    }
    if ((threadIdx.x & (WAVE - 1)) == WAVE - 1) wave_tot[threadIdx.x / WAVE] = inc;
    __syncthreads();
    int32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < GL_WAVES; ++w) {
      const int32_t t = wave_tot[w];
      if (w < (int)(threadIdx.x / WAVE)) before += t;
      total += t;
    }
    int32_t x[4];
    x[0] = before + inc - mine;
    x[1] = x[0] + c[0];
    x[2] = x[1] + c[1];
    x[3] = x[2] + c[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) base[i0 + j] = x[j];
    if (blockIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (i0 + j < n) tile_base[i0 + j] = x[j];
      if (threadIdx.x == 0) tile_base[n] = total;
    }
  }
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t e = (int64_t)blockIdx.x * GL_THREADS + threadIdx.x;
  int32_t p = e < E ? ent_part_new[e] : -1;
  if ((uint32_t)p >= (uint32_t)P) p = -1;  // see resort_hist_kernel
  int rank = 0;
  unsigned long long pending = __ballot(p >= 0);
  while (pending) {  // one round per distinct partition in the wave
    const int leader = __ffsll((long long)pending) - 1;
    const int32_t lp = __shfl(p, leader);
    const unsigned long long m = __ballot(p == lp);
    if (p == lp) rank = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == leader) wave_cnt[wave * P + lp] = __popcll(m);
    pending &= ~m;
  }
  __syncthreads();
  if (p >= 0) {
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wave_cnt[w * P + p];
    const int64_t slot = (int64_t)p * n_tiles + blockIdx.x;
    const int64_t dst = (PROLOGUE ? (int64_t)base[slot] : tile_base[slot]) + before + rank;
    out_part[dst] = p;
    for (int a = 0; a < A; ++a) out_values[dst * A + a] = ent_values[e * A + a];
    inv[e] = (int32_t)dst;
  }
  if (blockIdx.x == 0 && threadIdx.x <= P) {
    const int64_t first = (int64_t)threadIdx.x * n_tiles;
    ent_ptr[threadIdx.x] =
        threadIdx.x < P ? (PROLOGUE ? (int64_t)base[first] : tile_base[first]) : E;
  }
}

__global__ __launch_bounds__(GL_THREADS) void resort_scatter_kernel(
    const int32_t* __restrict__ ent_part_new, const int32_t* __restrict__ ent_values,
    const int64_t* __restrict__ tile_base, int64_t E, int A, int P, int64_t n_tiles,
    int32_t* __restrict__ out_part, int32_t* __restrict__ out_values,
    int32_t* __restrict__ inv, int64_t* __restrict__ ent_ptr) {
  resort_scatter_block<false>(ent_part_new, ent_values, nullptr, false,
                              const_cast<int64_t*>(tile_base), E, A, P, n_tiles,
                              out_part, out_values, inv, ent_ptr);
}

__global__ __launch_bounds__(GL_THREADS) void resort_scan_scatter_kernel(
    const int32_t* __restrict__ ent_part_new, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ hist, bool vec, int64_t* __restrict__ tile_base,
    int64_t E, int A, int P, int64_t n_tiles,
    int32_t* __restrict__ out_part, int32_t* __restrict__ out_values,
    int32_t* __restrict__ inv, int64_t* __restrict__ ent_ptr) {
  resort_scatter_block<true>(ent_part_new, ent_values, hist, vec, tile_base, E, A, P,
                             n_tiles, out_part, out_values, inv, ent_ptr);
}

// Re-sort pass 3: records stay put; their links follow the permutation.
DBL_D void resort_remap_item(
    const int64_t* __restrict__ rec_ent, const int32_t* __restrict__ inv,
    const int32_t* __restrict__ ent_part_new, int64_t R, int64_t r,
    int64_t* __restrict__ out_rec_ent, int32_t* __restrict__ out_rec_part) {
  if (r >= R) return;
  const int64_t e = rec_ent[r];
  out_rec_ent[r] = inv[e];
  out_rec_part[r] = ent_part_new[e];
}

__global__ void resort_remap_kernel(
    const int64_t* __restrict__ rec_ent, const int32_t* __restrict__ inv,
    const int32_t* __restrict__ ent_part_new, int64_t R,
    int64_t* __restrict__ out_rec_ent, int32_t* __restrict__ out_rec_part) {
  resort_remap_item(rec_ent, inv, ent_part_new, R,
                    (int64_t)blockIdx.x * blockDim.x + threadIdx.x, out_rec_ent,
                    out_rec_part);
}

// Sweep tail, launch 3: block 0 packs the summary (summary_finalize's work,
// which the remap neither feeds nor reads); the blocks after it remap.
__global__ void resort_remap_finalize_kernel(
    const int64_t* __restrict__ rec_ent, const int32_t* __restrict__ inv,
    const int32_t* __restrict__ ent_part_new, int64_t R,
    int64_t* __restrict__ out_rec_ent, int32_t* __restrict__ out_rec_part,
    const double* __restrict__ loglik, const unsigned long long* __restrict__ counts,
    int n_counts, const int* __restrict__ err, double* __restrict__ packed) {
  if (blockIdx.x == 0) {
    summary_finalize_items(loglik, counts, n_counts, err, (int)threadIdx.x,
                           (int)blockDim.x, packed);
  } else {
    resort_remap_item(rec_ent, inv, ent_part_new, R,
                      (int64_t)(blockIdx.x - 1) * blockDim.x + threadIdx.x,
                      out_rec_ent, out_rec_part);
  }
}

// ---------------------------------------------------------------------------
// K1 (GPU): banded Levenshtein / OSA sim-pair sweep over a value domain
// ---------------------------------------------------------------------------

// One WAVE per value i: the wave builds a Myers bit-parallel Peq table for
// string i in LDS once, then its 64 lanes sweep candidate values j from the
// length-bucketed window (sim > 0 bounds |len_i - len_j|). Edit distance via
// Hyyro's bit-vector recurrence: O(W * len_j) 64-bit ops per pair instead of
// the O(len_i * len_j) scratch-array DP, no scratch.
//
// The pattern (row value i) occupies W = ceil(len_i / 64) words, W compiled
// in. Rows are launched per length class (<= 64, 65..128, 129..192, 193..256)
// over that class's contiguous slice of len_order, so short rows always run
// the single-word instance whatever else the domain holds; the text (value j)
// may have any length at any W.
//
// Symbols are uint8 (direct-indexed 256-entry Peq) or 16-bit ids (per-wave
// open-addressing table over the pattern's own <= 64*W symbols); id 0 is
// padding in both and never occurs inside a value.
constexpr int SP_WAVES = 4;      // waves per block
constexpr int SP_WAVES_WIDE = 2; // 16-bit symbols at W >= 3 (LDS budget)
constexpr int SP_MAX_LEN = 256;  // 4 Myers words

// LDS per wave and the LDS-bound residency on a 160 KiB CU:
//   uint8   W=1..4: 2/4/6/8 KiB per wave, 4 waves per block
//           -> 20/10/6/5 blocks = 32/32/24/20 waves per CU
//   16-bit  W=1,2: 128/256 slots, 1.5/5 KiB per wave, 4 waves per block
//           -> 32/32 waves per CU
//           W=3,4: 512 slots, 14/18 KiB per wave, 2 waves per block
//           -> 5/4 blocks = 10/8 waves per CU
template <typename Sym, int W>
struct SimPeq;

template <int W>
struct SimPeq<uint8_t, W> {
  static constexpr int WORDS = 256 * W;  // 64-bit words per wave
  unsigned long long* mask;              // [256][W]

  __device__ explicit SimPeq(unsigned long long* lds) : mask(lds) {}
  __device__ void clear(int lane) {
    for (int c = lane; c < WORDS; c += WAVE) mask[c] = 0ull;
  }
  __device__ void insert(uint8_t sym, int pos) {
    atomicOr(&mask[(int)sym * W + (pos >> 6)], 1ull << (pos & 63));
  }
  __device__ void lookup(uint8_t sym, unsigned long long (&Eq)[W]) const {
#pragma unroll
    for (int w = 0; w < W; ++w) Eq[w] = mask[(int)sym * W + w];
  }
};

// Open addressing, linear probing, load <= 1/2 (a pattern of W words has at
// most 64*W distinct symbols). Key 0 marks an empty slot.
template <int W>
struct SimPeq<uint16_t, W> {
  static constexpr int SLOTS = W == 1 ? 128 : (W == 2 ? 256 : 512);
  static constexpr int WORDS = SLOTS * W + SLOTS / 2;
  unsigned long long* mask;  // [SLOTS][W]
  unsigned int* key;         // [SLOTS]

  __device__ explicit SimPeq(unsigned long long* lds)
      : mask(lds), key(reinterpret_cast<unsigned int*>(lds + SLOTS * W)) {}
  __device__ static unsigned slot_of(unsigned sym) {
    return ((sym * 40503u) >> 4) & (unsigned)(SLOTS - 1);
  }
  __device__ void clear(int lane) {
    for (int c = lane; c < WORDS; c += WAVE) mask[c] = 0ull;
  }
  __device__ void insert(uint16_t sym, int pos) {
    unsigned h = slot_of(sym);
    for (;;) {
      const unsigned prev = atomicCAS(&key[h], 0u, (unsigned)sym);
      if (prev == 0u || prev == (unsigned)sym) break;
      h = (h + 1u) & (unsigned)(SLOTS - 1);
    }
    atomicOr(&mask[(int)h * W + (pos >> 6)], 1ull << (pos & 63));
  }
  __device__ void lookup(uint16_t sym, unsigned long long (&Eq)[W]) const {
    unsigned h = slot_of(sym);
    for (;;) {
      const unsigned k = key[h];
      if (k == (unsigned)sym || k == 0u) break;  // empty slot: masks are 0
      h = (h + 1u) & (unsigned)(SLOTS - 1);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) Eq[w] = mask[(int)h * W + w];
  }
};

// The recurrence on a 64*W-bit integer held as W words: every step is
// bitwise except the add, which carries word to word, and the Ph/Mh left
// shifts, which carry their top bit (Ph's low word shifts in 1). The caller
// guarantees (m-1)/64 == W-1, so the score bit sits in the last word.
//
// TRANSPOSE adds the restricted Damerau-Levenshtein (optimal string
// alignment) term: an adjacent swap costs 1. Pattern position p may take a
// diagonal-zero through a transposition at text position j when p matches
// text j-1 (Eqprev), p-1 matches text j (Eq shifted up one, carrying across
// words) and the cell two back on the diagonal was no diagonal-zero
// (~D0prev). D0prev and Eqprev are the previous text position's D0 and Eq,
// kept in registers per lane, and are 0 before the first character. The
// term is OR-ed into Xh and Xv before Ph/Mh/Pv/Mv are formed; without
// TRANSPOSE none of it is compiled.
template <typename Sym, int W, bool TRANSPOSE>
__device__ int myers_distance(const SimPeq<Sym, W>& peq, int m, const Sym* b, int lb) {
  if (m == 0) return lb;
  int score = m;
  unsigned long long Pv[W], Mv[W];
  unsigned long long D0prev[W], Eqprev[W];  // TRANSPOSE only
#pragma unroll
  for (int w = 0; w < W; ++w) {
    Pv[w] = ~0ull;
    Mv[w] = 0ull;
    D0prev[w] = 0ull;
    Eqprev[w] = 0ull;
  }
  const unsigned long long last = 1ull << ((m - 1) & 63);
  for (int j = 0; j < lb; ++j) {
    unsigned long long Eq[W];
    peq.lookup(b[j], Eq);
    unsigned long long add_c = 0ull, ph_c = 1ull, mh_c = 0ull, tr_c = 0ull;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      unsigned long long Xv = Eq[w] | Mv[w];
      const unsigned long long t = Eq[w] & Pv[w];
      const unsigned long long s1 = t + Pv[w];
      const unsigned long long s2 = s1 + add_c;
      add_c = (unsigned long long)(s1 < t) | (unsigned long long)(s2 < s1);
      unsigned long long Xh = (s2 ^ Pv[w]) | Eq[w];
      if constexpr (TRANSPOSE) {
        // x's top bit carries into word w+1; it is taken from this word's
        // previous-column D0 before that is overwritten below
        const unsigned long long x = ~D0prev[w] & Eq[w];
        const unsigned long long TR = ((x << 1) | tr_c) & Eqprev[w];
        tr_c = x >> 63;
        Xh |= TR;
        Xv |= TR;
        D0prev[w] = Xh | Mv[w];
        Eqprev[w] = Eq[w];
      }
      unsigned long long Ph = Mv[w] | ~(Xh | Pv[w]);
      unsigned long long Mh = Pv[w] & Xh;
      if (w == W - 1) {
        if (Ph & last) ++score;
        if (Mh & last) --score;
      }
      const unsigned long long ph_o = Ph >> 63, mh_o = Mh >> 63;
      Ph = (Ph << 1) | ph_c;
      Mh = (Mh << 1) | mh_c;
      ph_c = ph_o;
      mh_c = mh_o;
      Pv[w] = Mh | ~(Xv | Ph);
      Mv[w] = Ph & Xv;
    }
  }
  return score;
}

template <typename Sym, int W, int WAVES, bool TRANSPOSE>
__global__ void __launch_bounds__(WAVES * WAVE) sim_pairs_kernel(
    const Sym* __restrict__ strs,      // [V, max_len]
    const int32_t* __restrict__ lens,  // [V]
    const int32_t* __restrict__ len_order,  // [V] value ids sorted by length
    const int64_t* __restrict__ len_ptr,    // [max_len + 2] bucket offsets by length
    int64_t row_begin, int64_t row_end,     // this class's slice of len_order
    int max_len, float threshold, float max_sim,
    int64_t* __restrict__ row_counts,  // [V] (pass 1 out) or row offsets (pass 2 in)
    int32_t* __restrict__ out_col,     // pass 2
    float* __restrict__ out_expsim,    // pass 2 (stores exp(sim))
    int64_t* __restrict__ fill_pos,    // [V] atomic cursors (pass 2)
    int fill) {
  __shared__ unsigned long long peq_block[WAVES * SimPeq<Sym, W>::WORDS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  // longest rows of the class first: they carry the widest windows
  const int64_t r = row_end - 1 - ((int64_t)blockIdx.x * WAVES + wave);
  if (r < row_begin) return;
  const int i = len_order[r];
  SimPeq<Sym, W> peq(peq_block + wave * SimPeq<Sym, W>::WORDS);
  const int la = lens[i];
  const Sym* a = strs + (int64_t)i * max_len;
  peq.clear(lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  for (int p = lane; p < la; p += WAVE) peq.insert(a[p], p);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();

  const float u0 = threshold / max_sim;
  const float scale = max_sim / (max_sim - threshold);
  const float band = (1.0f - u0) / (1.0f + u0);
  // length window: |la - lb| < band * (la + lb)
  int lb_min, lb_max;
  if (band >= 0.999f) {  // threshold ~ 0: no length pruning possible
    lb_min = 0;
    lb_max = max_len;
  } else {
    lb_min = (int)ceilf((1.0f - band) / (1.0f + band) * (float)la);
    lb_max = (int)floorf((1.0f + band) / (1.0f - band) * (float)la);
  }
  if (la == 0) { lb_min = 0; lb_max = 0; }
  if (lb_min < 0) lb_min = 0;
  if (lb_max > max_len) lb_max = max_len;
  const int64_t j0 = len_ptr[lb_min], j1 = len_ptr[lb_max + 1];

  int64_t n_hits = 0;
  for (int64_t jj = j0 + lane; jj < j1; jj += WAVE) {
    const int j = len_order[jj];
    const int lb = lens[j];
    const int tot = la + lb;
    float unit;
    if (tot == 0) {
      unit = 1.0f;
    } else {
      if ((float)abs(la - lb) >= band * (float)tot) continue;
      const int d =
          myers_distance<Sym, W, TRANSPOSE>(peq, la, strs + (int64_t)j * max_len, lb);
      unit = 1.0f - 2.0f * (float)d / ((float)tot + (float)d);
    }
    const float trans = scale * (max_sim * unit - threshold);
    if (trans <= 0.0f) continue;  // expsim <= 1 filtered (AttributeIndex.scala:226)
    if (!fill) {
      ++n_hits;
    } else {
      const int64_t pos = atomicAdd((unsigned long long*)&fill_pos[i], 1ull) + row_counts[i];
      out_col[pos] = j;
      out_expsim[pos] = __expf(trans);
    }
  }
  if (!fill) {
    double total = wave_sum((double)n_hits);
    if (lane == 0) row_counts[i] = (int64_t)(total + 0.5);
  }
}

// ---------------------------------------------------------------------------
// K1 (GPU): Jaro sim-pair sweep with the Winkler prefix boost
// ---------------------------------------------------------------------------

// Bits lo..hi of the 64*W-bit pattern that fall into word w (empty when
// hi < lo). Every shift count stays within 0..63.
__device__ __forceinline__ unsigned long long jaro_window_word(int lo, int hi, int w) {
  int l = lo - 64 * w, h = hi - 64 * w;
  if (h < 0 || l > 63 || h < l) return 0ull;
  if (l < 0) l = 0;
  if (h > 63) h = 63;
  return (~0ull << l) & (~0ull >> (63 - h));
}

// Matches m and transpositions t of the pattern (masks in `peq`, length
// la >= 1) against the text b (length lb >= 1), definition in jaro.h. The text
// is the outer string of the greedy matching; m and t do not depend on which
// string is the outer one (tests/test_similarity_jaro.py checks that).
//
// P_flag holds the matched pattern positions, T_flag the matched text
// positions (a text has up to 256 symbols at any W). Text position j takes
// the lowest free pattern position within [j-r, j+r] that holds its symbol.
// The second loop pairs the matched text positions, ascending, with the
// matched pattern positions, ascending: the two symbols agree exactly when
// the text symbol's mask has that pattern bit. All array indices are
// compile-time after unrolling, so the flags stay in registers.
template <typename Sym, int W>
__device__ void jaro_matches(const SimPeq<Sym, W>& peq, int la, const Sym* b, int lb,
                             int* m_out, int* t_out) {
  const int longer = la > lb ? la : lb;
  const int r = longer / 2 - 1 > 0 ? longer / 2 - 1 : 0;
  unsigned long long P_flag[W], T_flag[4];
#pragma unroll
  for (int w = 0; w < W; ++w) P_flag[w] = 0ull;
#pragma unroll
  for (int w = 0; w < 4; ++w) T_flag[w] = 0ull;
  // text positions past la - 1 + r see an empty window
  const int j_end = lb < la + r ? lb : la + r;
  for (int j = 0; j < j_end; ++j) {
    unsigned long long Eq[W];
    peq.lookup(b[j], Eq);
    const int lo = j - r > 0 ? j - r : 0;
    const int hi = j + r < la - 1 ? j + r : la - 1;  // never a bit at or above la
    bool taken = false;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const unsigned long long PM = Eq[w] & jaro_window_word(lo, hi, w) & ~P_flag[w];
      const unsigned long long low = PM & (0ull - PM);
      P_flag[w] |= taken ? 0ull : low;
      taken = taken || PM != 0ull;
    }
    const unsigned long long tbit = taken ? 1ull << (j & 63) : 0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) T_flag[w] |= (j >> 6) == w ? tbit : 0ull;
  }
  int m = 0;
#pragma unroll
  for (int w = 0; w < W; ++w) m += __popcll(P_flag[w]);
  int half = 0;
#pragma unroll
  for (int tw = 0; tw < 4; ++tw) {
    unsigned long long T = T_flag[tw];
    while (T != 0ull) {
      const int j = 64 * tw + __builtin_ctzll(T);
      T &= T - 1ull;
      unsigned long long Eq[W];
      peq.lookup(b[j], Eq);
      bool found = false, same = false;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const unsigned long long q = found ? 0ull : P_flag[w] & (0ull - P_flag[w]);
        same = same || (Eq[w] & q) != 0ull;
        P_flag[w] ^= q;
        found = found || q != 0ull;
      }
      half += same ? 0 : 1;
    }
  }
  *m_out = m;
  *t_out = half >> 1;
}

// Launched like sim_pairs_kernel: one wave per row value of one length class,
// the row's masks in LDS, lanes striding over the candidate window, a count
// pass (fill == 0) and a fill pass. The score is formed in fp64 from the
// integers (jaro_trans), so a pair enters the index here exactly when it does
// in jaro_pairs_cpu; only exp() of the result is fp32.
template <typename Sym, int W, int WAVES>
__global__ void __launch_bounds__(WAVES * WAVE) jaro_pairs_kernel(
    const Sym* __restrict__ strs,      // [V, max_len]
    const int32_t* __restrict__ lens,  // [V]
    const int32_t* __restrict__ len_order,  // [V] value ids sorted by length
    const int64_t* __restrict__ len_ptr,    // [max_len + 2] bucket offsets by length
    int64_t row_begin, int64_t row_end,     // this class's slice of len_order
    int max_len, JaroScale sc,
    int64_t* __restrict__ row_counts,  // [V] (pass 1 out) or row offsets (pass 2 in)
    int32_t* __restrict__ out_col,     // pass 2
    float* __restrict__ out_expsim,    // pass 2 (stores exp(sim))
    int64_t* __restrict__ fill_pos,    // [V] atomic cursors (pass 2)
    int fill) {
  __shared__ unsigned long long peq_block[WAVES * SimPeq<Sym, W>::WORDS];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t r = row_end - 1 - ((int64_t)blockIdx.x * WAVES + wave);
  if (r < row_begin) return;
  const int i = len_order[r];
  SimPeq<Sym, W> peq(peq_block + wave * SimPeq<Sym, W>::WORDS);
  const int la = lens[i];
  const Sym* a = strs + (int64_t)i * max_len;
  peq.clear(lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
  for (int p = lane; p < la; p += WAVE) peq.insert(a[p], p);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();

  // Length window from jaro_length_prunes: unit can exceed u0 only when
  // min/max of the two lengths exceeds q. One length of slack on either side
  // covers the rounding of the products; the per-pair test below decides.
  int lb_min = 0, lb_max = max_len;
  const double boost = 4.0 * sc.prefix_scale;
  if (boost < 1.0) {
    const double q = 3.0 * (sc.u0 - boost) / (1.0 - boost) - 2.0;
    if (q > 0.0) {
      lb_min = (int)floor(q * (double)la) - 1;
      const double top = ceil((double)la / q) + 1.0;
      if (top < (double)max_len) lb_max = (int)top;
    }
  }
  if (la == 0) { lb_min = 0; lb_max = 0; }  // an empty value scores with itself only
  if (lb_min < 0) lb_min = 0;
  if (lb_max > max_len) lb_max = max_len;
  const int64_t j0 = len_ptr[lb_min], j1 = len_ptr[lb_max + 1];

  int64_t n_hits = 0;
  for (int64_t jj = j0 + lane; jj < j1; jj += WAVE) {
    const int j = len_order[jj];
    const int lb = lens[j];
    if (jaro_length_prunes(sc, la, lb)) continue;
    const Sym* b = strs + (int64_t)j * max_len;
    int m = 0, t = 0;
    if (la > 0 && lb > 0) jaro_matches<Sym, W>(peq, la, b, lb, &m, &t);
    if (m == 0 && la + lb > 0) continue;  // unit 0
    // 32-bit gate: lengths are at most SP_MAX_LEN
    const double trans = jaro_trans<int>(sc, m, t, la, lb, jaro_common_prefix(a, la, b, lb));
    // exp(trans) > 1 in fp64, the CPU sweep's criterion: 1 + x rounds above 1
    // exactly when x > 2^-53
    if (!(trans > 0x1p-53)) continue;
    if (!fill) {
      ++n_hits;
    } else {
      const int64_t pos = atomicAdd((unsigned long long*)&fill_pos[i], 1ull) + row_counts[i];
      out_col[pos] = j;
      out_expsim[pos] = __expf((float)trans);
    }
  }
  if (!fill) {
    double total = wave_sum((double)n_hits);
    if (lane == 0) row_counts[i] = (int64_t)(total + 0.5);
  }
}

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------

static int64_t wave_grid(int64_t items, int waves_per_block) {
  return (items + waves_per_block - 1) / waves_per_block;
}

// LDS sim-row staging in the link kernels; DBLINK_SIMH=0 restores the
// global-memory binary-search path (A/B; results are bitwise identical).
// Re-read per launch so one process can time both arms.
static int simh_enabled() {
  const char* e = std::getenv("DBLINK_SIMH");
  return e ? std::atoi(e) : 1;
}

// Operands common to the link launchers, checked and unpacked in one place.
// The kernels keep flat __restrict__ parameters (struct members would lose
// the qualifier and with it the scalar loads); this bundles the host side.
// Shapes are on link_update_kernel's parameter list.
struct LinkArgs {
  const int32_t *rec_values, *rec_part, *ent_values, *csr_col;
  const uint8_t *rec_dist, *attr_const;
  const int64_t *rec_gid, *ent_ptr, *voff, *csr_row_ptr;
  const int64_t* ctrl;          // {seed, iteration} device override (or null)
  const float *log_norm, *csr_sim;
  int64_t* rec_ent_out;
  const int64_t* rec_ent_in;    // dense path: null, like log_norm, error_count
  int* error_count;
  int64_t R;
  uint64_t seed;
  uint32_t iteration;
  int A, simh_on;
};

static LinkArgs make_link_args(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_gid,
    torch::Tensor rec_part, torch::Tensor ent_values, torch::Tensor ent_ptr,
    torch::Tensor log_norm, torch::Tensor voff, torch::Tensor csr_row_ptr,
    torch::Tensor csr_col, torch::Tensor csr_sim, torch::Tensor attr_const,
    int64_t seed, int64_t iteration, torch::Tensor ctrl,
    torch::Tensor rec_ent_out, torch::Tensor rec_ent_in,
    torch::Tensor error_count) {
  CHECK_GPU(rec_values);
  LinkArgs a;
  a.R = rec_values.size(0);
  a.A = (int)rec_values.size(1);
  // 32-bit attr masks; nibble-packed staging descriptors hold 16 attributes
  TORCH_CHECK(a.A <= MAX_ATTRS, "at most ", MAX_ATTRS, " matching attributes supported");
  a.rec_values = rec_values.data_ptr<int32_t>();
  a.rec_dist = rec_dist.data_ptr<uint8_t>();
  a.rec_gid = rec_gid.data_ptr<int64_t>();
  a.rec_part = rec_part.data_ptr<int32_t>();
  a.ent_values = ent_values.data_ptr<int32_t>();
  a.ent_ptr = ent_ptr.data_ptr<int64_t>();
  a.log_norm = log_norm.defined() ? log_norm.data_ptr<float>() : nullptr;
  a.voff = voff.data_ptr<int64_t>();
  a.csr_row_ptr = csr_row_ptr.data_ptr<int64_t>();
  a.csr_col = csr_col.data_ptr<int32_t>();
  a.csr_sim = csr_sim.data_ptr<float>();
  a.attr_const = attr_const.data_ptr<uint8_t>();
  a.seed = (uint64_t)seed;
  a.iteration = (uint32_t)iteration;
  a.ctrl = ctrl.numel() ? ctrl.data_ptr<int64_t>() : nullptr;
  a.rec_ent_out = rec_ent_out.data_ptr<int64_t>();
  a.rec_ent_in = rec_ent_in.defined() ? rec_ent_in.data_ptr<int64_t>() : nullptr;
  a.error_count = error_count.defined() ? error_count.data_ptr<int>() : nullptr;
  a.simh_on = simh_enabled();
  return a;
}

// split_len > 0 takes records whose base list is longer off the wave kernel:
// it appends them to split_list ([R] int32, count in split_count[0], zeroed
// by the caller) and link_update_split_kernel serves the list from a static
// grid of split_grid blocks, so the launch pair is graph-safe.
void link_update_split(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_gid,
    torch::Tensor rec_part, torch::Tensor cand_lo, torch::Tensor cand_hi,
    torch::Tensor postings, torch::Tensor ent_values, torch::Tensor ent_ptr,
    torch::Tensor log_norm, torch::Tensor voff, torch::Tensor csr_row_ptr,
    torch::Tensor csr_col, torch::Tensor csr_sim, torch::Tensor attr_const,
    int64_t seed, int64_t iteration, torch::Tensor rec_ent_out,
    torch::Tensor rec_ent_in, torch::Tensor error_count,
    torch::Tensor small_mask, torch::Tensor ctrl, torch::Tensor pair_a1,
    torch::Tensor pair_a2, torch::Tensor split_list, torch::Tensor split_count,
    int64_t split_len, int64_t split_grid) {
  const LinkArgs L = make_link_args(
      rec_values, rec_dist, rec_gid, rec_part, ent_values, ent_ptr, log_norm,
      voff, csr_row_ptr, csr_col, csr_sim, attr_const, seed, iteration, ctrl,
      rec_ent_out, rec_ent_in, error_count);
  if (L.R == 0) return;
  const int NP = (int)pair_a1.numel();
  const int64_t* lo = cand_lo.data_ptr<int64_t>();
  const int64_t* hi = cand_hi.data_ptr<int64_t>();
  const int32_t* post = postings.data_ptr<int32_t>();
  const int32_t* a1 = pair_a1.data_ptr<int32_t>();
  const int32_t* a2 = pair_a2.data_ptr<int32_t>();
  constexpr int WPB = 4;
  int32_t* list_ptr = nullptr;
  int* count_ptr = nullptr;
  if (split_len > 0) {
    CHECK_GPU(split_list);
    CHECK_GPU(split_count);
    TORCH_CHECK(split_list.scalar_type() == torch::kInt32 &&
                    split_count.scalar_type() == torch::kInt32,
                "split_list and split_count must be int32");
    TORCH_CHECK(split_list.numel() >= L.R && split_count.numel() >= 1,
                "split_list holds R records, split_count one counter");
    TORCH_CHECK(L.R <= INT32_MAX, "split list indexes records with int32");
    TORCH_CHECK(split_grid >= 1 && split_grid <= 65535, "split_grid out of range");
    list_ptr = split_list.data_ptr<int32_t>();
    count_ptr = split_count.data_ptr<int>();
  }
  const bool split = small_mask.numel() > 0;
  const uint8_t* mask_ptr = split ? small_mask.data_ptr<uint8_t>() : nullptr;
  hipLaunchKernelGGL(link_update_kernel, dim3((unsigned)wave_grid(L.R, WPB)),
                     dim3(WPB * WAVE), 0, at::cuda::getCurrentCUDAStream(),
                     L.rec_values, L.rec_dist, L.rec_gid, L.rec_part, lo, hi,
                     post, L.ent_values, L.ent_ptr, L.log_norm, L.voff,
                     L.csr_row_ptr, L.csr_col, L.csr_sim, L.attr_const, a1, a2,
                     NP, mask_ptr, L.R, L.A, L.seed, L.iteration, L.ctrl,
                     L.rec_ent_out, L.rec_ent_in, L.error_count, L.simh_on,
                     split_len, list_ptr, count_ptr);
  if (split_len > 0)
    hipLaunchKernelGGL(link_update_split_kernel, dim3((unsigned)split_grid),
                       dim3(LINK_SPLIT_THREADS), 0,
                       at::cuda::getCurrentCUDAStream(), list_ptr, count_ptr,
                       L.rec_values, L.rec_dist, L.rec_gid, L.rec_part, lo, hi,
                       post, L.ent_values, L.ent_ptr, L.log_norm, L.voff,
                       L.csr_row_ptr, L.csr_col, L.csr_sim, L.attr_const, a1,
                       a2, NP, L.A, L.seed, L.iteration, L.ctrl, L.rec_ent_out,
                       L.rec_ent_in, L.error_count, L.simh_on);
  if (split)
    hipLaunchKernelGGL(link_update_small_kernel,
                       dim3((unsigned)((L.R + 255) / 256)), dim3(256), 0,
                       at::cuda::getCurrentCUDAStream(), mask_ptr, L.R,
                       L.rec_values, L.rec_dist, L.rec_gid, L.rec_part, lo, hi,
                       post, L.ent_values, L.ent_ptr, L.log_norm, L.voff,
                       L.csr_row_ptr, L.csr_col, L.csr_sim, L.attr_const, a1,
                       a2, NP, L.A, L.seed, L.iteration, L.ctrl, L.rec_ent_out,
                       L.rec_ent_in, L.error_count);
}

void link_update(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_gid,
    torch::Tensor rec_part, torch::Tensor cand_lo, torch::Tensor cand_hi,
    torch::Tensor postings, torch::Tensor ent_values, torch::Tensor ent_ptr,
    torch::Tensor log_norm, torch::Tensor voff, torch::Tensor csr_row_ptr,
    torch::Tensor csr_col, torch::Tensor csr_sim, torch::Tensor attr_const,
    int64_t seed, int64_t iteration, torch::Tensor rec_ent_out,
    torch::Tensor rec_ent_in, torch::Tensor error_count,
    torch::Tensor small_mask, torch::Tensor ctrl, torch::Tensor pair_a1,
    torch::Tensor pair_a2) {
  link_update_split(rec_values, rec_dist, rec_gid, rec_part, cand_lo, cand_hi,
                    postings, ent_values, ent_ptr, log_norm, voff, csr_row_ptr,
                    csr_col, csr_sim, attr_const, seed, iteration, rec_ent_out,
                    rec_ent_in, error_count, small_mask, ctrl, pair_a1, pair_a2,
                    torch::Tensor(), torch::Tensor(), 0, 0);
}

// The link phase in one launch, for a split list that the previous launch
// completed (postings_scatter_ranges_split with the same split_len > 0):
// split_grid blocks serve the list, the wave blocks skip the listed records.
void link_update_merged(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_gid,
    torch::Tensor rec_part, torch::Tensor cand_lo, torch::Tensor cand_hi,
    torch::Tensor postings, torch::Tensor ent_values, torch::Tensor ent_ptr,
    torch::Tensor log_norm, torch::Tensor voff, torch::Tensor csr_row_ptr,
    torch::Tensor csr_col, torch::Tensor csr_sim, torch::Tensor attr_const,
    int64_t seed, int64_t iteration, torch::Tensor rec_ent_out,
    torch::Tensor rec_ent_in, torch::Tensor error_count, torch::Tensor ctrl,
    torch::Tensor pair_a1, torch::Tensor pair_a2, torch::Tensor split_list,
    torch::Tensor split_count, int64_t split_len, int64_t split_grid) {
  const LinkArgs L = make_link_args(
      rec_values, rec_dist, rec_gid, rec_part, ent_values, ent_ptr, log_norm,
      voff, csr_row_ptr, csr_col, csr_sim, attr_const, seed, iteration, ctrl,
      rec_ent_out, rec_ent_in, error_count);
  if (L.R == 0) return;
  CHECK_GPU(split_list);
  CHECK_GPU(split_count);
  TORCH_CHECK(split_len > 0, "link_update_merged needs split_len > 0");
  TORCH_CHECK(split_list.scalar_type() == torch::kInt32 &&
                  split_count.scalar_type() == torch::kInt32,
              "split_list and split_count must be int32");
  TORCH_CHECK(split_list.numel() >= L.R && split_count.numel() >= 1 &&
                  L.R <= INT32_MAX,
              "split_list holds R records, split_count one counter");
  TORCH_CHECK(split_grid >= 1 && split_grid <= 65535, "split_grid out of range");
  const int64_t n_wave = wave_grid(L.R, LINK_SPLIT_WAVES);
  hipLaunchKernelGGL(link_update_merged_kernel, dim3((unsigned)(split_grid + n_wave)),
                     dim3(LINK_SPLIT_THREADS), 0, at::cuda::getCurrentCUDAStream(),
                     split_list.data_ptr<int32_t>(), split_count.data_ptr<int>(),
                     L.rec_values, L.rec_dist, L.rec_gid, L.rec_part,
                     cand_lo.data_ptr<int64_t>(), cand_hi.data_ptr<int64_t>(),
                     postings.data_ptr<int32_t>(), L.ent_values, L.ent_ptr,
                     L.log_norm, L.voff, L.csr_row_ptr, L.csr_col, L.csr_sim,
                     L.attr_const, pair_a1.data_ptr<int32_t>(),
                     pair_a2.data_ptr<int32_t>(), (int)pair_a1.numel(), L.R, L.A,
                     L.seed, L.iteration, L.ctrl, L.rec_ent_out, L.rec_ent_in,
                     L.error_count, L.simh_on, split_len, (unsigned)split_grid);
}

void postings_hist(torch::Tensor ent_part, torch::Tensor ent_values,
                   torch::Tensor pair_a1, torch::Tensor pair_a2,
                   torch::Tensor pair_v2, int64_t Vmax, torch::Tensor counts) {
  const int64_t E = ent_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t n = E * (A + NP);
  if (n == 0) return;
  TORCH_CHECK(counts.numel() <= INT32_MAX, "dense key space exceeds int32");
  dim3 grid((unsigned)((n + PB_THREADS - 1) / PB_THREADS));
  hipLaunchKernelGGL(postings_hist_kernel, grid, dim3(PB_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), E, A, NP, Vmax,
                     counts.data_ptr<int32_t>());
}

// Sweep head in one launch: postings_hist into counts, zero_blk (int32) all
// zero, and stage (device) = stage_pin (pinned host memory, same byte count,
// whole 32-bit words).
void sweep_begin(torch::Tensor ent_part, torch::Tensor ent_values,
                 torch::Tensor pair_a1, torch::Tensor pair_a2,
                 torch::Tensor pair_v2, int64_t Vmax, torch::Tensor counts,
                 torch::Tensor zero_blk, torch::Tensor stage_pin,
                 torch::Tensor stage) {
  CHECK_GPU(ent_values);
  CHECK_GPU(zero_blk);
  CHECK_GPU(stage);
  CHECK_CONTIG(zero_blk);
  CHECK_CONTIG(stage_pin);
  CHECK_CONTIG(stage);
  const int64_t E = ent_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t n = E * (A + NP);
  TORCH_CHECK(counts.numel() <= INT32_MAX, "dense key space exceeds int32");
  TORCH_CHECK(zero_blk.scalar_type() == torch::kInt32, "sweep_begin: zero_blk int32");
  TORCH_CHECK(!stage_pin.is_cuda() && stage_pin.is_pinned(),
              "sweep_begin: stage_pin must be pinned host memory");
  const int64_t stage_bytes = stage.numel() * stage.element_size();
  TORCH_CHECK(stage_pin.numel() * stage_pin.element_size() == stage_bytes &&
                  stage_bytes % 4 == 0 && stage_bytes / 4 <= INT32_MAX &&
                  (reinterpret_cast<uintptr_t>(stage.data_ptr()) & 3) == 0 &&
                  (reinterpret_cast<uintptr_t>(stage_pin.data_ptr()) & 3) == 0,
              "sweep_begin: stage buffers must be equal-sized runs of 32-bit words");
  const int64_t n_hist = (n + PB_THREADS - 1) / PB_THREADS;
  const int64_t zero_n = zero_blk.numel();
  const int64_t n_zero = (zero_n + 4 * PB_THREADS - 1) / (4 * PB_THREADS);
  TORCH_CHECK(n_hist + 1 + n_zero <= INT32_MAX, "sweep_begin: grid out of range");
  const bool zero_vec = (reinterpret_cast<uintptr_t>(zero_blk.data_ptr()) & 15) == 0;
  hipLaunchKernelGGL(sweep_begin_kernel, dim3((unsigned)(n_hist + 1 + n_zero)),
                     dim3(PB_THREADS), 0, at::cuda::getCurrentCUDAStream(),
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), E, A, NP, Vmax,
                     counts.data_ptr<int32_t>(), (unsigned)n_hist,
                     zero_blk.data_ptr<int32_t>(), zero_n, zero_vec,
                     static_cast<const uint32_t*>(stage_pin.data_ptr()),
                     static_cast<uint32_t*>(stage.data_ptr()),
                     (int)(stage_bytes / 4));
}

void postings_scatter(torch::Tensor ent_part, torch::Tensor ent_values,
                      torch::Tensor pair_a1, torch::Tensor pair_a2,
                      torch::Tensor pair_v2, int64_t Vmax, torch::Tensor cursor,
                      torch::Tensor postings) {
  const int64_t E = ent_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t n = E * (A + NP);
  if (n == 0) return;
  TORCH_CHECK(cursor.numel() <= INT32_MAX, "dense key space exceeds int32");
  dim3 grid((unsigned)((n + PB_THREADS - 1) / PB_THREADS));
  hipLaunchKernelGGL(postings_scatter_kernel, grid, dim3(PB_THREADS), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), E, A, NP, Vmax,
                     cursor.data_ptr<int32_t>(), postings.data_ptr<int32_t>());
}

void classify_modes(torch::Tensor rec_values, torch::Tensor rec_dist,
                    torch::Tensor rec_part, torch::Tensor ent_ptr,
                    torch::Tensor cand_lo, torch::Tensor cand_hi, int64_t NP,
                    int64_t small_threshold, int64_t heavy_threshold,
                    torch::Tensor mode) {
  const int64_t R = rec_values.size(0);
  const int A = (int)rec_values.size(1);
  if (R == 0) return;
  dim3 grid((unsigned)((R + 255) / 256));
  hipLaunchKernelGGL(classify_modes_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     rec_values.data_ptr<int32_t>(), rec_dist.data_ptr<uint8_t>(),
                     rec_part.data_ptr<int32_t>(), ent_ptr.data_ptr<int64_t>(),
                     cand_lo.data_ptr<int64_t>(), cand_hi.data_ptr<int64_t>(),
                     R, A, (int)NP, small_threshold, heavy_threshold,
                     mode.data_ptr<uint8_t>());
}

// Stable inverted-index keys: (key * E + e) sorts into the same segment
// boundaries as the counting-sort prefix, but with entities in ascending-id
// order within each segment — deterministic indexed draws for the heavy
// sampler's posting-segment proposals.
__global__ void build_ekeys_stable_kernel(
    const int32_t* __restrict__ ent_part, const int32_t* __restrict__ ent_values,
    const int32_t* __restrict__ pair_a1, const int32_t* __restrict__ pair_a2,
    const int32_t* __restrict__ pair_v2, int64_t E, int A, int NP, int64_t Vmax,
    int64_t* __restrict__ ekeys) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int T = A + NP;
  if (idx >= E * T) return;
  const int t = (int)(idx / E);
  const int64_t e = idx % E;
  const int64_t v = posting_slot_value(ent_values, e, A, t, pair_a1, pair_a2, pair_v2);
  const int64_t key = ((int64_t)ent_part[e] * T + t) * Vmax + v;
  ekeys[idx] = key * E + e;
}

// hipGraph-safe radix sort: torch.sort allocates its workspace through the
// caching allocator, which faults on replay when capture records multi-GB
// pools (the r01 ">4M records" graph bug). These wrappers let the engine own
// ONE persistent workspace and keep every launch on the capture stream.
int64_t radix_sort_pairs_temp_bytes(int64_t n) {
  size_t bytes = 0;
  rocprim::radix_sort_pairs(
      nullptr, bytes, (const int64_t*)nullptr, (int64_t*)nullptr,
      (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)n);
  return (int64_t)bytes;
}

void radix_sort_pairs_i64_i32(torch::Tensor keys_in, torch::Tensor keys_out,
                              torch::Tensor vals_in, torch::Tensor vals_out,
                              int64_t end_bit, torch::Tensor temp) {
  const size_t n = (size_t)keys_in.numel();
  if (n == 0) return;
  size_t bytes = (size_t)temp.numel();
  hipError_t err = rocprim::radix_sort_pairs(
      temp.data_ptr(), bytes, keys_in.data_ptr<int64_t>(),
      keys_out.data_ptr<int64_t>(), vals_in.data_ptr<int32_t>(),
      vals_out.data_ptr<int32_t>(), n, 0, (unsigned)end_bit,
      at::cuda::getCurrentCUDAStream());
  TORCH_CHECK(err == hipSuccess, "radix_sort_pairs failed: ",
              hipGetErrorString(err));
}

void build_ekeys_stable(torch::Tensor ent_part, torch::Tensor ent_values,
                        torch::Tensor pair_a1, torch::Tensor pair_a2,
                        torch::Tensor pair_v2, int64_t Vmax,
                        torch::Tensor ekeys) {
  const int64_t E = ent_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t n = E * (A + NP);
  if (n == 0) return;
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(build_ekeys_stable_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), E, A, NP, Vmax,
                     ekeys.data_ptr<int64_t>());
}

void link_update_heavy(
    torch::Tensor mode, torch::Tensor rec_values, torch::Tensor rec_dist,
    torch::Tensor rec_gid, torch::Tensor rec_part, torch::Tensor ent_values,
    torch::Tensor ent_ptr, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor attr_const, torch::Tensor csr_row_ptr_big,
    torch::Tensor csr_col_big, torch::Tensor csr_sim_big, double tau,
    torch::Tensor postings, torch::Tensor idx_ptr,
    int64_t Vmax, int64_t NP, int64_t seed, int64_t iteration, torch::Tensor ctrl,
    torch::Tensor rec_ent_out, torch::Tensor rec_ent_in,
    torch::Tensor error_count, torch::Tensor stats) {
  const LinkArgs L = make_link_args(
      rec_values, rec_dist, rec_gid, rec_part, ent_values, ent_ptr, log_norm,
      voff, csr_row_ptr, csr_col, csr_sim, attr_const, seed, iteration, ctrl,
      rec_ent_out, rec_ent_in, error_count);
  if (L.R == 0) return;
  hipLaunchKernelGGL(link_update_heavy_kernel,
                     dim3((unsigned)wave_grid(L.R, HEAVY_WAVES)),
                     dim3(HEAVY_WAVES * WAVE), 0, at::cuda::getCurrentCUDAStream(),
                     mode.data_ptr<uint8_t>(), L.rec_values, L.rec_dist,
                     L.rec_gid, L.rec_part, L.ent_values, L.ent_ptr, L.log_norm,
                     L.voff, L.csr_row_ptr, L.csr_col, L.csr_sim, L.attr_const,
                     csr_row_ptr_big.data_ptr<int64_t>(),
                     csr_col_big.data_ptr<int32_t>(), csr_sim_big.data_ptr<float>(),
                     (float)tau, postings.data_ptr<int32_t>(),
                     idx_ptr.data_ptr<int64_t>(), Vmax, (int)NP, L.R, L.A,
                     L.seed, L.iteration, L.ctrl, L.rec_ent_out, L.rec_ent_in,
                     L.error_count,
                     stats.numel() ? (unsigned long long*)stats.data_ptr<int64_t>()
                                   : nullptr,
                     L.simh_on);
}

void cand_ranges(torch::Tensor rec_part, torch::Tensor rec_values,
                 torch::Tensor pair_a1, torch::Tensor pair_a2,
                 torch::Tensor pair_v2, torch::Tensor ptr, int64_t Vmax,
                 torch::Tensor cand_lo, torch::Tensor cand_hi) {
  const int64_t R = rec_values.size(0);
  const int A = (int)rec_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t n = R * (A + NP);
  if (n == 0) return;
  dim3 grid((unsigned)((n + 255) / 256));
  hipLaunchKernelGGL(cand_ranges_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     rec_part.data_ptr<int32_t>(), rec_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), ptr.data_ptr<int64_t>(),
                     R, A, NP, Vmax,
                     cand_lo.data_ptr<int64_t>(), cand_hi.data_ptr<int64_t>());
}

// postings_scatter and cand_ranges as one launch (same results as the pair).
// split_len < 0: scatter and ranges only. Otherwise the launch also builds the
// link phase's split list (postings_scatter_ranges_split_kernel).
static void postings_scatter_ranges_run(
    torch::Tensor ent_part, torch::Tensor ent_values, torch::Tensor rec_part,
    torch::Tensor rec_values, torch::Tensor pair_a1, torch::Tensor pair_a2,
    torch::Tensor pair_v2, int64_t Vmax, torch::Tensor cursor, torch::Tensor ptr,
    torch::Tensor postings, torch::Tensor cand_lo, torch::Tensor cand_hi,
    torch::Tensor rec_dist, torch::Tensor attr_const, torch::Tensor ent_ptr,
    torch::Tensor split_list, torch::Tensor split_count, int64_t split_len) {
  CHECK_GPU(ent_values);
  CHECK_CONTIG(ent_values);
  CHECK_CONTIG(rec_values);
  CHECK_CONTIG(postings);
  CHECK_CONTIG(cand_lo);
  CHECK_CONTIG(cand_hi);
  const int64_t E = ent_values.size(0), R = rec_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t T = A + NP;
  TORCH_CHECK(rec_values.size(1) == A && ent_part.numel() == E &&
              rec_part.numel() == R && postings.numel() >= E * T &&
              cand_lo.numel() == R * T && cand_hi.numel() == R * T &&
              ptr.numel() == cursor.numel() + 1,
              "postings_scatter_ranges: shape mismatch");
  TORCH_CHECK(cursor.numel() <= INT32_MAX, "dense key space exceeds int32");
  const bool with_list = split_len >= 0;
  const int64_t n_scatter = (E * T + PB_THREADS - 1) / PB_THREADS;
  const int64_t n_ranges = ((with_list ? R : R * T) + PB_THREADS - 1) / PB_THREADS;
  if (n_scatter + n_ranges == 0) return;
  TORCH_CHECK(n_scatter + n_ranges <= INT32_MAX, "postings_scatter_ranges: grid too large");
  auto stream = at::cuda::getCurrentCUDAStream();
  if (!with_list) {
    hipLaunchKernelGGL(postings_scatter_ranges_kernel,
                       dim3((unsigned)(n_scatter + n_ranges)), dim3(PB_THREADS), 0,
                       stream,
                       ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                       rec_part.data_ptr<int32_t>(), rec_values.data_ptr<int32_t>(),
                       pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                       pair_v2.data_ptr<int32_t>(), ptr.data_ptr<int64_t>(), E, R, A,
                       NP, Vmax, (unsigned)n_scatter, cursor.data_ptr<int32_t>(),
                       postings.data_ptr<int32_t>(), cand_lo.data_ptr<int64_t>(),
                       cand_hi.data_ptr<int64_t>());
    return;
  }
  CHECK_GPU(split_list);
  CHECK_GPU(split_count);
  CHECK_CONTIG(rec_dist);
  TORCH_CHECK(A <= MAX_ATTRS, "at most ", MAX_ATTRS, " matching attributes supported");
  TORCH_CHECK(split_list.scalar_type() == torch::kInt32 &&
                  split_count.scalar_type() == torch::kInt32,
              "split_list and split_count must be int32");
  TORCH_CHECK(split_list.numel() >= R && split_count.numel() >= 1 && R <= INT32_MAX,
              "split_list holds R records, split_count one counter");
  TORCH_CHECK(rec_dist.numel() == R * A && attr_const.numel() == A &&
                  ent_ptr.scalar_type() == torch::kInt64,
              "postings_scatter_ranges_split: shape mismatch");
  hipLaunchKernelGGL(postings_scatter_ranges_split_kernel,
                     dim3((unsigned)(n_scatter + n_ranges)), dim3(PB_THREADS), 0,
                     stream,
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     rec_part.data_ptr<int32_t>(), rec_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(), ptr.data_ptr<int64_t>(), E, R, A,
                     NP, Vmax, (unsigned)n_scatter, cursor.data_ptr<int32_t>(),
                     postings.data_ptr<int32_t>(), cand_lo.data_ptr<int64_t>(),
                     cand_hi.data_ptr<int64_t>(), rec_dist.data_ptr<uint8_t>(),
                     attr_const.data_ptr<uint8_t>(), ent_ptr.data_ptr<int64_t>(),
                     split_len, split_list.data_ptr<int32_t>(),
                     split_count.data_ptr<int>());
}

void postings_scatter_ranges(torch::Tensor ent_part, torch::Tensor ent_values,
                             torch::Tensor rec_part, torch::Tensor rec_values,
                             torch::Tensor pair_a1, torch::Tensor pair_a2,
                             torch::Tensor pair_v2, int64_t Vmax,
                             torch::Tensor cursor, torch::Tensor ptr,
                             torch::Tensor postings, torch::Tensor cand_lo,
                             torch::Tensor cand_hi) {
  postings_scatter_ranges_run(ent_part, ent_values, rec_part, rec_values, pair_a1,
                              pair_a2, pair_v2, Vmax, cursor, ptr, postings, cand_lo,
                              cand_hi, {}, {}, {}, {}, {}, -1);
}

// postings_scatter_ranges plus the split list of link_update_merged: record r
// is listed when its base list is longer than split_len (>= 0). split_count
// must be zero on entry.
void postings_scatter_ranges_split(
    torch::Tensor ent_part, torch::Tensor ent_values, torch::Tensor rec_part,
    torch::Tensor rec_values, torch::Tensor pair_a1, torch::Tensor pair_a2,
    torch::Tensor pair_v2, int64_t Vmax, torch::Tensor cursor, torch::Tensor ptr,
    torch::Tensor postings, torch::Tensor cand_lo, torch::Tensor cand_hi,
    torch::Tensor rec_dist, torch::Tensor attr_const, torch::Tensor ent_ptr,
    torch::Tensor split_list, torch::Tensor split_count, int64_t split_len) {
  TORCH_CHECK(split_len >= 0, "postings_scatter_ranges_split: split_len >= 0");
  postings_scatter_ranges_run(ent_part, ent_values, rec_part, rec_values, pair_a1,
                              pair_a2, pair_v2, Vmax, cursor, ptr, postings, cand_lo,
                              cand_hi, rec_dist, attr_const, ent_ptr, split_list,
                              split_count, split_len);
}

void link_update_dense(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_gid,
    torch::Tensor rec_part, torch::Tensor rec_file, torch::Tensor ent_values,
    torch::Tensor ent_ptr, torch::Tensor theta, torch::Tensor phi,
    torch::Tensor norm_lin, torch::Tensor voff, torch::Tensor csr_row_ptr,
    torch::Tensor csr_col, torch::Tensor csr_sim, torch::Tensor attr_const,
    int64_t collapsed, int64_t seed, int64_t iteration, torch::Tensor rec_ent_out,
    torch::Tensor ctrl) {
  // linear norm_lin instead of log_norm; no empty-set tail (weights > 0)
  const LinkArgs L = make_link_args(
      rec_values, rec_dist, rec_gid, rec_part, ent_values, ent_ptr, {}, voff,
      csr_row_ptr, csr_col, csr_sim, attr_const, seed, iteration, ctrl,
      rec_ent_out, {}, {});
  const int F = (int)theta.size(1);
  if (L.R == 0) return;
  constexpr int WPB = 4;
  hipLaunchKernelGGL(link_update_dense_kernel,
                     dim3((unsigned)wave_grid(L.R, WPB)), dim3(WPB * WAVE), 0,
                     at::cuda::getCurrentCUDAStream(), L.rec_values, L.rec_dist,
                     L.rec_gid, L.rec_part, rec_file.data_ptr<int32_t>(),
                     L.ent_values, L.ent_ptr, theta.data_ptr<float>(),
                     phi.data_ptr<float>(), norm_lin.data_ptr<float>(), L.voff,
                     L.csr_row_ptr, L.csr_col, L.csr_sim, L.attr_const, L.R, L.A,
                     F, (int)collapsed, L.seed, L.iteration, L.ctrl,
                     L.rec_ent_out, L.simh_on);
}

// Opt-in value-phase work counters (DBLink_VALUE_STATS): set once from
// python; the tensor is held so the device pointer stays alive.
static unsigned long long* g_value_stats = nullptr;
static torch::Tensor g_value_stats_keep;
static const double* g_tab_excl = nullptr;
static const double* g_tab_rawsum = nullptr;
static const float* g_self_expsim = nullptr;
static int g_ktab_max = 0;
static int64_t g_tab_nnz = 0;
static std::vector<torch::Tensor> g_ktab_keep;
static const double* g_tab2_excl = nullptr;
static const double* g_tab2_rawsum = nullptr;
static int g_k2tab_max = 0;
static std::vector<torch::Tensor> g_k2tab_keep;

void set_value_k2tables(torch::Tensor excl, torch::Tensor rawsum, int64_t k2max) {
  if (k2max >= 2 && excl.numel()) {
    g_k2tab_keep = {excl, rawsum};
    g_tab2_excl = excl.data_ptr<double>();
    g_tab2_rawsum = rawsum.data_ptr<double>();
    g_k2tab_max = (int)k2max;
  } else {
    g_k2tab_keep.clear();
    g_tab2_excl = nullptr;
    g_tab2_rawsum = nullptr;
    g_k2tab_max = 0;
  }
}

// Install the k>=2 single-distinct-value perturbation tables (one level per
// k in [2, kmax]); pairs whose linked records all share one (value, file)
// then draw in O(log row) like the k=1 kernel.
void set_value_ktables(torch::Tensor excl, torch::Tensor rawsum,
                       torch::Tensor self_expsim, int64_t kmax, int64_t nnz) {
  if (kmax >= 2 && excl.numel()) {
    g_ktab_keep = {excl, rawsum, self_expsim};
    g_tab_excl = excl.data_ptr<double>();
    g_tab_rawsum = rawsum.data_ptr<double>();
    g_self_expsim = self_expsim.data_ptr<float>();
    g_ktab_max = (int)kmax;
    g_tab_nnz = nnz;
  } else {
    g_ktab_keep.clear();
    g_tab_excl = nullptr;
    g_tab_rawsum = nullptr;
    g_self_expsim = nullptr;
    g_ktab_max = 0;
    g_tab_nnz = 0;
  }
}

void set_value_stats(torch::Tensor t) {
  if (t.numel()) {
    g_value_stats_keep = t;
    g_value_stats = (unsigned long long*)t.data_ptr<int64_t>();
  } else {
    g_value_stats = nullptr;
    g_value_stats_keep = torch::Tensor();
  }
}

static ValueArgs make_value_args(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor ent_rec_idx, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor log_phi,
    torch::Tensor norm_lin, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor phi_prob, torch::Tensor phi_alias, torch::Tensor pow_prob,
    torch::Tensor pow_alias, torch::Tensor pow_off, torch::Tensor log_pow_total,
    torch::Tensor attr_const, int64_t Kc, int64_t collapsed, int64_t seed,
    int64_t iteration, int64_t ent_id_base, torch::Tensor error_count,
    torch::Tensor csr_excl, torch::Tensor csr_rawsum, torch::Tensor z1) {
  ValueArgs a;
  a.ctrl = nullptr;
  a.kobs = nullptr;
  a.pair_list = nullptr;
  a.pair_lists = nullptr;
  a.list_count = nullptr;
  a.stats = g_value_stats;
  {
    const char* e = std::getenv("DBLINK_VCHUNK");
    a.vchunk = e ? std::atoi(e) : 1;
  }
  a.tab_excl = g_tab_excl;
  a.tab_rawsum = g_tab_rawsum;
  a.self_expsim = g_self_expsim;
  a.ktab_max = g_ktab_max;
  a.nnz = g_tab_nnz;
  a.tab2_excl = g_tab2_excl;
  a.tab2_rawsum = g_tab2_rawsum;
  a.k2tab_max = g_k2tab_max;
  a.csr_excl = csr_excl.numel() ? csr_excl.data_ptr<double>() : nullptr;
  a.csr_rawsum = csr_rawsum.data_ptr<double>();
  a.z1 = z1.data_ptr<double>();
  a.rec_values = rec_values.data_ptr<int32_t>();
  a.rec_dist = rec_dist.data_ptr<uint8_t>();
  a.rec_file = rec_file.data_ptr<int32_t>();
  a.ent_rec_ptr = ent_rec_ptr.data_ptr<int64_t>();
  a.ent_rec_idx = ent_rec_idx.data_ptr<int64_t>();
  a.ent_values = ent_values.data_ptr<int32_t>();
  a.theta = theta.data_ptr<float>();
  a.phi = phi.data_ptr<float>();
  a.log_phi = log_phi.data_ptr<float>();
  a.norm_lin = norm_lin.data_ptr<float>();
  a.log_norm = log_norm.data_ptr<float>();
  a.voff = voff.data_ptr<int64_t>();
  a.csr_row_ptr = csr_row_ptr.data_ptr<int64_t>();
  a.csr_col = csr_col.data_ptr<int32_t>();
  a.csr_sim = csr_sim.data_ptr<float>();
  a.phi_prob = phi_prob.data_ptr<float>();
  a.phi_alias = phi_alias.data_ptr<int32_t>();
  a.pow_prob = pow_prob.numel() ? pow_prob.data_ptr<float>() : nullptr;
  a.pow_alias = pow_alias.numel() ? pow_alias.data_ptr<int32_t>() : nullptr;
  a.pow_off = pow_off.data_ptr<int64_t>();
  a.log_pow_total = log_pow_total.data_ptr<float>();
  a.attr_const = attr_const.data_ptr<uint8_t>();
  a.Kc = (int)Kc;
  a.E = ent_values.size(0);
  a.A = (int)ent_values.size(1);
  a.F = (int)theta.size(1);
  a.collapsed = (int)collapsed;
  a.seed = (uint64_t)seed;
  a.iteration = (uint32_t)iteration;
  a.ent_id_base = (uint64_t)ent_id_base;
  a.error_count = error_count.data_ptr<int>();
  return a;
}

// pair_lists ([E*A] int32) and list_count ([2] int32, zeroed by the caller)
// switch the kobs mode to list mode: value_update_kd1_kernel classifies every
// k >= 2 pair once and the hash and merge kernels run one wave per listed
// pair from a static grid of at most list_grid blocks. Empty tensors keep the
// self-selecting kobs mode.
static void value_update_run(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor ent_rec_idx, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor log_phi,
    torch::Tensor norm_lin, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor phi_prob, torch::Tensor phi_alias, torch::Tensor pow_prob,
    torch::Tensor pow_alias, torch::Tensor pow_off, torch::Tensor log_pow_total,
    torch::Tensor attr_const, int64_t Kc, int64_t collapsed, int64_t sequential,
    int64_t seed, int64_t iteration, int64_t ent_id_base, torch::Tensor error_count,
    torch::Tensor wave_pairs, torch::Tensor base_pairs, torch::Tensor k1_pairs,
    torch::Tensor csr_excl, torch::Tensor csr_rawsum, torch::Tensor z1,
    torch::Tensor ctrl, torch::Tensor kobs, torch::Tensor pair_lists,
    torch::Tensor list_count, int64_t list_grid, bool thread_merge) {
  ValueArgs args = make_value_args(
      rec_values, rec_dist, rec_file, ent_rec_ptr, ent_rec_idx, ent_values, theta,
      phi, log_phi, norm_lin, log_norm, voff, csr_row_ptr, csr_col, csr_sim,
      phi_prob, phi_alias, pow_prob, pow_alias, pow_off, log_pow_total, attr_const,
      Kc, collapsed, seed, iteration, ent_id_base, error_count, csr_excl,
      csr_rawsum, z1);
  args.ctrl = ctrl.numel() ? ctrl.data_ptr<int64_t>() : nullptr;
  const auto stream = at::cuda::getCurrentCUDAStream();
  // thread-per-pair kernels: one thread per entry of the current pair range
  auto launch_threads = [&](void (*kernel)(ValueArgs)) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((args.n_pairs + 255) / 256)),
                       dim3(256), 0, stream, args);
  };
  // wave kernels: n_waves waves, WAVES_PER_BLOCK_VAL per block
  auto launch_waves = [&](void (*kernel)(ValueArgs), int64_t n_waves) {
    hipLaunchKernelGGL(kernel,
                       dim3((unsigned)wave_grid(n_waves, WAVES_PER_BLOCK_VAL)),
                       dim3(WAVES_PER_BLOCK_VAL * WAVE), 0, stream, args);
  };
  if (sequential) {
    const int64_t pairs = args.E * args.A;
    if (pairs == 0) return;
    args.pair_list = nullptr;
    args.n_pairs = pairs;
    launch_waves(value_update_seq_kernel, pairs);
    return;
  }
  if (kobs.numel() > 0) {
    // kobs self-selection: no host-side pair lists, no stream sync — the
    // kernels each cover every pair and act only on their class (k=0 base,
    // k=1, k>=2 table kd1/kd2, k>=2 hash, k>=2 union-merge)
    args.kobs = kobs.data_ptr<int32_t>();
    args.n_pairs = kobs.numel();
    const bool lists = list_count.numel() > 0;
    if (lists) {
      CHECK_GPU(pair_lists);
      CHECK_GPU(list_count);
      TORCH_CHECK(pair_lists.scalar_type() == torch::kInt32 &&
                      list_count.scalar_type() == torch::kInt32,
                  "pair_lists and list_count must be int32");
      TORCH_CHECK(pair_lists.numel() >= args.n_pairs && list_count.numel() >= 2,
                  "pair_lists holds E*A pairs, list_count two counters");
      TORCH_CHECK(args.n_pairs <= INT32_MAX, "pair lists index pairs with int32");
      TORCH_CHECK(list_grid >= 1, "list_grid must be positive");
      args.pair_lists = pair_lists.data_ptr<int32_t>();
      args.list_count = list_count.data_ptr<int>();
    }
    // in list mode kd1 also classifies, so it runs without k-tables too
    const bool kd1 = lists || args.tab_excl != nullptr;
    if (thread_merge) {
      hipLaunchKernelGGL(value_update_thread_kernel,
                         dim3((unsigned)((args.n_pairs + 255) / 256)), dim3(256), 0,
                         stream, args, kd1);
    } else {
      launch_threads(value_base_draw_kernel);
      launch_threads(value_update_k1_kernel);
      if (kd1) launch_threads(value_update_kd1_kernel);
    }
    if (args.tab2_excl != nullptr)
      launch_waves(value_update_kd2_kernel, (args.n_pairs + 7) / 8);
    // list mode: a wave per listed pair, at most list_grid blocks that stride
    const int64_t n_waves =
        lists ? std::min(args.n_pairs, list_grid * WAVES_PER_BLOCK_VAL)
              : (args.n_pairs + VAL_STRIDE - 1) / VAL_STRIDE;
    launch_waves(value_update_kernel_t<1>, n_waves);
    launch_waves(value_update_kernel_t<2>, n_waves);
    return;
  }
  // explicit pair lists (tests / special cases)
  auto use_list = [&](const torch::Tensor& pairs) {
    args.pair_list = pairs.data_ptr<int64_t>();
    args.n_pairs = pairs.numel();
    return args.n_pairs > 0;
  };
  if (use_list(base_pairs)) launch_threads(value_base_draw_kernel);
  if (use_list(k1_pairs)) launch_threads(value_update_k1_kernel);
  if (use_list(wave_pairs)) launch_waves(value_update_kernel_t<0>, args.n_pairs);
}

void value_update_lists(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor ent_rec_idx, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor log_phi,
    torch::Tensor norm_lin, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor phi_prob, torch::Tensor phi_alias, torch::Tensor pow_prob,
    torch::Tensor pow_alias, torch::Tensor pow_off, torch::Tensor log_pow_total,
    torch::Tensor attr_const, int64_t Kc, int64_t collapsed, int64_t sequential,
    int64_t seed, int64_t iteration, int64_t ent_id_base, torch::Tensor error_count,
    torch::Tensor wave_pairs, torch::Tensor base_pairs, torch::Tensor k1_pairs,
    torch::Tensor csr_excl, torch::Tensor csr_rawsum, torch::Tensor z1,
    torch::Tensor ctrl, torch::Tensor kobs, torch::Tensor pair_lists,
    torch::Tensor list_count, int64_t list_grid) {
  value_update_run(rec_values, rec_dist, rec_file, ent_rec_ptr, ent_rec_idx, ent_values,
                   theta, phi, log_phi, norm_lin, log_norm, voff, csr_row_ptr,
                   csr_col, csr_sim, phi_prob, phi_alias, pow_prob, pow_alias,
                   pow_off, log_pow_total, attr_const, Kc, collapsed, sequential,
                   seed, iteration, ent_id_base, error_count, wave_pairs,
                   base_pairs, k1_pairs, csr_excl, csr_rawsum, z1, ctrl, kobs,
                   pair_lists, list_count, list_grid, false);
}

// value_update_lists with the kobs mode's three thread-per-pair kernels as
// one launch (value_update_thread_kernel); same draws.
void value_update_merged(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor ent_rec_idx, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor log_phi,
    torch::Tensor norm_lin, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor phi_prob, torch::Tensor phi_alias, torch::Tensor pow_prob,
    torch::Tensor pow_alias, torch::Tensor pow_off, torch::Tensor log_pow_total,
    torch::Tensor attr_const, int64_t Kc, int64_t collapsed, int64_t sequential,
    int64_t seed, int64_t iteration, int64_t ent_id_base, torch::Tensor error_count,
    torch::Tensor wave_pairs, torch::Tensor base_pairs, torch::Tensor k1_pairs,
    torch::Tensor csr_excl, torch::Tensor csr_rawsum, torch::Tensor z1,
    torch::Tensor ctrl, torch::Tensor kobs, torch::Tensor pair_lists,
    torch::Tensor list_count, int64_t list_grid) {
  value_update_run(rec_values, rec_dist, rec_file, ent_rec_ptr, ent_rec_idx, ent_values,
                   theta, phi, log_phi, norm_lin, log_norm, voff, csr_row_ptr,
                   csr_col, csr_sim, phi_prob, phi_alias, pow_prob, pow_alias,
                   pow_off, log_pow_total, attr_const, Kc, collapsed, sequential,
                   seed, iteration, ent_id_base, error_count, wave_pairs,
                   base_pairs, k1_pairs, csr_excl, csr_rawsum, z1, ctrl, kobs,
                   pair_lists, list_count, list_grid, true);
}

void value_update(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor ent_rec_idx, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor log_phi,
    torch::Tensor norm_lin, torch::Tensor log_norm, torch::Tensor voff,
    torch::Tensor csr_row_ptr, torch::Tensor csr_col, torch::Tensor csr_sim,
    torch::Tensor phi_prob, torch::Tensor phi_alias, torch::Tensor pow_prob,
    torch::Tensor pow_alias, torch::Tensor pow_off, torch::Tensor log_pow_total,
    torch::Tensor attr_const, int64_t Kc, int64_t collapsed, int64_t sequential,
    int64_t seed, int64_t iteration, int64_t ent_id_base, torch::Tensor error_count,
    torch::Tensor wave_pairs, torch::Tensor base_pairs, torch::Tensor k1_pairs,
    torch::Tensor csr_excl, torch::Tensor csr_rawsum, torch::Tensor z1,
    torch::Tensor ctrl, torch::Tensor kobs) {
  value_update_lists(rec_values, rec_dist, rec_file, ent_rec_ptr, ent_rec_idx,
                     ent_values, theta, phi, log_phi, norm_lin, log_norm, voff,
                     csr_row_ptr, csr_col, csr_sim, phi_prob, phi_alias, pow_prob,
                     pow_alias, pow_off, log_pow_total, attr_const, Kc, collapsed,
                     sequential, seed, iteration, ent_id_base, error_count,
                     wave_pairs, base_pairs, k1_pairs, csr_excl, csr_rawsum, z1,
                     ctrl, kobs, torch::Tensor(), torch::Tensor(), 0);
}

void distortion_update(
    torch::Tensor rec_values, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor rec_gid, torch::Tensor rec_ent, torch::Tensor ent_values,
    torch::Tensor theta, torch::Tensor phi, torch::Tensor norm_lin,
    torch::Tensor self_expsim, torch::Tensor voff, torch::Tensor attr_const,
    int64_t seed, int64_t iteration, torch::Tensor ctrl, torch::Tensor log_phi,
    torch::Tensor log_norm, torch::Tensor csr_row_ptr, torch::Tensor csr_col,
    torch::Tensor csr_sim, torch::Tensor loglik) {
  const int64_t* ctrl_ptr = ctrl.numel() ? ctrl.data_ptr<int64_t>() : nullptr;
  const bool fuse = loglik.numel() > 0;
  TORCH_CHECK(!fuse || loglik.numel() >= 256, "loglik buffer must have 256 slots");
  const int64_t R = rec_values.size(0);
  const int A = (int)rec_values.size(1);
  const int F = (int)theta.size(1);
  const int64_t E = fuse ? ent_values.size(0) : 0;
  if (R == 0) return;
  const int64_t total = (E + R) * A;
  dim3 grid((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(distortion_update_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     rec_values.data_ptr<int32_t>(), rec_dist.data_ptr<uint8_t>(),
                     rec_file.data_ptr<int32_t>(), rec_gid.data_ptr<int64_t>(),
                     rec_ent.data_ptr<int64_t>(), ent_values.data_ptr<int32_t>(),
                     theta.data_ptr<float>(), phi.data_ptr<float>(),
                     norm_lin.data_ptr<float>(), self_expsim.data_ptr<float>(),
                     voff.data_ptr<int64_t>(), attr_const.data_ptr<uint8_t>(),
                     R, A, F, (uint64_t)seed, (uint32_t)iteration, ctrl_ptr,
                     log_phi.data_ptr<float>(), log_norm.data_ptr<float>(),
                     csr_row_ptr.data_ptr<int64_t>(), csr_col.data_ptr<int32_t>(),
                     csr_sim.data_ptr<float>(), E,
                     fuse ? loglik.data_ptr<double>() : nullptr);
}

void summary_loglik(
    torch::Tensor ent_values, torch::Tensor rec_values, torch::Tensor rec_dist,
    torch::Tensor rec_ent, torch::Tensor log_phi, torch::Tensor log_norm,
    torch::Tensor voff, torch::Tensor csr_row_ptr, torch::Tensor csr_col,
    torch::Tensor csr_sim, torch::Tensor attr_const, torch::Tensor out) {
  TORCH_CHECK(out.numel() >= 256, "loglik buffer must have 256 slots");
  const int64_t E = ent_values.size(0);
  const int64_t R = rec_values.size(0);
  const int A = (int)ent_values.size(1);
  const int64_t total = (E + R) * A;
  if (total == 0) return;
  dim3 grid((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(summary_loglik_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_values.data_ptr<int32_t>(), rec_values.data_ptr<int32_t>(),
                     rec_dist.data_ptr<uint8_t>(), rec_ent.data_ptr<int64_t>(),
                     log_phi.data_ptr<float>(), log_norm.data_ptr<float>(),
                     voff.data_ptr<int64_t>(), csr_row_ptr.data_ptr<int64_t>(),
                     csr_col.data_ptr<int32_t>(), csr_sim.data_ptr<float>(),
                     attr_const.data_ptr<uint8_t>(), E, R, A,
                     out.data_ptr<double>());
}

void build_keys(torch::Tensor ent_part, torch::Tensor ent_values,
                torch::Tensor rec_part, torch::Tensor rec_values,
                torch::Tensor pair_a1, torch::Tensor pair_a2,
                torch::Tensor pair_v2, int64_t Vmax,
                torch::Tensor ekeys, torch::Tensor qkeys) {
  const int64_t E = ent_values.size(0);
  const int64_t R = rec_values.size(0);
  const int A = (int)ent_values.size(1);
  const int NP = (int)pair_a1.numel();
  const int64_t total = (E + R) * (A + NP);
  if (total == 0) return;
  dim3 grid((unsigned)((total + 255) / 256));
  hipLaunchKernelGGL(build_keys_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_part.data_ptr<int32_t>(), ent_values.data_ptr<int32_t>(),
                     rec_part.data_ptr<int32_t>(), rec_values.data_ptr<int32_t>(),
                     pair_a1.data_ptr<int32_t>(), pair_a2.data_ptr<int32_t>(),
                     pair_v2.data_ptr<int32_t>(),
                     E, R, A, NP, Vmax, ekeys.data_ptr<int64_t>(),
                     qkeys.data_ptr<int64_t>());
}

void summary_counts(torch::Tensor rec_dist, torch::Tensor rec_file,
                    torch::Tensor ent_rec_ptr, int64_t E, torch::Tensor counts,
                    torch::Tensor loglik, torch::Tensor packed,
                    torch::Tensor err) {
  const int64_t R = rec_dist.size(0);
  const int A = (int)rec_dist.size(1);
  const int F = (int)((counts.numel() - 1 - (A + 1)) / A);
  const int64_t total = E + R;
  const int n_counts = (int)counts.numel();
  // err (int32 [1], may be empty) lands in one extra slot past the counts
  const bool with_err = err.numel() > 0;
  TORCH_CHECK(packed.numel() >= 1 + n_counts + (with_err ? 1 : 0),
              "packed summary buffer too small");
  if (total > 0) {
    dim3 grid((unsigned)((total + 255) / 256));
    hipLaunchKernelGGL(summary_counts_kernel, grid, dim3(256),
                       n_counts * sizeof(unsigned int),
                       at::cuda::getCurrentCUDAStream(),
                       rec_dist.data_ptr<uint8_t>(), rec_file.data_ptr<int32_t>(),
                       ent_rec_ptr.data_ptr<int64_t>(), E, R, A, F, n_counts,
                       (unsigned long long*)counts.data_ptr<int64_t>());
  }
  dim3 g2((unsigned)((n_counts + 255) / 256));
  hipLaunchKernelGGL(summary_finalize_kernel, g2, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     loglik.data_ptr<double>(),
                     (const unsigned long long*)counts.data_ptr<int64_t>(),
                     n_counts, with_err ? err.data_ptr<int>() : nullptr,
                     packed.data_ptr<double>());
}

// Exclusive prefix of int32 counts [n] into ptr [n + 1] (int64), with an
// optional int32 cursor [n] = ptr[:n]: one block up to SCAN_SINGLE_MAX
// counters, cumsum (+ copy) above. With `clear`, counts is all zero on
// return (inside the one-block scan; by a fill after cumsum above it).
void scan_excl(torch::Tensor counts, torch::Tensor ptr, torch::Tensor cursor,
               bool clear) {
  CHECK_GPU(counts);
  CHECK_CONTIG(counts);
  CHECK_CONTIG(ptr);
  CHECK_CONTIG(cursor);
  const int64_t n = counts.numel();
  TORCH_CHECK(counts.scalar_type() == torch::kInt32 &&
              ptr.scalar_type() == torch::kInt64, "scan_excl: int32 -> int64");
  TORCH_CHECK(ptr.numel() == n + 1, "scan_excl: ptr must hold n + 1 entries");
  const bool with_cursor = cursor.numel() > 0;
  TORCH_CHECK(!with_cursor || (cursor.numel() == n &&
                               cursor.scalar_type() == torch::kInt32),
              "scan_excl: cursor must be int32 [n]");
  if (n <= SCAN_SINGLE_MAX) {
    const auto misaligned = [](const void* p) {
      return (reinterpret_cast<uintptr_t>(p) & 15) != 0;
    };
    const bool vec = !misaligned(counts.data_ptr()) && !misaligned(ptr.data_ptr()) &&
                     !(with_cursor && misaligned(cursor.data_ptr()));
    hipLaunchKernelGGL(scan_excl_kernel, dim3(1), dim3(GL_THREADS), 0,
                       at::cuda::getCurrentCUDAStream(),
                       counts.data_ptr<int32_t>(), n, ptr.data_ptr<int64_t>(),
                       with_cursor ? cursor.data_ptr<int32_t>() : nullptr, vec,
                       clear);
    return;
  }
  ptr.narrow(0, 0, 1).zero_();
  auto tail = ptr.narrow(0, 1, n);
  at::cumsum_out(tail, counts, 0, torch::kInt64);
  if (with_cursor) cursor.copy_(ptr.narrow(0, 0, n));
  if (clear) counts.zero_();
}

// Entity -> records CSR in stable order, the kobs counts and the store of
// the new links, from zeroed counters (left zeroed: ent_cnt; filled: kobs).
void ent_csr_build(torch::Tensor rec_ent_new, torch::Tensor rec_values,
                   torch::Tensor rec_ent, torch::Tensor ent_cnt,
                   torch::Tensor kobs, torch::Tensor ent_rec_ptr,
                   torch::Tensor ent_rec_idx) {
  CHECK_GPU(rec_ent_new);
  CHECK_CONTIG(rec_ent_new);
  CHECK_CONTIG(rec_values);
  CHECK_CONTIG(rec_ent);
  CHECK_CONTIG(ent_cnt);
  CHECK_CONTIG(kobs);
  CHECK_CONTIG(ent_rec_idx);
  const int64_t R = rec_values.size(0);
  const int A = (int)rec_values.size(1);
  const int64_t E = ent_cnt.numel();
  TORCH_CHECK(rec_ent_new.numel() == R && ent_rec_idx.numel() == R &&
              ent_rec_ptr.numel() == E + 1 && kobs.numel() == E * A,
              "ent_csr_build: shape mismatch");
  TORCH_CHECK(rec_ent.numel() == 0 || rec_ent.numel() == R,
              "ent_csr_build: rec_ent must be empty or [R]");
  auto stream = at::cuda::getCurrentCUDAStream();
  const dim3 rgrid((unsigned)((R + 255) / 256));
  if (R > 0)
    hipLaunchKernelGGL(csr_count_kernel, rgrid, dim3(256), 0, stream,
                       rec_ent_new.data_ptr<int64_t>(),
                       rec_values.data_ptr<int32_t>(), R, A,
                       rec_ent.numel() ? rec_ent.data_ptr<int64_t>() : nullptr,
                       ent_cnt.data_ptr<int32_t>(), kobs.data_ptr<int32_t>());
  scan_excl(ent_cnt, ent_rec_ptr, ent_cnt.narrow(0, 0, 0), false);  // no cursor
  if (R == 0) return;
  hipLaunchKernelGGL(csr_scatter_kernel, rgrid, dim3(256), 0, stream,
                     rec_ent_new.data_ptr<int64_t>(),
                     ent_rec_ptr.data_ptr<int64_t>(), R,
                     ent_cnt.data_ptr<int32_t>(),
                     ent_rec_idx.data_ptr<int64_t>());
  hipLaunchKernelGGL(csr_order_kernel,
                     dim3((unsigned)((E + CSR_ORDER_THREADS - 1) / CSR_ORDER_THREADS)),
                     dim3(CSR_ORDER_THREADS), 0, stream,
                     rec_ent_new.data_ptr<int64_t>(),
                     ent_rec_ptr.data_ptr<int64_t>(), E, R,
                     ent_rec_idx.data_ptr<int64_t>());
}

int64_t resort_max_parts() { return RESORT_MAX_PARTS; }

static int64_t resort_tiles(int64_t E) { return (E + GL_THREADS - 1) / GL_THREADS; }

// Histogram counters partition_resort needs for E entities in P partitions
// (its scanned bases take one more).
int64_t resort_hist_size(int64_t E, int64_t P) { return P * resort_tiles(E); }

// The scatter scans the tile histograms in its own prologue while they fit
// RESORT_SCAN_MAX counters; DBLINK_RESORT_SCAN=0 keeps the scan a launch of
// its own at every size (A/B; results are identical). Re-read per launch.
static bool resort_scan_fused() {
  const char* e = std::getenv("DBLINK_RESORT_SCAN");
  return e ? std::atoi(e) != 0 : true;
}

// Operands of the re-sort launches, checked and unpacked in one place.
struct ResortArgs {
  int64_t E, R, n_tiles;
  int A, P;
};

static ResortArgs make_resort_args(
    const torch::Tensor& ent_values, const torch::Tensor& ent_part,
    const torch::Tensor& rec_ent, int64_t P, const torch::Tensor& hist,
    const torch::Tensor& tile_base, const torch::Tensor& inv,
    const torch::Tensor& out_ent_part, const torch::Tensor& out_ent_values,
    const torch::Tensor& out_rec_ent, const torch::Tensor& out_rec_part,
    const torch::Tensor& ent_ptr) {
  CHECK_GPU(ent_values);
  CHECK_CONTIG(ent_values);
  CHECK_CONTIG(ent_part);
  CHECK_CONTIG(rec_ent);
  CHECK_CONTIG(hist);
  CHECK_CONTIG(tile_base);
  CHECK_CONTIG(out_ent_part);
  CHECK_CONTIG(out_ent_values);
  CHECK_CONTIG(out_rec_ent);
  CHECK_CONTIG(out_rec_part);
  ResortArgs r;
  r.E = ent_values.size(0);
  r.A = (int)ent_values.size(1);
  r.R = rec_ent.numel();
  r.P = (int)P;
  TORCH_CHECK(P >= 1 && P <= RESORT_MAX_PARTS, "partition_resort supports 1..",
              RESORT_MAX_PARTS, " partitions");
  TORCH_CHECK(r.E >= 1 && r.E <= INT32_MAX,
              "partition_resort: entity count out of range");
  r.n_tiles = resort_tiles(r.E);
  TORCH_CHECK(hist.numel() == P * r.n_tiles && tile_base.numel() == P * r.n_tiles + 1 &&
              inv.numel() == r.E && ent_ptr.numel() == P + 1 &&
              ent_part.numel() == r.E && out_ent_part.numel() == r.E &&
              out_ent_values.numel() == r.E * r.A && out_rec_ent.numel() == r.R &&
              out_rec_part.numel() == r.R,
              "partition_resort: shape mismatch");
  TORCH_CHECK(hist.scalar_type() == torch::kInt32 &&
              tile_base.scalar_type() == torch::kInt64,
              "partition_resort: hist int32, tile_base int64");
  return r;
}

// Scan of hist into tile_base and the stable scatter: one launch while the
// counters fit the scatter's prologue, the one-block scan and the scatter
// above that (or with the switch off).
static void resort_scan_scatter(
    const ResortArgs& r, torch::Tensor ent_values, torch::Tensor ent_part,
    torch::Tensor hist, torch::Tensor tile_base, torch::Tensor inv,
    torch::Tensor out_ent_part, torch::Tensor out_ent_values, torch::Tensor ent_ptr) {
  auto stream = at::cuda::getCurrentCUDAStream();
  if (hist.numel() <= RESORT_SCAN_MAX && resort_scan_fused()) {
    const bool vec = (reinterpret_cast<uintptr_t>(hist.data_ptr()) & 15) == 0;
    hipLaunchKernelGGL(resort_scan_scatter_kernel, dim3((unsigned)r.n_tiles),
                       dim3(GL_THREADS), 0, stream, ent_part.data_ptr<int32_t>(),
                       ent_values.data_ptr<int32_t>(), hist.data_ptr<int32_t>(), vec,
                       tile_base.data_ptr<int64_t>(), r.E, r.A, r.P, r.n_tiles,
                       out_ent_part.data_ptr<int32_t>(),
                       out_ent_values.data_ptr<int32_t>(), inv.data_ptr<int32_t>(),
                       ent_ptr.data_ptr<int64_t>());
    return;
  }
  scan_excl(hist, tile_base, hist.narrow(0, 0, 0), false);  // no cursor
  hipLaunchKernelGGL(resort_scatter_kernel, dim3((unsigned)r.n_tiles),
                     dim3(GL_THREADS), 0, stream, ent_part.data_ptr<int32_t>(),
                     ent_values.data_ptr<int32_t>(), tile_base.data_ptr<int64_t>(),
                     r.E, r.A, r.P, r.n_tiles, out_ent_part.data_ptr<int32_t>(),
                     out_ent_values.data_ptr<int32_t>(), inv.data_ptr<int32_t>(),
                     ent_ptr.data_ptr<int64_t>());
}

// KD descent + stable re-sort of the entities by partition id into the other
// buffer set, the record remap, and the next sweep's partition offsets.
// ent_part receives the unsorted new partition ids (as kd_descent + copy did).
void partition_resort(
    torch::Tensor ent_values, torch::Tensor ent_part, torch::Tensor rec_ent,
    torch::Tensor node_kind, torch::Tensor node_attr, torch::Tensor node_a,
    torch::Tensor node_b, torch::Tensor rset, int64_t P,
    torch::Tensor hist, torch::Tensor tile_base, torch::Tensor inv,
    torch::Tensor out_ent_part, torch::Tensor out_ent_values,
    torch::Tensor out_rec_ent, torch::Tensor out_rec_part,
    torch::Tensor ent_ptr) {
  const ResortArgs r = make_resort_args(ent_values, ent_part, rec_ent, P, hist,
                                        tile_base, inv, out_ent_part, out_ent_values,
                                        out_rec_ent, out_rec_part, ent_ptr);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(resort_hist_kernel, dim3((unsigned)r.n_tiles), dim3(GL_THREADS),
                     0, stream, ent_values.data_ptr<int32_t>(),
                     node_kind.data_ptr<int32_t>(), node_attr.data_ptr<int32_t>(),
                     node_a.data_ptr<int32_t>(), node_b.data_ptr<int32_t>(),
                     rset.data_ptr<int32_t>(), r.E, r.A, r.P, r.n_tiles,
                     ent_part.data_ptr<int32_t>(), hist.data_ptr<int32_t>());
  resort_scan_scatter(r, ent_values, ent_part, hist, tile_base, inv, out_ent_part,
                      out_ent_values, ent_ptr);
  if (r.R > 0)
    hipLaunchKernelGGL(resort_remap_kernel, dim3((unsigned)((r.R + 255) / 256)),
                       dim3(256), 0, stream, rec_ent.data_ptr<int64_t>(),
                       inv.data_ptr<int32_t>(), ent_part.data_ptr<int32_t>(), r.R,
                       out_rec_ent.data_ptr<int64_t>(),
                       out_rec_part.data_ptr<int32_t>());
}

// Single-rank sweep tail: partition_resort and summary_counts (same operands,
// same results) in three launches. The summary counts ride with the tile
// histograms and the summary pack with the record remap: neither reads what
// the re-sort writes. counts must be zero on entry, as for summary_counts.
void sweep_tail(
    torch::Tensor ent_values, torch::Tensor ent_part, torch::Tensor rec_ent,
    torch::Tensor node_kind, torch::Tensor node_attr, torch::Tensor node_a,
    torch::Tensor node_b, torch::Tensor rset, int64_t P,
    torch::Tensor hist, torch::Tensor tile_base, torch::Tensor inv,
    torch::Tensor out_ent_part, torch::Tensor out_ent_values,
    torch::Tensor out_rec_ent, torch::Tensor out_rec_part,
    torch::Tensor ent_ptr, torch::Tensor rec_dist, torch::Tensor rec_file,
    torch::Tensor ent_rec_ptr, torch::Tensor counts, torch::Tensor loglik,
    torch::Tensor packed, torch::Tensor err) {
  const ResortArgs r = make_resort_args(ent_values, ent_part, rec_ent, P, hist,
                                        tile_base, inv, out_ent_part, out_ent_values,
                                        out_rec_ent, out_rec_part, ent_ptr);
  CHECK_CONTIG(rec_dist);
  CHECK_CONTIG(rec_file);
  CHECK_CONTIG(ent_rec_ptr);
  CHECK_CONTIG(counts);
  const int n_counts = (int)counts.numel();
  const int F = (n_counts - 1 - (r.A + 1)) / r.A;
  const bool with_err = err.numel() > 0;
  TORCH_CHECK(rec_dist.size(0) == r.R && rec_dist.size(1) == r.A &&
              rec_file.numel() == r.R && ent_rec_ptr.numel() == r.E + 1 &&
              F >= 1 && n_counts == 1 + r.A * F + r.A + 1 && loglik.numel() >= 256,
              "sweep_tail: summary shape mismatch");
  TORCH_CHECK(packed.numel() >= 1 + n_counts + (with_err ? 1 : 0),
              "packed summary buffer too small");
  auto stream = at::cuda::getCurrentCUDAStream();
  const int64_t count_blocks = (r.E + r.R + GL_THREADS - 1) / GL_THREADS;
  const size_t lds = sizeof(unsigned int) * (size_t)std::max(r.P, n_counts);
  TORCH_CHECK(lds <= 48 * 1024, "sweep_tail: too many summary counters");
  hipLaunchKernelGGL(resort_hist_counts_kernel,
                     dim3((unsigned)(r.n_tiles + count_blocks)), dim3(GL_THREADS), lds,
                     stream, ent_values.data_ptr<int32_t>(),
                     node_kind.data_ptr<int32_t>(), node_attr.data_ptr<int32_t>(),
                     node_a.data_ptr<int32_t>(), node_b.data_ptr<int32_t>(),
                     rset.data_ptr<int32_t>(), r.E, r.A, r.P, r.n_tiles,
                     ent_part.data_ptr<int32_t>(), hist.data_ptr<int32_t>(),
                     rec_dist.data_ptr<uint8_t>(), rec_file.data_ptr<int32_t>(),
                     ent_rec_ptr.data_ptr<int64_t>(), r.R, F, n_counts,
                     (unsigned long long*)counts.data_ptr<int64_t>());
  resort_scan_scatter(r, ent_values, ent_part, hist, tile_base, inv, out_ent_part,
                      out_ent_values, ent_ptr);
  hipLaunchKernelGGL(resort_remap_finalize_kernel,
                     dim3((unsigned)(1 + (r.R + 255) / 256)), dim3(256), 0, stream,
                     rec_ent.data_ptr<int64_t>(), inv.data_ptr<int32_t>(),
                     ent_part.data_ptr<int32_t>(), r.R,
                     out_rec_ent.data_ptr<int64_t>(),
                     out_rec_part.data_ptr<int32_t>(), loglik.data_ptr<double>(),
                     (const unsigned long long*)counts.data_ptr<int64_t>(), n_counts,
                     with_err ? err.data_ptr<int>() : nullptr,
                     packed.data_ptr<double>());
}

void kd_descent(
    torch::Tensor ent_values, torch::Tensor node_kind, torch::Tensor node_attr,
    torch::Tensor node_a, torch::Tensor node_b, torch::Tensor rset,
    torch::Tensor ent_part_out) {
  const int64_t E = ent_values.size(0);
  const int A = (int)ent_values.size(1);
  if (E == 0) return;
  dim3 grid((unsigned)((E + 255) / 256));
  hipLaunchKernelGGL(kd_descent_kernel, grid, dim3(256), 0,
                     at::cuda::getCurrentCUDAStream(),
                     ent_values.data_ptr<int32_t>(), node_kind.data_ptr<int32_t>(),
                     node_attr.data_ptr<int32_t>(), node_a.data_ptr<int32_t>(),
                     node_b.data_ptr<int32_t>(), rset.data_ptr<int32_t>(), E, A,
                     ent_part_out.data_ptr<int32_t>());
}

// One pass (count or fill) of a K1 sweep's operands, whatever the metric;
// shapes are on sim_pairs_kernel's parameter list.
struct SimSweep {
  const void* strs;
  const int32_t *lens, *len_order;
  const int64_t* len_ptr;
  int max_len;
  int64_t* row_counts;
  int32_t* out_col;
  float* out_expsim;
  int64_t* fill_pos;
  int fill;
};

// What a sweep scores with: launch_sim_class is overloaded on these.
struct EditMetric {
  float threshold, max_sim;
  bool transpositions;  // OSA instead of Levenshtein
};

template <typename Sym, int W, int WAVES>
static void launch_sim_class(const SimSweep& s, const EditMetric& m, int64_t row_begin,
                             int64_t row_end) {
  if (row_end <= row_begin) return;
  dim3 grid((unsigned)wave_grid(row_end - row_begin, WAVES));
  const auto kernel = m.transpositions ? sim_pairs_kernel<Sym, W, WAVES, true>
                                       : sim_pairs_kernel<Sym, W, WAVES, false>;
  hipLaunchKernelGGL(kernel, grid, dim3(WAVES * WAVE), 0,
                     at::cuda::getCurrentCUDAStream(),
                     static_cast<const Sym*>(s.strs), s.lens, s.len_order, s.len_ptr,
                     row_begin, row_end, s.max_len, m.threshold, m.max_sim,
                     s.row_counts, s.out_col, s.out_expsim, s.fill_pos, s.fill);
}

template <typename Sym, int W, int WAVES>
static void launch_sim_class(const SimSweep& s, const JaroScale& m, int64_t row_begin,
                             int64_t row_end) {
  if (row_end <= row_begin) return;
  dim3 grid((unsigned)wave_grid(row_end - row_begin, WAVES));
  hipLaunchKernelGGL((jaro_pairs_kernel<Sym, W, WAVES>), grid, dim3(WAVES * WAVE), 0,
                     at::cuda::getCurrentCUDAStream(),
                     static_cast<const Sym*>(s.strs), s.lens, s.len_order, s.len_ptr,
                     row_begin, row_end, s.max_len, m,
                     s.row_counts, s.out_col, s.out_expsim, s.fill_pos, s.fill);
}

// One kernel instance per row-length class; class_ptr[k] is the first
// len_order position whose length exceeds 64*k.
template <typename Sym, typename Metric>
static void launch_sim_sweep(const SimSweep& s, const Metric& m, const int64_t (&class_ptr)[5]) {
  constexpr int WIDE = sizeof(Sym) == 1 ? SP_WAVES : SP_WAVES_WIDE;
  launch_sim_class<Sym, 1, SP_WAVES>(s, m, class_ptr[0], class_ptr[1]);
  launch_sim_class<Sym, 2, SP_WAVES>(s, m, class_ptr[1], class_ptr[2]);
  launch_sim_class<Sym, 3, WIDE>(s, m, class_ptr[2], class_ptr[3]);
  launch_sim_class<Sym, 4, WIDE>(s, m, class_ptr[3], class_ptr[4]);
}

// The host side of a K1 sweep, shared by the metrics: operand checks, length
// order and buckets, class boundaries, then a count pass, the CSR allocation
// and a fill pass. `who` names the entry point in error messages.
template <typename Metric>
static std::vector<torch::Tensor> sim_sweep_gpu(torch::Tensor strs, torch::Tensor lens,
                                                const Metric& metric, const char* who) {
  CHECK_GPU(strs);
  CHECK_GPU(lens);
  TORCH_CHECK(strs.dim() == 2 && strs.is_contiguous(), "strs must be a contiguous [V, stride] tensor");
  const bool wide = strs.scalar_type() == torch::kInt16 || strs.scalar_type() == torch::kUInt16;
  TORCH_CHECK(wide || strs.scalar_type() == torch::kUInt8,
              "strs must hold uint8 symbols or 16-bit symbol ids (int16 storage)");
  TORCH_CHECK(lens.scalar_type() == torch::kInt32 && lens.is_contiguous() &&
              lens.numel() == strs.size(0), "lens must be a contiguous int32 [V] tensor");
  const int V = (int)strs.size(0);
  const int max_len = (int)strs.size(1);
  TORCH_CHECK(max_len <= SP_MAX_LEN, who, ": row stride ", max_len,
              " exceeds the GPU sweep's limit of ", SP_MAX_LEN,
              " symbols per value (longer domains take the CPU pass)");
  auto opts_i64 = torch::TensorOptions().dtype(torch::kInt64).device(strs.device());
  // length buckets: candidates for value i live in a contiguous window of
  // the length-sorted order
  auto lens64 = lens.to(torch::kInt64);
  auto len_order = torch::argsort(lens64, /*stable=*/true).to(torch::kInt32).contiguous();
  auto sorted_lens = std::get<0>(torch::sort(lens64));
  auto len_ptr = torch::searchsorted(
      sorted_lens, torch::arange(max_len + 2, opts_i64), /*out_int32=*/false, /*right=*/false)
      .contiguous();
  // Rows of length 64(k-1)+1 .. 64k form class k (class 1 also holds length
  // 0). A length outside [0, max_len] falls outside every class and every
  // candidate window, so such a row comes back empty instead of being read.
  auto len_ptr_host = len_ptr.cpu();
  const int64_t* lp = len_ptr_host.data_ptr<int64_t>();
  int64_t class_ptr[5];
  class_ptr[0] = lp[0];
  for (int k = 1; k <= 4; ++k) class_ptr[k] = lp[std::min(64 * k, max_len) + 1];

  SimSweep s;
  s.strs = strs.data_ptr();
  s.lens = lens.data_ptr<int32_t>();
  s.len_order = len_order.data_ptr<int32_t>();
  s.len_ptr = len_ptr.data_ptr<int64_t>();
  s.max_len = max_len;
  auto sweep = [&]() {
    if (wide) launch_sim_sweep<uint16_t>(s, metric, class_ptr);
    else launch_sim_sweep<uint8_t>(s, metric, class_ptr);
  };

  auto row_counts = torch::zeros({V}, opts_i64);
  s.row_counts = row_counts.data_ptr<int64_t>();
  s.out_col = nullptr;
  s.out_expsim = nullptr;
  s.fill_pos = nullptr;
  s.fill = 0;
  sweep();
  auto row_ptr = torch::zeros({V + 1}, opts_i64);
  row_ptr.slice(0, 1, V + 1) = torch::cumsum(row_counts, 0);
  auto row_start = row_ptr.slice(0, 0, V).contiguous();
  const int64_t nnz = row_ptr[V].item<int64_t>();
  auto col = torch::empty({nnz}, torch::TensorOptions().dtype(torch::kInt32).device(strs.device()));
  auto expsim = torch::empty({nnz}, torch::TensorOptions().dtype(torch::kFloat32).device(strs.device()));
  auto fill_pos = torch::zeros({V}, opts_i64);
  s.row_counts = row_start.data_ptr<int64_t>();
  s.out_col = col.data_ptr<int32_t>();
  s.out_expsim = expsim.data_ptr<float>();
  s.fill_pos = fill_pos.data_ptr<int64_t>();
  s.fill = 1;
  sweep();
  return {row_ptr, col, expsim};
}

std::vector<torch::Tensor> sim_pairs_gpu(torch::Tensor strs, torch::Tensor lens,
                                         double threshold, double max_sim,
                                         bool transpositions) {
  const EditMetric metric{(float)threshold, (float)max_sim, transpositions};
  return sim_sweep_gpu(strs, lens, metric, "sim_pairs_gpu");
}

// prefix_scale is Winkler's p (0 = plain Jaro); everything else as above.
std::vector<torch::Tensor> jaro_pairs_gpu(torch::Tensor strs, torch::Tensor lens,
                                          double threshold, double max_sim,
                                          double prefix_scale) {
  TORCH_CHECK(prefix_scale >= 0.0 && prefix_scale <= 0.25,
              "prefix_scale must be in [0, 0.25]");
  return sim_sweep_gpu(strs, lens, jaro_scale(threshold, max_sim, prefix_scale),
                       "jaro_pairs_gpu");
}

}  // namespace dblink
