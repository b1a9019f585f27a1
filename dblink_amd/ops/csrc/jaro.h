// Jaro similarity with the Winkler prefix boost: the parts shared by the CPU
// sweep (sim_pairs_cpu.cpp) and the GPU sweep (kernels.hip). No torch here, so
// a stand-alone host program can include it.
//
// Definition (dblink_amd/models/similarity.py holds the oracle):
//   window r = max(max(la, lb) / 2 - 1, 0); greedy matching in string order;
//   m matches, t = (matched characters that differ in order) / 2;
//   jaro = (m/la + m/lb + (m-t)/m) / 3, 1 for two empty strings, 0 for m == 0;
//   unit = jaro + l * p * (1 - jaro), l = common prefix capped at 4, applied
//   only when jaro > 0.7, decided in integers (jaro_boost_gate).
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define JARO_HD __host__ __device__ __forceinline__
#else
#define JARO_HD inline
#endif

namespace dblink {

// Threshold, scale and the conservative length filter of one Jaro sweep.
struct JaroScale {
  double threshold, max_sim, prefix_scale;
  double u0;     // threshold / max_sim
  double scale;  // max_sim / (max_sim - threshold)
};

JARO_HD JaroScale jaro_scale(double threshold, double max_sim, double prefix_scale) {
  JaroScale s;
  s.threshold = threshold;
  s.max_sim = max_sim;
  s.prefix_scale = prefix_scale;
  s.u0 = threshold / max_sim;
  s.scale = max_sim / (max_sim - threshold);
  return s;
}

// With s = min(la, lb), L = max(la, lb): m <= s and t >= 0 give
// jaro <= (2 + s/L) / 3, and the boost adds at most 4p(1 - jaro). A pair can
// be skipped only when that bound does not exceed thr/max; at threshold 0
// (u0 == 0) the bound is positive and nothing is skipped.
JARO_HD bool jaro_length_prunes(const JaroScale& s, int la, int lb) {
  const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
  if (hi == 0) return false;
  const double jmax = (2.0 + (double)lo / (double)hi) / 3.0;
  const double umax = jmax + 4.0 * s.prefix_scale * (1.0 - jmax);
  return umax <= s.u0;
}

// jaro > 0.7 in exact integers:
//   10 * (m*m*(la+lb) + (m-t)*la*lb) > 21 * m*la*lb.
// With m <= min(la, lb) <= 256 every term stays below 2^32 (the largest,
// 21 * 256^3, is about 3.5e8); Int is int64_t on the host, where lengths are
// unbounded.
template <typename Int>
JARO_HD bool jaro_boost_gate(Int m, Int t, Int la, Int lb) {
  return 10 * (m * m * (la + lb) + (m - t) * la * lb) > 21 * m * la * lb;
}

// The truncated, scaled similarity before the max(0, .), in fp64 and in the
// oracle's order of operations, so every implementation takes the same
// inclusion decision. `prefix` is the common-prefix length capped at 4.
template <typename Int>
JARO_HD double jaro_trans(const JaroScale& s, int m, int t, int la, int lb, int prefix) {
#ifdef __clang__
#pragma clang fp contract(off)  // no fused multiply-add: the same bits on host and device
#endif
  double unit;
  if (la == 0 && lb == 0) {
    unit = 1.0;
  } else if (m == 0) {
    unit = 0.0;
  } else {
    const double dm = (double)m;
    unit = (dm / (double)la + dm / (double)lb + (double)(m - t) / dm) / 3.0;
    if (jaro_boost_gate<Int>(m, t, la, lb))
      unit = unit + ((double)prefix * s.prefix_scale) * (1.0 - unit);
  }
  return s.scale * (s.max_sim * unit - s.threshold);
}

// Greedy matching of a (outer) against b on the host. `taken` holds lb bytes,
// `matched` la symbols.
template <typename Sym>
inline void jaro_parts_host(const Sym* a, int la, const Sym* b, int lb,
                            uint8_t* taken, Sym* matched, int* m_out, int* t_out) {
  const int longer = la > lb ? la : lb;
  const int r = longer / 2 - 1 > 0 ? longer / 2 - 1 : 0;
  for (int j = 0; j < lb; ++j) taken[j] = 0;
  int m = 0;
  for (int i = 0; i < la; ++i) {
    const int j0 = i - r > 0 ? i - r : 0;
    const int j1 = i + r + 1 < lb ? i + r + 1 : lb;
    const Sym ca = a[i];
    for (int j = j0; j < j1; ++j) {
      if (!taken[j] && b[j] == ca) {
        taken[j] = 1;
        matched[m++] = ca;
        break;
      }
    }
  }
  int half = 0, k = 0;
  for (int j = 0; j < lb; ++j)
    if (taken[j]) half += matched[k++] != b[j];
  *m_out = m;
  *t_out = half / 2;
}

template <typename Sym>
JARO_HD int jaro_common_prefix(const Sym* a, int la, const Sym* b, int lb) {
  int cap = la < lb ? la : lb;
  if (cap > 4) cap = 4;
  int l = 0;
  while (l < cap && a[l] == b[l]) ++l;
  return l;
}

}  // namespace dblink
