// CPU (OpenMP) banded edit-distance (Levenshtein or OSA) sim-pair sweep over
// an attribute domain.
//
// Replaces the reference's Spark cartesian V x V sweep
// (AttributeIndex.scala:219-231) with a threshold-pruned exact pass:
// sim(a,b) > 0 requires unit(a,b) > thr/max, i.e. edit distance
// d < (|a|+|b|) * (1-u0)/(1+u0), which bounds |len(a)-len(b)| and enables a
// banded DP with early exit. Used at index-build time on the host; the GPU
// variant lives in kernels.hip (sim_pairs_gpu).
//
// jaro_pairs_cpu is the same sweep over the Jaro similarity with the Winkler
// prefix boost (GPU variant: jaro_pairs_gpu).

#include <torch/extension.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "jaro.h"

namespace dblink {

// Edit distance with early exit once every cell of a row exceeds `band`
// (the exact distance is then irrelevant: sim truncates to 0). Attribute
// values are short (tens of symbols; any length is accepted), so a plain
// rolling-array DP with the row-min cutoff is both simple and fast; the big
// win is the caller's length filter. Sym is uint8_t or a 16-bit symbol id.
template <typename Sym>
static int levenshtein_capped(const Sym* a, int la, const Sym* b, int lb,
                              int band, int* scratch) {
  if (la == 0) return lb;
  if (lb == 0) return la;
  int* prev = scratch;
  int* cur = scratch + lb + 1;
  for (int j = 0; j <= lb; ++j) prev[j] = j;
  for (int i = 1; i <= la; ++i) {
    cur[0] = i;
    int row_min = i;
    const Sym ca = a[i - 1];
    for (int j = 1; j <= lb; ++j) {
      const int cost = (ca == b[j - 1]) ? 0 : 1;
      int m = prev[j - 1] + cost;
      const int del = cur[j - 1] + 1;
      const int ins = prev[j] + 1;
      if (del < m) m = del;
      if (ins < m) m = ins;
      cur[j] = m;
      if (m < row_min) row_min = m;
    }
    if (row_min > band) return band + 1;
    std::swap(prev, cur);
  }
  return prev[lb];
}

// Restricted Damerau-Levenshtein (optimal string alignment): the recurrence
// above plus D[i-2][j-2] + 1 where the last two symbols of both prefixes are
// swapped, on three rolling rows of lb + 1 cells.
//
// The single-row early exit stays valid. D is 1-Lipschitz along a row (the
// induction on i goes through with the transposition term), so if every cell
// of row i exceeds `band`, every cell of row i-1 is at least `band`: a cell
// of row i-1 below `band` would put its lower neighbour at or below `band`.
// A transposition into row i+1 reads row i-1 and so yields at least
// band + 1, like the three Levenshtein terms reading row i; every later row
// therefore exceeds `band` too.
template <typename Sym>
static int osa_capped(const Sym* a, int la, const Sym* b, int lb, int band,
                      int* scratch) {
  if (la == 0) return lb;
  if (lb == 0) return la;
  int* prev2 = scratch + 2 * (lb + 1);  // row i-2, first read at i == 2
  int* prev = scratch;
  int* cur = scratch + lb + 1;
  for (int j = 0; j <= lb; ++j) prev[j] = j;
  for (int i = 1; i <= la; ++i) {
    cur[0] = i;
    int row_min = i;
    const Sym ca = a[i - 1];
    for (int j = 1; j <= lb; ++j) {
      const int cost = (ca == b[j - 1]) ? 0 : 1;
      int m = prev[j - 1] + cost;
      const int del = cur[j - 1] + 1;
      const int ins = prev[j] + 1;
      if (del < m) m = del;
      if (ins < m) m = ins;
      if (i > 1 && j > 1 && ca == b[j - 2] && a[i - 2] == b[j - 1]) {
        const int tr = prev2[j - 2] + 1;
        if (tr < m) m = tr;
      }
      cur[j] = m;
      if (m < row_min) row_min = m;
    }
    if (row_min > band) return band + 1;
    int* t = prev2;
    prev2 = prev;
    prev = cur;
    cur = t;
  }
  return prev[lb];
}

// Per-row hit lists to CSR (row_ptr int64, col int32, expsim fp32).
static std::vector<torch::Tensor> rows_to_csr(const std::vector<std::vector<int32_t>>& cols,
                                              const std::vector<std::vector<float>>& sims) {
  const int64_t V = (int64_t)cols.size();
  auto row_ptr = torch::zeros({V + 1}, torch::kInt64);
  int64_t* rp = row_ptr.data_ptr<int64_t>();
  for (int64_t i = 0; i < V; ++i) rp[i + 1] = rp[i] + (int64_t)cols[i].size();
  const int64_t nnz = rp[V];
  auto col = torch::empty({nnz}, torch::kInt32);
  auto expsim = torch::empty({nnz}, torch::kFloat32);
  int32_t* cp = col.data_ptr<int32_t>();
  float* sp = expsim.data_ptr<float>();
#pragma omp parallel for schedule(static)
  for (int64_t i = 0; i < V; ++i) {
    std::copy(cols[i].begin(), cols[i].end(), cp + rp[i]);
    std::copy(sims[i].begin(), sims[i].end(), sp + rp[i]);
  }
  return {row_ptr, col, expsim};
}

template <typename Sym, bool TRANSPOSE>
static std::vector<torch::Tensor> sim_pairs_cpu_impl(torch::Tensor strs, torch::Tensor lens,
                                                     double threshold, double max_sim) {
  const int64_t V = strs.size(0);
  const int64_t max_len = strs.size(1);
  const Sym* S = static_cast<const Sym*>(strs.data_ptr());
  const int32_t* L = lens.data_ptr<int32_t>();
  const double u0 = threshold / max_sim;
  const double scale = max_sim / (max_sim - threshold);

  std::vector<std::vector<int32_t>> cols(V);
  std::vector<std::vector<float>> sims(V);

#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < V; ++i) {
    const Sym* a = S + i * max_len;
    const int la = L[i];
    std::vector<int> scratch((TRANSPOSE ? 3 : 2) * (max_len + 1));
    for (int64_t j = 0; j < V; ++j) {
      const int lb = L[j];
      const int tot = la + lb;
      double unit;
      if (tot == 0) {
        unit = 1.0;
      } else {
        // d < dmax for sim > 0
        const double dmax_f = tot * (1.0 - u0) / (1.0 + u0);
        const int band = (int)std::ceil(dmax_f);
        if (std::abs(la - lb) >= dmax_f) continue;
        const int d = TRANSPOSE
            ? osa_capped(a, la, S + j * max_len, lb, band, scratch.data())
            : levenshtein_capped(a, la, S + j * max_len, lb, band, scratch.data());
        if (d > band) continue;
        unit = 1.0 - 2.0 * (double)d / ((double)tot + d);
      }
      const double trans = scale * (max_sim * unit - threshold);
      // inclusion criterion matches the python oracle exactly: exp(sim) > 1
      // in f64 (knife-edge sims ~1e-17 round exp() to exactly 1.0 and are
      // excluded on both sides; they would carry zero weight anyway)
      const double es = std::exp(trans);
      if (es > 1.0) {
        cols[i].push_back((int32_t)j);
        sims[i].push_back((float)es);
      }
    }
  }

  return rows_to_csr(cols, sims);
}

// strs: [V, stride] uint8 symbols, or 16-bit symbol ids in int16 storage
// (read as uint16_t); id 0 pads either. `transpositions` selects the
// restricted Damerau-Levenshtein (OSA) distance instead of Levenshtein.
std::vector<torch::Tensor> sim_pairs_cpu(torch::Tensor strs, torch::Tensor lens,
                                         double threshold, double max_sim,
                                         bool transpositions) {
  TORCH_CHECK(strs.dim() == 2 && strs.is_contiguous() && !strs.is_cuda());
  TORCH_CHECK(lens.dtype() == torch::kInt32 && lens.is_contiguous() &&
              lens.numel() == strs.size(0));
  if (strs.scalar_type() == torch::kUInt8)
    return transpositions
        ? sim_pairs_cpu_impl<uint8_t, true>(strs, lens, threshold, max_sim)
        : sim_pairs_cpu_impl<uint8_t, false>(strs, lens, threshold, max_sim);
  TORCH_CHECK(strs.scalar_type() == torch::kInt16 || strs.scalar_type() == torch::kUInt16,
              "strs must hold uint8 symbols or 16-bit symbol ids (int16 storage)");
  return transpositions
      ? sim_pairs_cpu_impl<uint16_t, true>(strs, lens, threshold, max_sim)
      : sim_pairs_cpu_impl<uint16_t, false>(strs, lens, threshold, max_sim);
}

// Jaro similarity with the Winkler prefix boost (jaro.h) over every pair the
// conservative length filter lets through; any value length.
template <typename Sym>
static std::vector<torch::Tensor> jaro_pairs_cpu_impl(torch::Tensor strs, torch::Tensor lens,
                                                      const JaroScale& sc) {
  const int64_t V = strs.size(0);
  const int64_t max_len = strs.size(1);
  const Sym* S = static_cast<const Sym*>(strs.data_ptr());
  const int32_t* L = lens.data_ptr<int32_t>();

  std::vector<std::vector<int32_t>> cols(V);
  std::vector<std::vector<float>> sims(V);

#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < V; ++i) {
    const Sym* a = S + i * max_len;
    const int la = L[i];
    std::vector<uint8_t> taken(max_len + 1);
    std::vector<Sym> matched(max_len + 1);
    for (int64_t j = 0; j < V; ++j) {
      const int lb = L[j];
      if (jaro_length_prunes(sc, la, lb)) continue;
      const Sym* b = S + j * max_len;
      int m = 0, t = 0;
      if (la > 0 && lb > 0) jaro_parts_host(a, la, b, lb, taken.data(), matched.data(), &m, &t);
      const int prefix = jaro_common_prefix(a, la, b, lb);
      const double trans = jaro_trans<int64_t>(sc, m, t, la, lb, prefix);
      const double es = std::exp(trans);  // inclusion as in sim_pairs_cpu_impl
      if (es > 1.0) {
        cols[i].push_back((int32_t)j);
        sims[i].push_back((float)es);
      }
    }
  }
  return rows_to_csr(cols, sims);
}

// Same buffers as sim_pairs_cpu; prefix_scale is Winkler's p (0 = plain Jaro).
std::vector<torch::Tensor> jaro_pairs_cpu(torch::Tensor strs, torch::Tensor lens,
                                          double threshold, double max_sim,
                                          double prefix_scale) {
  TORCH_CHECK(strs.dim() == 2 && strs.is_contiguous() && !strs.is_cuda());
  TORCH_CHECK(lens.dtype() == torch::kInt32 && lens.is_contiguous() &&
              lens.numel() == strs.size(0));
  TORCH_CHECK(prefix_scale >= 0.0 && prefix_scale <= 0.25,
              "prefix_scale must be in [0, 0.25]");
  const JaroScale sc = jaro_scale(threshold, max_sim, prefix_scale);
  if (strs.scalar_type() == torch::kUInt8)
    return jaro_pairs_cpu_impl<uint8_t>(strs, lens, sc);
  TORCH_CHECK(strs.scalar_type() == torch::kInt16 || strs.scalar_type() == torch::kUInt16,
              "strs must hold uint8 symbols or 16-bit symbol ids (int16 storage)");
  return jaro_pairs_cpu_impl<uint16_t>(strs, lens, sc);
}

}  // namespace dblink
