// Stand-alone host check of jaro_pairs_cpu (dblink_amd/ops/csrc/sim_pairs_cpu.cpp)
// for sanitizer builds: no Python, no GPU. It sweeps seeded domains of uint8
// and 16-bit symbols (lengths 0..300, ids above 32768) at several thresholds
// and prefix scales and compares every row with a direct evaluation of the
// definition written here independently of jaro.h. Build line: docs/testing.md.

#include <torch/torch.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

namespace dblink {
std::vector<torch::Tensor> jaro_pairs_cpu(torch::Tensor strs, torch::Tensor lens,
                                          double threshold, double max_sim,
                                          double prefix_scale);
}

using Str = std::vector<int>;

static double unit_by_definition(const Str& a, const Str& b, double p) {
  const int la = (int)a.size(), lb = (int)b.size();
  if (la == 0 && lb == 0) return 1.0;
  const int r = std::max(std::max(la, lb) / 2 - 1, 0);
  std::vector<char> used(lb, 0);
  Str ma, mb;
  for (int i = 0; i < la; ++i)
    for (int j = std::max(i - r, 0); j < std::min(i + r + 1, lb); ++j)
      if (!used[j] && b[j] == a[i]) {
        used[j] = 1;
        ma.push_back(a[i]);
        break;
      }
  for (int j = 0; j < lb; ++j)
    if (used[j]) mb.push_back(b[j]);
  const long long m = (long long)ma.size();
  if (m == 0) return 0.0;
  long long half = 0;
  for (size_t k = 0; k < ma.size(); ++k) half += ma[k] != mb[k];
  const long long t = half / 2;
  double unit = ((double)m / la + (double)m / lb + (double)(m - t) / (double)m) / 3.0;
  const long long A = la, B = lb;
  if (10 * (m * m * (A + B) + (m - t) * A * B) > 21 * m * A * B) {
    int l = 0;
    while (l < std::min(4, std::min(la, lb)) && a[l] == b[l]) ++l;
    unit = unit + ((double)l * p) * (1.0 - unit);
  }
  return unit;
}

static std::vector<Str> make_domain(std::mt19937& rng, const std::vector<int>& alphabet) {
  std::vector<Str> out = {{}, {alphabet[0]}, {alphabet[1]}, {alphabet[0], alphabet[1]}};
  auto pick = [&]() { return alphabet[rng() % alphabet.size()]; };
  for (int c = 0; c < 12; ++c) {
    const int n = c == 0 ? 300 : 1 + (int)(rng() % 40);
    Str base(n);
    for (auto& x : base) x = pick();
    out.push_back(base);
    for (int k = 0; k < 4; ++k) {
      Str s = base;
      for (int e = 0; e < 1 + (int)(rng() % 3); ++e) {
        const int pos = (int)(rng() % s.size());
        switch (rng() % 4) {
          case 0: s[pos] = pick(); break;
          case 1: if (s.size() > 1) s.erase(s.begin() + pos); break;
          case 2: if (s.size() < 300) s.insert(s.begin() + pos, pick()); break;
          default: std::swap(s[pos], s[rng() % s.size()]);
        }
      }
      out.push_back(s);
    }
  }
  return out;
}

template <typename Sym>
static long check(const std::vector<Str>& dom, torch::ScalarType dtype, double thr, double p) {
  const int64_t V = (int64_t)dom.size();
  int64_t stride = 1;
  for (const auto& s : dom) stride = std::max<int64_t>(stride, (int64_t)s.size());
  auto strs = torch::zeros({V, stride}, dtype);
  auto lens = torch::zeros({V}, torch::kInt32);
  Sym* S = static_cast<Sym*>(strs.data_ptr());
  for (int64_t v = 0; v < V; ++v) {
    lens.data_ptr<int32_t>()[v] = (int32_t)dom[v].size();
    for (size_t k = 0; k < dom[v].size(); ++k) S[v * stride + k] = (Sym)dom[v][k];
  }
  const double msim = 10.0;
  auto out = dblink::jaro_pairs_cpu(strs, lens, thr, msim, p);
  const int64_t* rp = out[0].data_ptr<int64_t>();
  const int32_t* col = out[1].data_ptr<int32_t>();
  const float* es = out[2].data_ptr<float>();
  long bad = 0;
  for (int64_t i = 0; i < V; ++i) {
    int64_t pos = rp[i];
    for (int64_t j = 0; j < V; ++j) {
      const double unit = unit_by_definition(dom[i], dom[j], p);
      const double e = std::exp(msim / (msim - thr) * (msim * unit - thr));
      if (!(e > 1.0)) continue;
      if (pos >= rp[i + 1] || col[pos] != (int32_t)j ||
          std::fabs((double)es[pos] - e) > 1e-6 * e)
        ++bad;
      ++pos;
    }
    if (pos != rp[i + 1]) ++bad;
  }
  return bad;
}

int main() {
  std::mt19937 rng(2024);
  const std::vector<int> narrow = {1, 2, 3, 4};
  const std::vector<int> wide = {300, 7000, 33000, 50000, 65535};
  long bad = 0;
  for (double thr : {0.0, 1.0, 7.3, 9.0})
    for (double p : {0.0, 0.1, 0.25}) {
      bad += check<uint8_t>(make_domain(rng, narrow), torch::kUInt8, thr, p);
      bad += check<uint16_t>(make_domain(rng, wide), torch::kInt16, thr, p);
    }
  std::printf("jaro_pairs_cpu check: %ld mismatching rows or entries\n", bad);
  return bad != 0;
}
