// mfm_foldin_gibbs_plan.hpp -- the host side of mfm_foldin_gibbs_* that needs no device (mfm_foldin_gibbs.hip): the
// refusals made before any launch and the walk over (entity, sample) cells in chunks whose scratch stays under the handle's bound.
// Plain C++ with no HIP header, so that a stand-alone program can run it under a host sanitizer.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace mfm {

constexpr int FOLDIN_GIBBS_MAX_SWEEPS = 65535;  // the sweep number shares the draw word with a 16-bit-shifted tag (mfm_foldin_gibbs.hpp)
constexpr int FOLDIN_TASK_CLASSIFIER = 0, FOLDIN_TASK_ORDERED = 1;

// "" when the call may run, else the message of MFM_ERR_INVALID. mu / lam: [S][K + 1], component 0 read only with `lin`;
// cut: [S][n_class - 1] (ordered probit); y: the handle's n labels.
inline std::string foldin_gibbs_check(int S, int K, int lin, int task, int n_class, const double *cut, const double *mu,
                                      const double *lam, int64_t n_burn, int64_t n_inner, const double *y, int64_t n) {
  if (task != FOLDIN_TASK_CLASSIFIER && task != FOLDIN_TASK_ORDERED) return "fold-in: task must be 0 (classifier) or 1 (ordered probit)";
  if (n_inner < 1) return "fold-in: n_inner must be at least 1";
  if (n_burn < 0) return "fold-in: n_burn must not be negative";
  if (n_burn + n_inner > FOLDIN_GIBBS_MAX_SWEEPS)
    return "fold-in: n_burn + n_inner must not exceed " + std::to_string(FOLDIN_GIBBS_MAX_SWEEPS);
  if (!mu || !lam) return "no hyper-parameter arrays";
  for (int s = 0; s < S; s++)
    for (int j = 1 - lin; j < K + 1; j++) {
      const double l = lam[(size_t)s * (K + 1) + j], m = mu[(size_t)s * (K + 1) + j];
      if (!(l > 0.0) || !std::isfinite(l) || !std::isfinite(m))
        return "fold-in: sample " + std::to_string(s) + " has a prior precision that is not positive and finite, or a prior mean "
               "that is not finite (component " + std::to_string(j) + ")";
    }
  if (task == FOLDIN_TASK_ORDERED) {
    if (n_class < 2) return "fold-in: ordered probit needs at least 2 classes";
    if (!cut) return "fold-in: ordered probit needs the cutpoints of every sample";
    for (int s = 0; s < S; s++)
      for (int c = 0; c < n_class - 1; c++) {
        const double g = cut[(size_t)s * (n_class - 1) + c];
        if (!std::isfinite(g)) return "fold-in: sample " + std::to_string(s) + " has a cutpoint that is not finite";
        if (c > 0 && g < cut[(size_t)s * (n_class - 1) + c - 1])
          return "fold-in: the cutpoints of sample " + std::to_string(s) + " are not non-decreasing";
      }
    for (int64_t i = 0; i < n; i++)
      if (!(y[i] >= 0.0) || !(y[i] < (double)n_class) || y[i] != std::floor(y[i]))
        return "fold-in: y holds a label that is not an integer in [0, " + std::to_string(n_class) + ")";
  }
  return "";
}

struct FoldinChunk {
  int64_t u0, nu;  // entities [u0, u0 + nu)
  int s0, ns;      // samples [s0, s0 + ns)
};

// doubles of scratch of one chunk: per sample the rows' z and f, (M + 1) per row, and the results, (K + 1) per entity
inline int64_t foldin_gibbs_chunk_doubles(const int64_t *eoff, const FoldinChunk &c, int M, int K) {
  return (int64_t)c.ns * ((eoff[c.u0 + c.nu] - eoff[c.u0]) * (int64_t)(M + 1) + c.nu * (int64_t)(K + 1));
}

// The chunks of a call, in launch order. Entities are taken whole sample ranges at a time, as many as the prefix sums of eoff
// (U + 1 entries) keep under `bound` bytes; an entity whose S cells alone exceed the bound is walked in ranges of samples, and a
// single cell larger than the bound runs alone. Every (entity, sample) is in exactly one chunk.
inline std::vector<FoldinChunk> foldin_gibbs_plan(const int64_t *eoff, int64_t U, int S, int M, int K, int64_t bound) {
  std::vector<FoldinChunk> out;
  const int64_t cap = std::max<int64_t>(bound / (int64_t)sizeof(double), 1);  // doubles
  const int64_t max_grid = 2147483647;
  auto cell = [&](int64_t u) { return (eoff[u + 1] - eoff[u]) * (int64_t)(M + 1) + (int64_t)(K + 1); };
  int64_t u0 = 0;
  while (u0 < U) {
    int64_t nu = 0, sum = 0;  // doubles of one sample's slab of entities [u0, u0 + nu)
    while (u0 + nu < U && nu < max_grid && (sum + cell(u0 + nu)) <= cap / S) {
      sum += cell(u0 + nu);
      nu++;
    }
    if (nu > 0) {
      out.push_back(FoldinChunk{u0, nu, 0, S});
      u0 += nu;
      continue;
    }
    const int64_t per = cell(u0);  // one entity: ranges of samples
    const int Sc = (int)std::min<int64_t>(S, std::max<int64_t>(cap / per, 1));
    for (int s0 = 0; s0 < S; s0 += Sc) out.push_back(FoldinChunk{u0, 1, s0, std::min(Sc, S - s0)});
    u0++;
  }
  return out;
}

}  // namespace mfm
