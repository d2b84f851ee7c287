// A stand-alone program around csrc/mfm_foldin_gibbs_plan.hpp, the host code of mfm_foldin_gibbs_* that needs no device: built with
// -fsanitize=address,undefined by tests/test_fold_in_gibbs_cpu.py. Exit status 0 and "plan: ok", "check: ok" on success.
#include "mfm_foldin_gibbs_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

using namespace mfm;

#define REQUIRE(c)                                                  \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #c); \
      return 1;                                                     \
    }                                                               \
  } while (0)

static int plan_cases() {
  std::mt19937_64 rng(7);
  const int row_choices[] = {0, 1, 2, 63, 64, 65, 257};
  for (int rep = 0; rep < 400; rep++) {
    const int64_t U = 1 + (int64_t)(rng() % 40);
    const int S = 1 + (int)(rng() % 9), K = (int)(rng() % 66), lin = (int)(rng() % 2), M = K + lin;
    if (M == 0) continue;
    std::vector<int64_t> eoff(U + 1, 0);
    for (int64_t u = 0; u < U; u++) eoff[u + 1] = eoff[u] + row_choices[rng() % 7];
    const int64_t one = (257 * (int64_t)(M + 1) + K + 1) * 8;
    const int64_t bounds[] = {1, 8, one / 3, one, 3 * one + 5, S * one, 20 * S * one, (int64_t)256 << 20};
    for (int64_t bound : bounds) {
      const std::vector<FoldinChunk> chunks = foldin_gibbs_plan(eoff.data(), U, S, M, K, bound);
      std::vector<int> seen((size_t)U * S, 0);
      int64_t next_u = 0;
      for (const FoldinChunk &c : chunks) {
        REQUIRE(c.nu >= 1 && c.ns >= 1 && c.u0 >= 0 && c.u0 + c.nu <= U && c.s0 >= 0 && c.s0 + c.ns <= S);
        REQUIRE(c.u0 == next_u || (c.u0 + 1 == next_u && c.nu == 1 && c.s0 > 0));  // entities in order, samples inside one entity
        next_u = c.u0 + c.nu;
        for (int64_t u = c.u0; u < c.u0 + c.nu; u++)
          for (int s = c.s0; s < c.s0 + c.ns; s++) seen[(size_t)u * S + s]++;
        if (c.nu * (int64_t)c.ns > 1) REQUIRE(foldin_gibbs_chunk_doubles(eoff.data(), c, M, K) * 8 <= bound);
        if (c.nu > 1) REQUIRE(c.s0 == 0 && c.ns == S);
      }
      for (int v : seen) REQUIRE(v == 1);
      if (bound == ((int64_t)256 << 20)) REQUIRE(chunks.size() == 1);
    }
  }
  std::printf("plan: ok\n");
  return 0;
}

static int check_cases() {
  const int S = 2, K = 2, C = 4;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> mu(S * (K + 1), 0.25), lam(S * (K + 1), 1.5), cut = {-1.0, 0.0, 1.0, -0.5, -0.5, 2.0}, y = {0, 3, 1, 2, 0};
  auto run = [&](int lin, int task, int64_t nb, int64_t ni) {
    return foldin_gibbs_check(S, K, lin, task, C, cut.data(), mu.data(), lam.data(), nb, ni, y.data(), (int64_t)y.size());
  };
  REQUIRE(run(1, 0, 10, 40).empty() && run(1, 1, 0, 1).empty() && run(0, 1, 65534, 1).empty());
  REQUIRE(!run(1, 2, 10, 40).empty() && !run(1, -1, 10, 40).empty());
  REQUIRE(!run(1, 0, 10, 0).empty() && !run(1, 0, -1, 5).empty() && !run(1, 0, 65535, 1).empty() && !run(1, 0, 0, 65536).empty());
  REQUIRE(!run(1, 0, 2147483647, 2147483647).empty());
  for (double bad : {0.0, -1.0, inf, nan}) {
    lam[3] = bad;  // sample 1, component 0: read only with the linear term
    REQUIRE(!run(1, 0, 1, 1).empty() && run(0, 0, 1, 1).empty());
    lam[3] = 1.5;
    lam[5] = bad;
    REQUIRE(!run(0, 1, 1, 1).empty());
    lam[5] = 1.5;
  }
  for (double bad : {inf, -inf, nan}) {
    mu[1] = bad;
    REQUIRE(!run(1, 0, 1, 1).empty());
    mu[1] = 0.25;
    cut[4] = bad;
    REQUIRE(!run(1, 1, 1, 1).empty() && run(1, 0, 1, 1).empty());  // (the classifier reads no cutpoints)
    cut[4] = -0.5;
  }
  cut[2] = -0.5;  // decreasing
  REQUIRE(!run(1, 1, 1, 1).empty());
  cut[2] = 1.0;
  for (double bad : {4.0, -1.0, 1.5, nan, inf}) {
    y[2] = bad;
    REQUIRE(!run(1, 1, 1, 1).empty());
    y[2] = 1.0;
  }
  REQUIRE(foldin_gibbs_check(S, K, 1, 1, 1, cut.data(), mu.data(), lam.data(), 1, 1, y.data(), 0) != "");  // one class
  REQUIRE(foldin_gibbs_check(S, K, 1, 1, C, nullptr, mu.data(), lam.data(), 1, 1, y.data(), 5) != "");
  REQUIRE(foldin_gibbs_check(S, K, 1, 0, 0, nullptr, nullptr, lam.data(), 1, 1, y.data(), 5) != "");
  REQUIRE(foldin_gibbs_check(0, K, 1, 1, C, cut.data(), mu.data(), lam.data(), 1, 1, nullptr, 0).empty());
  std::printf("check: ok\n");
  return 0;
}

int main() { return plan_cases() || check_cases(); }
