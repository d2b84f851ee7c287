// mfm_philox.hpp -- the counter-based per-row random stream: Philox4x32-10 keyed by (seed, draw_index, row). Every row owns its
// stream, so a draw is reproducible for a seed and independent of the launch geometry. Included by mfm_tasks.hpp (the latent
// draws of the probit tasks) and by mfm_foldin.hpp (the posterior draws of folded-in entities); restated in tests/philox_ref.py.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mfm {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
    const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += W0;
    k.y += W1;
  }
  return c;
}

struct RowRng {
  uint2 key;
  uint32_t row, d0, d1, n;
  __device__ RowRng(uint64_t seed, uint64_t draw, uint32_t row_)
      : key(make_uint2((uint32_t)seed, (uint32_t)(seed >> 32))), row(row_), d0((uint32_t)draw), d1((uint32_t)(draw >> 32)), n(0) {}
  // two uniforms in (0, 1)
  __device__ __forceinline__ double2 next2() {
    const uint4 r = philox4x32_10(make_uint4(row, n++, d0, d1), key);
    const double a = ((double)(((uint64_t)r.x << 21) | (r.y >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    const double b = ((double)(((uint64_t)r.z << 21) | (r.w >> 11)) + 0.5) * (1.0 / 9007199254740992.0);
    return make_double2(a, b);
  }
};

}  // namespace mfm
