// distr_philox.hpp -- Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants), one
// round function for the host and the device. The dropout mask of the layer-wise train path is a pure function of it (DESIGN.md
// section 8g): no generator state anywhere, the same bits in the kernels' epilogues and in distr_train_dropout_keep.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DISTR_HD __host__ __device__
#else
#define DISTR_HD
#endif

namespace distr {

struct Philox4 { uint32_t v[4]; };

DISTR_HD inline uint32_t philox_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

DISTR_HD inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = philox_mulhi(M0, c0), l0 = M0 * c0;
    const uint32_t h1 = philox_mulhi(M1, c2), l1 = M1 * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1;
    c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += W0; k1 += W1;
  }
  Philox4 o;
  o.v[0] = c0; o.v[1] = c1; o.v[2] = c2; o.v[3] = c3;
  return o;
}

// The four draws of the dropout mask for points 4q .. 4q + 3 of global segment g, output unit n of lin_layer: the counter layout of
// include/distr_train.h. keep = draw >= threshold.
DISTR_HD inline Philox4 dropout_draws(uint32_t key0, uint32_t key1, uint32_t layer, uint32_t g, uint32_t q, uint32_t n) {
  return philox4x32_10(q, g, n, layer, key0, key1);
}

}  // namespace distr
