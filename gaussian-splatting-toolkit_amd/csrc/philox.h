// philox.h -- the counter-based generator of the refinement kernels (refine.hip, mcmc.hip): Philox4x32-10
// (Salmon et al., SC'11, the Random123 constants) and the Box-Muller normals built on it.  Mirrored in
// oracle/refine.py (`philox4x32_10`, `split_normals`).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3, uint32_t k0,
                                             uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1,
                 n3 = (uint32_t)p0;
  c0 = n0, c1 = n1, c2 = n2, c3 = n3;
}

// one block: counter (c0, c1, c2, c3) in, four words out; key = (seed low, seed high)
__device__ __forceinline__ void philox4x32_10(const uint64_t seed, uint32_t &c0, uint32_t &c1, uint32_t &c2,
                                              uint32_t &c3) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c0, c1, c2, c3, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// three N(0,1) floats from the block of counter (i, j, 0, 0): Box-Muller on the pairs (x0, x1) -> z0, z1 and
// (x2, x3) -> z2
__device__ __forceinline__ void split_normals(const uint64_t seed, const uint32_t i, const uint32_t j, float z[3]) {
  uint32_t c0 = i, c1 = j, c2 = 0, c3 = 0;
  philox4x32_10(seed, c0, c1, c2, c3);
  const float r0 = sqrtf(-2.f * logf(u01(c0))), r1 = sqrtf(-2.f * logf(u01(c2)));
  const float a0 = 6.283185307179586f * u01(c1), a1 = 6.283185307179586f * u01(c3);
  z[0] = r0 * cosf(a0);
  z[1] = r0 * sinf(a0);
  z[2] = r1 * cosf(a1);
}
