// fdcn_philox.h -- the normal generator of the Monte Carlo path kernels
// (fdcn_mc.hip, fdcn_mc_bgk.hip).  The counter / key mapping is a contract of
// include/fdcn.h; both kernels draw the same z for the same (seed, stream id,
// observation, pair).
#ifndef FDCN_PHILOX_H
#define FDCN_PHILOX_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

// u53 is evaluated with separately rounded multiply and add (fdcn.h)
#pragma clang fp contract(off)

namespace fdcn_philox {

// ---- Philox4x32-10 (Salmon et al., SC'11; Random123 constants) ------------
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0;
  x[1] = c1;
  x[2] = c2;
  x[3] = c3;
}

// 53 bits of two words -> (0, 1]: ((hi >> 5) 2^26 + (lo >> 6) + 0.5) 2^-53
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * 0x1p-53;
}

// The normals z[2j], z[2j+1] of observation `obs` (the mapping of fdcn.h).
__device__ __forceinline__ void normal_pair(uint64_t obs, uint32_t j, uint32_t stream,
                                            uint64_t seed, double& z0, double& z1) {
  uint32_t x[4];
  philox4x32_10((uint32_t)obs, (uint32_t)(obs >> 32), j, stream, (uint32_t)seed,
                (uint32_t)(seed >> 32), x);
  const double u1 = u53(x[0], x[1]);
  const double u2 = u53(x[2], x[3]);
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  z0 = r * cs;
  z1 = r * sn;
}

}  // namespace fdcn_philox

#endif  // FDCN_PHILOX_H
