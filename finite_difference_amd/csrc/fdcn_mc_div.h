// fdcn_mc_div.h -- the cash-dividend map of the Monte Carlo path kernels on the
// log-spot, and its inverse (include/fdcn.h, fdcn_mc_lsm_div_batch): one
// definition for the least-squares kernel (fdcn_mc_lsm.hip, forward and
// backward) and for the forward-only walks of the dual and the table-policy
// kernels (fdcn_mc_dual.hip, fdcn_mc_policy.h).
//
//   g(s) = s - D  (s >= 2 D),  s / 2  (below)
//
// g is continuous at 2 D, so a rounding that takes the other branch on the way
// back moves x by rounding error only.  Include after a
// `#pragma clang fp contract(off)`: every operation is rounded separately.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>

namespace fdcn_div {

constexpr double kLn2 = 0.6931471805599453094;

__device__ __forceinline__ double div_forward(double x, double d) {
  const double s = exp(x);
  return s >= 2.0 * d ? log(s - d) : x - kLn2;
}

__device__ __forceinline__ double div_backward(double x, double d) {
  const double s = exp(x);
  return s >= d ? log(s + d) : x + kLn2;
}

// D_m of a dividend row.  The row is uniform across the workgroup and nothing
// writes it during a launch; reading it through the constant address space
// makes the load a scalar one whatever the compiler can prove about the stores
// around it (inside the dual kernels' nested loops it proves too little, and a
// plain read becomes a vector load with a vector compare behind it).
__device__ __forceinline__ double div_at(const double* row, int i) {
  return ((const __attribute__((address_space(4))) double*)row)[i];
}

}  // namespace fdcn_div
