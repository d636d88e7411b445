// fdcn_mc_qmc.hip -- quasi-Monte Carlo paths for the discrete-barrier pricer:
// digitally shifted Sobol points, inverse-CDF normals and a table-driven
// Brownian-bridge path construction, all inside the path kernel.  The path
// functional is fdcn_mc.hip's (fdcn_mc_path.h); the contract of every number
// below is written out in include/fdcn.h (fdcn_mc_qmc_batch).
//
//   qmc_path_kernel<T, ANTI>  one workgroup = one (contract, replicate, chunk
//                             of T * kPerThread observations).  A thread walks
//                             kPerThread observations; for each it generates
//                             the n_steps normals dimension by dimension and
//                             fills W[0 .. n_steps] from the table, then walks
//                             the steps on W's increments.  W lives in LDS as
//                             [n_steps + 1][T]: a lane owns one column, lanes
//                             of a wave read consecutive doubles, and nothing
//                             is a runtime-indexed private array.  The
//                             replicate's digital shift (one Philox block per
//                             dimension, uniform over the workgroup) is put
//                             into LDS once.  sum(p), sum(p^2) per thread in
//                             index order, fixed LDS tree, one partial pair
//                             per workgroup.
//   qmc_finalize_kernel       one thread per contract: the partials of each
//                             replicate in block order, the replicates in
//                             replicate order.
//   qmc_normals_kernel        the generator alone (include/fdcn_diag.h)
//
// T is 256 up to 30 steps and 64 above (fdcn_mc_qmc_plan), so the dynamic LDS
// of a workgroup -- (n_steps + 1) * T doubles and 64 shift words -- is at most
// 62 KB (30 steps) and 33 KB (64 steps).  No floating-point atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "../../include/fdcn_diag.h"
#include "fdcn_mc_path.h"
#include "fdcn_philox.h"
#include "fdcn_qmc_table.h"
#include "fdcn_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPerThread = 16;
constexpr int kWideThreads = 256;   // n_steps <= kWideSteps
constexpr int kWideSteps = 30;
constexpr int kNarrowThreads = 64;  // up to FDCN_QMC_MAX_STEPS
constexpr int kFinalThreads = 256;

using fdcn_mc_path::advance_by;
using fdcn_mc_path::Contract;
using fdcn_mc_path::Path;
using fdcn_mc_path::payoff;

// ---- the generator ----------------------------------------------------------
// Sobol word of Gray code g in one dimension: XOR of the direction numbers of
// g's set bits.  d and n_bits are uniform over a launch (n_bits: the bit length
// of its last observation index), so d[k] is a scalar load.
__device__ __forceinline__ uint32_t sobol_word(const uint32_t* __restrict__ d, uint32_t g,
                                               int n_bits) {
  uint32_t w = 0;
  for (int k = 0; k < n_bits; ++k) w ^= d[k] & (0u - ((g >> k) & 1u));
  return w;
}

// the digital shift of (dimension j, replicate rho): x0 of one Philox block
__device__ __forceinline__ uint32_t shift_word(uint32_t j, uint32_t rho, uint32_t stream,
                                               uint64_t seed) {
  uint32_t x[4];
  fdcn_philox::philox4x32_10(j, rho, 0u, stream, (uint32_t)seed, (uint32_t)(seed >> 32), x);
  return x[0];
}

__device__ __forceinline__ double uniform_of(uint32_t w) { return ((double)w + 0.5) * 0x1p-32; }

// Wichura's AS241 PPND16 with the branches, constants and Horner order of
// CPython's statistics._normal_dist_inv_cdf.  p in (0, 1).
__device__ __forceinline__ double as241(double p) {
  const double q = p - 0.5;
  double r, num, den;
  if (fabs(q) <= 0.425) {
    r = 0.180625 - q * q;
    num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
               6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
             1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
           1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
    den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
               3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
             5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
           4.2313330701600911252e+1) * r + 1.0);
    return num / den;
  }
  r = q <= 0.0 ? p : 1.0 - p;
  r = sqrt(-log(r));
  if (r <= 5.0) {
    r = r - 1.6;
    num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r +
               2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
             3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
           4.63033784615654529590e+0) * r + 1.42343711074968357734e+0);
    den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r +
               1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
             6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
           2.05319162663775882187e+0) * r + 1.0);
  } else {
    r = r - 5.0;
    num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
               1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
             2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
           5.46378491116411436990e+0) * r + 6.65790464350110377720e+0);
    den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r +
               1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
             1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
           5.99832206555888793690e-1) * r + 1.0);
  }
  const double x = num / den;
  return q < 0.0 ? -x : x;
}

// ---- the path kernel --------------------------------------------------------
// bridge_idx, checked on the host (fdcn_qmc_table.h), by value: uniform reads
// from the kernel-argument segment
struct BridgeIdx {
  uint8_t target[FDCN_QMC_MAX_STEPS], left[FDCN_QMC_MAX_STEPS], right[FDCN_QMC_MAX_STEPS];
};

struct QmcArgs {
  int32_t n_steps, n_blocks, R, rep_first, n_bits, scramble;
  int64_t n_obs, obs_first;
  uint64_t seed;
};

// workspace of one contract: R * n_blocks partial pairs, then R replicate means
__host__ __device__ inline size_t ws_doubles(int32_t R, int64_t n_blocks) {
  return (size_t)R * (size_t)n_blocks * 2 + (size_t)R;
}

template <int T, bool ANTI>
__global__ void __launch_bounds__(T)
qmc_path_kernel(QmcArgs a, BridgeIdx bi, const double* __restrict__ params,
                const int32_t* __restrict__ flags, const double* __restrict__ step,
                const uint32_t* __restrict__ dirnum, const double* __restrict__ bridge_w,
                double* __restrict__ ws, double* __restrict__ payoff_out) {
  extern __shared__ double lds[];
  const int n = a.n_steps;
  double* W = lds;                                                // [n + 1][T]
  uint32_t* shift = reinterpret_cast<uint32_t*>(lds + (size_t)(n + 1) * T);  // [n]

  const int blk = blockIdx.x % a.n_blocks;                    // chunk of observations
  const int rep = (blockIdx.x / a.n_blocks) % a.R;            // replicate within the call
  const int b = blockIdx.x / (a.n_blocks * a.R);              // contract
  const int tid = threadIdx.x;
  const double* P = params + (size_t)b * FDCN_MC_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_MC_NFLAG;
  const double* S = step + (size_t)b * n * FDCN_MC_NSTEP;
  const double* BW = bridge_w + (size_t)b * n * 3;
  const Contract c = fdcn_mc_path::load_contract(P, F);
  const uint32_t stream = (uint32_t)F[FDCN_MC_F_STREAM];

  for (int j = tid; j < n; j += T)
    shift[j] = a.scramble ? shift_word((uint32_t)j, (uint32_t)(a.rep_first + rep), stream, a.seed)
                          : 0u;
  W[tid] = 0.0;  // W[0]; no row of the table targets it
  __syncthreads();

  double sum = 0.0, sum2 = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = (int64_t)blk * (T * kPerThread) + (int64_t)k * T + tid;
    if (i >= a.n_obs) break;
    const uint32_t o = (uint32_t)(a.obs_first + i);
    const uint32_t g = o ^ (o >> 1);
    for (int j = 0; j < n; ++j) {
      const uint32_t w = sobol_word(dirnum + (size_t)j * 32, g, a.n_bits) ^ shift[j];
      const double y = as241(uniform_of(w));
      const double* bw = BW + (size_t)j * 3;
      const double mid = bw[0] * W[(int)bi.left[j] * T + tid] + bw[1] * W[(int)bi.right[j] * T + tid];
      W[(int)bi.target[j] * T + tid] = mid + bw[2] * y;
    }
    Path up{c.spot, c.df_T, true}, dn{c.spot, c.df_T, true};
    double prev = 0.0;
    for (int m = 1; m <= n; ++m) {
      const double cur = W[m * T + tid];
      const double dw = cur - prev;
      prev = cur;
      advance_by(up, c, S + (size_t)(m - 1) * FDCN_MC_NSTEP, dw);
      if (ANTI) advance_by(dn, c, S + (size_t)(m - 1) * FDCN_MC_NSTEP, -dw);
    }
    double p = payoff(up, c);
    if (ANTI) p = 0.5 * (p + payoff(dn, c));
    if (payoff_out)
      payoff_out[((size_t)b * (size_t)a.R + (size_t)rep) * (size_t)a.n_obs + (size_t)i] = p;
    sum += p;
    sum2 += p * p;
  }

  // W is done with: its first two rows (n >= 1) hold the tree
  __syncthreads();
  double* sh0 = lds;
  double* sh1 = lds + T;
  sh0[tid] = sum;
  sh1[tid] = sum2;
  __syncthreads();
  for (int off = T / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sh0[tid] += sh0[tid + off];
      sh1[tid] += sh1[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* w = ws + (size_t)b * ws_doubles(a.R, a.n_blocks) +
                ((size_t)rep * (size_t)a.n_blocks + (size_t)blk) * 2;
    w[0] = sh0[0];
    w[1] = sh1[0];
  }
}

// stats[b] = price, stderr, sum m, sum m^2 over the replicate means m
__global__ void __launch_bounds__(kFinalThreads)
qmc_finalize_kernel(int32_t B, int32_t R, int32_t n_blocks, int64_t n_obs,
                    double* __restrict__ ws, double* __restrict__ stats,
                    double* __restrict__ rep_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double* w = ws + (size_t)b * ws_doubles(R, n_blocks);
  double* mean = w + (size_t)R * (size_t)n_blocks * 2;
  const double n = (double)n_obs;
  double sm = 0.0, sm2 = 0.0;
  for (int r = 0; r < R; ++r) {
    const double* wr = w + (size_t)r * (size_t)n_blocks * 2;
    double sum = 0.0, sum2 = 0.0;
    for (int k = 0; k < n_blocks; ++k) {
      sum += wr[2 * k];
      sum2 += wr[2 * k + 1];
    }
    if (rep_out) {
      double* ro = rep_out + ((size_t)b * (size_t)R + (size_t)r) * 2;
      ro[0] = sum;
      ro[1] = sum2;
    }
    const double m = sum / n;
    mean[r] = m;
    sm += m;
    sm2 += m * m;
  }
  const double price = sm / (double)R;
  double ss = 0.0;
  for (int r = 0; r < R; ++r) {
    const double d = mean[r] - price;
    ss += d * d;
  }
  double* o = stats + (size_t)b * FDCN_MC_NSTAT;
  o[0] = price;
  o[1] = R > 1 ? sqrt(ss / (double)(R - 1) / (double)R) : 0.0;
  o[2] = sm;
  o[3] = sm2;
}

// one thread per (replicate, observation): its n_dims words and normals
__global__ void __launch_bounds__(kFinalThreads)
qmc_normals_kernel(int64_t n_obs, int32_t n_dims, int32_t R, int32_t scramble, int32_t n_bits,
                   const uint32_t* __restrict__ dirnum, uint64_t seed, uint32_t stream,
                   int64_t obs_first, int32_t rep_first, uint32_t* __restrict__ words_out,
                   double* __restrict__ y_out) {
  const int64_t t = (int64_t)blockIdx.x * kFinalThreads + threadIdx.x;
  if (t >= n_obs * R) return;
  const int64_t i = t % n_obs;
  const uint32_t rho = (uint32_t)(rep_first + (int32_t)(t / n_obs));
  const uint32_t o = (uint32_t)(obs_first + i);
  const uint32_t g = o ^ (o >> 1);
  for (int j = 0; j < n_dims; ++j) {
    uint32_t w = sobol_word(dirnum + (size_t)j * 32, g, n_bits);
    if (scramble) w ^= shift_word((uint32_t)j, rho, stream, seed);
    if (words_out) words_out[(size_t)t * n_dims + j] = w;
    if (y_out) y_out[(size_t)t * n_dims + j] = as241(uniform_of(w));
  }
}

// ---- host side --------------------------------------------------------------
int qfail(int code, const char* msg) { return fdcn_internal::set_error(code, msg); }

int threads_for(int32_t n_steps) { return n_steps <= kWideSteps ? kWideThreads : kNarrowThreads; }
int64_t chunk_for(int32_t n_steps) { return (int64_t)threads_for(n_steps) * kPerThread; }
int64_t blocks_for(int32_t n_steps, int64_t n_obs) {
  const int64_t c = chunk_for(n_steps);
  return (n_obs + c - 1) / c;
}

// bit length of the last observation index: the Gray-code bits a launch reads
int bits_for(int64_t last) {
  int n = 0;
  while (last >> n) ++n;
  return n;
}

int fail_arg(const char* entry, const char* what) {
  char msg[200];
  snprintf(msg, sizeof msg, "%s: %s", entry, what);
  return qfail(FDCN_EINVAL, msg);
}

// the generator's range, shared by the path entries and fdcn_qmc_normals
int check_points(const char* entry, int64_t n_obs, int32_t R, int32_t scramble, int64_t obs_first,
                 int32_t rep_first) {
  if (n_obs < 1) return fail_arg(entry, "n_obs must be >= 1");
  if (R < 1) return fail_arg(entry, "R must be >= 1");
  if (scramble < 0 || scramble > 1) return fail_arg(entry, "scramble must be 0 or 1");
  if (scramble == 0 && R != 1)
    return fail_arg(entry, "scramble = 0 gives one point set: R must be 1");
  if (obs_first < 0) return fail_arg(entry, "obs_first must be >= 0");
  if (n_obs > ((int64_t)1 << 32) || obs_first > ((int64_t)1 << 32) - n_obs)
    return fail_arg(entry, "obs_first + n_obs must be <= 2^32");
  if (rep_first < 0) return fail_arg(entry, "rep_first must be >= 0");
  if ((int64_t)rep_first + R > 0x7fffffffLL) return fail_arg(entry, "rep_first + R overflows");
  return FDCN_OK;
}

int check_launch(const char* entry, int32_t B, int32_t n_steps, int64_t n_obs, int32_t R,
                 int32_t antithetic, int32_t scramble, const void* params, const void* flags,
                 const void* step, const void* dirnum, const int32_t* bridge_idx,
                 const void* bridge_w, int64_t obs_first, int32_t rep_first, const void* stats) {
  if (B < 1) return fail_arg(entry, "B must be >= 1");
  if (n_steps < 1 || n_steps > FDCN_QMC_MAX_STEPS)
    return fail_arg(entry, "n_steps must be in 1 .. 64 (FDCN_QMC_MAX_STEPS)");
  if (antithetic < 0 || antithetic > 1) return fail_arg(entry, "antithetic must be 0 or 1");
  int rc = check_points(entry, n_obs, R, scramble, obs_first, rep_first);
  if (rc) return rc;
  if ((double)blocks_for(n_steps, n_obs) * (double)R * (double)B > 2147483647.0)
    return fail_arg(entry, "B * R * n_obs is beyond one launch's grid");
  if (!params) return fail_arg(entry, "params is NULL");
  if (!flags) return fail_arg(entry, "flags is NULL");
  if (!step) return fail_arg(entry, "step is NULL");
  if (!dirnum) return fail_arg(entry, "dirnum is NULL");
  if (!bridge_idx) return fail_arg(entry, "bridge_idx is NULL");
  if (!bridge_w) return fail_arg(entry, "bridge_w is NULL");
  if (!stats) return fail_arg(entry, "stats is NULL");
  char why[160];
  if (fdcn_qmc::check_bridge_idx(n_steps, bridge_idx, why, sizeof why)) return fail_arg(entry, why);
  return FDCN_OK;
}

int launch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t R, int32_t antithetic,
           int32_t scramble, const double* params, const int32_t* flags, const double* step,
           const uint32_t* dirnum, const int32_t* bridge_idx, const double* bridge_w,
           uint64_t seed, int64_t obs_first, int32_t rep_first, double* stats, double* rep_out,
           double* payoff_out, double* workspace, hipStream_t stream) {
  QmcArgs a;
  a.n_steps = n_steps;
  a.n_blocks = (int32_t)blocks_for(n_steps, n_obs);
  a.R = R;
  a.rep_first = rep_first;
  a.n_bits = bits_for(obs_first + n_obs - 1);
  a.scramble = scramble;
  a.n_obs = n_obs;
  a.obs_first = obs_first;
  a.seed = seed;
  BridgeIdx bi = {};
  for (int j = 0; j < n_steps; ++j) {  // checked: every entry is in 0 .. n_steps <= 64
    bi.target[j] = (uint8_t)bridge_idx[3 * j];
    bi.left[j] = (uint8_t)bridge_idx[3 * j + 1];
    bi.right[j] = (uint8_t)bridge_idx[3 * j + 2];
  }
  const int T = threads_for(n_steps);
  const size_t lds = (size_t)(n_steps + 1) * T * sizeof(double) +
                     FDCN_QMC_MAX_STEPS * sizeof(uint32_t);
  const dim3 grid((uint32_t)((int64_t)a.n_blocks * R * B)), block(T);
  auto fn = T == kWideThreads
                ? (antithetic ? qmc_path_kernel<kWideThreads, true>
                              : qmc_path_kernel<kWideThreads, false>)
                : (antithetic ? qmc_path_kernel<kNarrowThreads, true>
                              : qmc_path_kernel<kNarrowThreads, false>);
  hipLaunchKernelGGL(fn, grid, block, lds, stream, a, bi, params, flags, step, dirnum, bridge_w,
                     workspace, payoff_out);
  if (hipGetLastError() != hipSuccess) return qfail(FDCN_EHIP, "mc_qmc_batch: launch failed");
  hipLaunchKernelGGL(qmc_finalize_kernel, dim3((B + kFinalThreads - 1) / kFinalThreads),
                     dim3(kFinalThreads), 0, stream, B, R, a.n_blocks, n_obs, workspace, stats,
                     rep_out);
  if (hipGetLastError() != hipSuccess) return qfail(FDCN_EHIP, "mc_qmc_batch: launch failed");
  return FDCN_OK;
}

}  // namespace

extern "C" {

int fdcn_mc_qmc_plan(int32_t n_steps, int64_t n_obs, int32_t R, int32_t* blocks_per_replicate,
                     int32_t* obs_per_block, int64_t* ws_bytes_per_contract) {
  if (n_steps < 1 || n_steps > FDCN_QMC_MAX_STEPS)
    return fail_arg("mc_qmc_plan", "n_steps must be in 1 .. 64 (FDCN_QMC_MAX_STEPS)");
  if (n_obs < 1 || n_obs > ((int64_t)1 << 32))
    return fail_arg("mc_qmc_plan", "n_obs must be in 1 .. 2^32");
  if (R < 1) return fail_arg("mc_qmc_plan", "R must be >= 1");
  const int64_t nb = blocks_for(n_steps, n_obs);
  if (blocks_per_replicate) *blocks_per_replicate = (int32_t)nb;
  if (obs_per_block) *obs_per_block = (int32_t)chunk_for(n_steps);
  if (ws_bytes_per_contract)
    *ws_bytes_per_contract = (int64_t)(ws_doubles(R, nb) * sizeof(double));
  return FDCN_OK;
}

int fdcn_mc_qmc_batch_dev(int32_t B, int32_t n_steps, int64_t n_obs, int32_t R, int32_t antithetic,
                          int32_t scramble, const double* params, const int32_t* flags,
                          const double* step, const uint32_t* dirnum, const int32_t* bridge_idx,
                          const double* bridge_w, uint64_t seed, int64_t obs_first,
                          int32_t rep_first, double* stats, double* rep_out, double* payoff_out,
                          double* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = check_launch("mc_qmc_batch_dev", B, n_steps, n_obs, R, antithetic, scramble,
                              params, flags, step, dirnum, bridge_idx, bridge_w, obs_first,
                              rep_first, stats);
  if (rc) return rc;
  const int64_t need =
      (int64_t)(ws_doubles(R, blocks_for(n_steps, n_obs)) * sizeof(double)) * B;
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_qmc_batch_dev", "this launch needs (fdcn_mc_qmc_plan)", workspace, workspace_bytes, need,
      (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, n_obs, R, antithetic, scramble, params, flags, step, dirnum,
                      bridge_idx, bridge_w, seed, obs_first, rep_first, stats, rep_out, payoff_out,
                      (double*)ws, (hipStream_t)stream);
      });
}

int fdcn_mc_qmc_batch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t R, int32_t antithetic,
                      int32_t scramble, const double* params, const int32_t* flags,
                      const double* step, const uint32_t* dirnum, const int32_t* bridge_idx,
                      const double* bridge_w, uint64_t seed, int64_t obs_first, int32_t rep_first,
                      double* stats, double* rep_out, double* payoff_out) {
  int rc = check_launch("mc_qmc_batch", B, n_steps, n_obs, R, antithetic, scramble, params, flags,
                        step, dirnum, bridge_idx, bridge_w, obs_first, rep_first, stats);
  if (rc) return rc;
  rc = fdcn_internal::mc_check_contracts("mc_qmc_batch", B, params, flags);
  if (rc) return rc;
  char why[160];
  if (fdcn_qmc::check_bridge_w(B, n_steps, bridge_w, why, sizeof why))
    return fail_arg("mc_qmc_batch", why);
  fdcn_internal::HostCall c("mc_qmc_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B, ns = (size_t)n_steps, nr = (size_t)R;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_MC_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_MC_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * ns * FDCN_MC_NSTEP);
  const int rD = c.in(dirnum, sizeof(uint32_t) * ns * 32);
  const int rW = c.in(bridge_w, sizeof(double) * nb * ns * 3);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_MC_NSTAT);
  const int rR = c.out(rep_out, sizeof(double) * nb * nr * 2);
  const int rY = c.out(payoff_out, sizeof(double) * nb * nr * (size_t)n_obs);
  const int rX = c.scratch(sizeof(double) * ws_doubles(R, blocks_for(n_steps, n_obs)) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, n_obs, R, antithetic, scramble, c.dev<double>(rP),
                  c.dev<int32_t>(rF), c.dev<double>(rS), c.dev<uint32_t>(rD), bridge_idx,
                  c.dev<double>(rW), seed, obs_first, rep_first, c.dev<double>(rO),
                  c.dev<double>(rR), c.dev<double>(rY), c.dev<double>(rX), stream);
  });
}

int fdcn_qmc_normals(int64_t n_obs, int32_t n_dims, int32_t R, int32_t scramble,
                     const uint32_t* dirnum, uint64_t seed, int32_t stream_id, int64_t obs_first,
                     int32_t rep_first, uint32_t* words_out, double* y_out) {
  if (n_dims < 1 || n_dims > FDCN_QMC_MAX_STEPS)
    return fail_arg("qmc_normals", "n_dims must be in 1 .. 64 (FDCN_QMC_MAX_STEPS)");
  int rc = check_points("qmc_normals", n_obs, R, scramble, obs_first, rep_first);
  if (rc) return rc;
  if (stream_id < 0) return fail_arg("qmc_normals", "stream id must be >= 0");
  if (!dirnum) return fail_arg("qmc_normals", "dirnum is NULL");
  if (!words_out && !y_out) return fail_arg("qmc_normals", "words_out and y_out are both NULL");
  const double threads = (double)n_obs * (double)R;
  if (threads > 2147483647.0 * kFinalThreads)
    return fail_arg("qmc_normals", "n_obs * R is beyond one launch's grid");
  const int64_t grid = (n_obs * R + kFinalThreads - 1) / kFinalThreads;
  fdcn_internal::HostCall c("qmc_normals");
  if ((rc = c.open())) return rc;
  const size_t count = (size_t)n_obs * (size_t)R * (size_t)n_dims;
  const int rD = c.in(dirnum, sizeof(uint32_t) * (size_t)n_dims * 32);
  const int rU = c.out(words_out, sizeof(uint32_t) * count);
  const int rY = c.out(y_out, sizeof(double) * count);
  const int n_bits = bits_for(obs_first + n_obs - 1);
  return c.run([&](hipStream_t stream) {
    hipLaunchKernelGGL(qmc_normals_kernel, dim3((uint32_t)grid), dim3(kFinalThreads), 0, stream,
                       n_obs, n_dims, R, scramble, n_bits, c.dev<uint32_t>(rD), seed,
                       (uint32_t)stream_id, obs_first, rep_first, c.dev<uint32_t>(rU),
                       c.dev<double>(rY));
    return hipGetLastError() == hipSuccess ? FDCN_OK
                                           : qfail(FDCN_EHIP, "qmc_normals: launch failed");
  });
}

}  // extern "C"
