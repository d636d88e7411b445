// fdcn_mc.hip -- Monte Carlo discrete-barrier pricer for gfx950.
//
// The cross-check of the FD barrier engines: price_discrete_barrier_mc of
// mc_discrete_barrier_option.py (:225-424).  One launch prices B contracts
// that share n_steps, n_obs and the antithetic switch; everything else is per
// contract.  A path's whole state is one double, so nothing touches memory
// except the per-step table (uniform across a workgroup: scalar loads), the
// optional supplied normals and the optional payoff dump.  fp64 throughout.
//
//   mc_path_kernel<ANTI, GEN>  one workgroup = kChunk consecutive
//                              observations of one contract; each thread
//                              walks kPerThread of them and keeps sum(p),
//                              sum(p^2) in index order; fixed LDS tree; one
//                              partial pair per workgroup into the workspace
//   mc_finalize_kernel         one thread per contract adds the partials in
//                              block order and writes price / stderr (:407-410)
//   mc_normals_kernel          the generator alone (include/fdcn_diag.h)
//
// No floating-point atomics: the chunk is a function of n_obs only and the
// tree is fixed, so a contract's result depends on neither B, its position in
// the batch, nor how the workgroups were scheduled.
//
// The path functional keeps the reference's operation order (simulate_payoffs,
// :314-387) with separately rounded multiply and add (contraction off), so on
// supplied normals it differs from NumPy only through the device exp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "../../include/fdcn_diag.h"
#include "fdcn_mc_path.h"
#include "fdcn_philox.h"
#include "fdcn_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // observations per workgroup

using fdcn_philox::normal_pair;  // Philox4x32-10 + Box-Muller (fdcn_philox.h)

// ---- one path: Contract / Path / advance / payoff of fdcn_mc_path.h ----------
using fdcn_mc_path::advance;
using fdcn_mc_path::Contract;
using fdcn_mc_path::Path;
using fdcn_mc_path::payoff;

struct McArgs {
  int32_t n_steps, n_blocks;
  int64_t n_obs, obs_first;
  uint64_t seed;
};

// The arrays are separate __restrict__ arguments: with the inputs known not to
// alias the payoff dump, the per-step table (uniform across a workgroup) is
// read with scalar loads.
template <bool ANTI, bool GEN>
__global__ void __launch_bounds__(kThreads)
mc_path_kernel(McArgs a, const double* __restrict__ params, const int32_t* __restrict__ flags,
               const double* __restrict__ step, const double* __restrict__ z,
               double* __restrict__ ws, double* __restrict__ payoff_out) {
  const int b = blockIdx.x / a.n_blocks;    // contract
  const int blk = blockIdx.x % a.n_blocks;  // chunk of observations
  const int tid = threadIdx.x;
  const double* P = params + (size_t)b * FDCN_MC_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_MC_NFLAG;
  const double* S = step + (size_t)b * a.n_steps * FDCN_MC_NSTEP;
  const Contract c = fdcn_mc_path::load_contract(P, F);
  const uint32_t stream = (uint32_t)F[FDCN_MC_F_STREAM];

  double sum = 0.0, sum2 = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = (int64_t)blk * kChunk + (int64_t)k * kThreads + tid;
    if (i >= a.n_obs) break;
    Path up{c.spot, c.df_T, true}, dn{c.spot, c.df_T, true};
    const double* zi = GEN ? nullptr : z + (size_t)i * a.n_steps;
    for (int m = 0; m < a.n_steps; m += 2) {
      double z0, z1 = 0.0;
      if (GEN) {
        normal_pair((uint64_t)(a.obs_first + i), (uint32_t)(m >> 1), stream, a.seed, z0, z1);
      } else {
        z0 = zi[m];
        if (m + 1 < a.n_steps) z1 = zi[m + 1];
      }
      advance(up, c, S + (size_t)m * FDCN_MC_NSTEP, z0);
      if (ANTI) advance(dn, c, S + (size_t)m * FDCN_MC_NSTEP, -z0);
      if (m + 1 < a.n_steps) {
        advance(up, c, S + (size_t)(m + 1) * FDCN_MC_NSTEP, z1);
        if (ANTI) advance(dn, c, S + (size_t)(m + 1) * FDCN_MC_NSTEP, -z1);
      }
    }
    double p = payoff(up, c);
    if (ANTI) p = 0.5 * (p + payoff(dn, c));
    if (payoff_out) payoff_out[(size_t)b * (size_t)a.n_obs + (size_t)i] = p;
    sum += p;
    sum2 += p * p;
  }

  __shared__ double sh[2][kThreads];
  sh[0][tid] = sum;
  sh[1][tid] = sum2;
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sh[0][tid] += sh[0][tid + off];
      sh[1][tid] += sh[1][tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* w = ws + ((size_t)b * a.n_blocks + blk) * 2;
    w[0] = sh[0][0];
    w[1] = sh[1][0];
  }
}

// stats[b] = price, stderr, sum p, sum p^2 (:407-410)
__global__ void __launch_bounds__(kThreads) mc_finalize_kernel(int32_t B, int32_t n_blocks,
                                                               int64_t n_obs,
                                                               const double* __restrict__ ws,
                                                               double* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* w = ws + (size_t)b * n_blocks * 2;
  double sum = 0.0, sum2 = 0.0;
  for (int k = 0; k < n_blocks; ++k) {
    sum += w[2 * k];
    sum2 += w[2 * k + 1];
  }
  const double n = (double)n_obs;
  const double price = sum / n;
  const double var = fmax(0.0, sum2 / n - price * price);
  double* o = stats + (size_t)b * FDCN_MC_NSTAT;
  o[0] = price;
  o[1] = sqrt(var / n);
  o[2] = sum;
  o[3] = sum2;
}

__global__ void __launch_bounds__(kThreads) mc_normals_kernel(int64_t n_obs, int32_t n_steps,
                                                              uint64_t seed, uint32_t stream,
                                                              int64_t obs_first,
                                                              double* __restrict__ z) {
  const int64_t n_pairs = (n_steps + 1) / 2;
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= n_obs * n_pairs) return;
  const int64_t i = t / n_pairs;
  const int64_t j = t % n_pairs;
  double z0, z1;
  normal_pair((uint64_t)(obs_first + i), (uint32_t)j, stream, seed, z0, z1);
  double* zi = z + (size_t)i * n_steps;
  zi[2 * j] = z0;
  if (2 * j + 1 < n_steps) zi[2 * j + 1] = z1;  // an odd n_steps drops the last sine
}

// ---- host side -------------------------------------------------------------
int mfail(int code, const char* msg) { return fdcn_internal::set_error(code, msg); }

int64_t blocks_for(int64_t n_obs) { return (n_obs + kChunk - 1) / kChunk; }

// sizes every entry point checks, before any device call
int check_sizes(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic) {
  if (B < 1) return mfail(FDCN_EINVAL, "mc_barrier_batch: B must be >= 1");
  if (n_steps < 1) return mfail(FDCN_EINVAL, "mc_barrier_batch: n_steps must be >= 1");
  if (n_obs < 1) return mfail(FDCN_EINVAL, "mc_barrier_batch: n_obs must be >= 1");
  if (antithetic < 0 || antithetic > 1)
    return mfail(FDCN_EINVAL, "mc_barrier_batch: antithetic must be 0 or 1");
  if (n_obs > ((int64_t)1 << 40) || blocks_for(n_obs) * (int64_t)B > 0x7fffffffLL)
    return mfail(FDCN_EINVAL, "mc_barrier_batch: B * n_obs is beyond one launch's grid");
  return FDCN_OK;
}

int launch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic, const double* params,
           const int32_t* flags, const double* step, const double* z, uint64_t seed,
           int64_t obs_first, double* stats, double* payoff_out, double* workspace,
           hipStream_t stream) {
  McArgs a;
  a.n_steps = n_steps;
  a.n_blocks = (int32_t)blocks_for(n_obs);
  a.n_obs = n_obs;
  a.obs_first = obs_first;
  a.seed = seed;
  const dim3 grid((uint32_t)((int64_t)a.n_blocks * B)), block(kThreads);
  auto fn = antithetic ? (z ? mc_path_kernel<true, false> : mc_path_kernel<true, true>)
                       : (z ? mc_path_kernel<false, false> : mc_path_kernel<false, true>);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, a, params, flags, step, z, workspace,
                     payoff_out);
  if (hipGetLastError() != hipSuccess) return mfail(FDCN_EHIP, "mc_barrier_batch: launch failed");
  hipLaunchKernelGGL(mc_finalize_kernel, dim3((B + kThreads - 1) / kThreads), block, 0, stream, B,
                     a.n_blocks, n_obs, workspace, stats);
  if (hipGetLastError() != hipSuccess) return mfail(FDCN_EHIP, "mc_barrier_batch: launch failed");
  return FDCN_OK;
}

}  // namespace

// the per-contract checks of the host entries (also fdcn_mc_qmc_batch)
int fdcn_internal::mc_check_contracts(const char* entry, int32_t B, const double* params,
                                       const int32_t* flags) {
  char msg[160];
  for (int32_t b = 0; b < B; ++b) {
    const int32_t* f = flags + (size_t)b * FDCN_MC_NFLAG;
    const double* p = params + (size_t)b * FDCN_MC_NPARAM;
    const char* bad = nullptr;
    if (f[FDCN_MC_F_PUT] < 0 || f[FDCN_MC_F_PUT] > 1) bad = "flag put must be 0 or 1";
    else if (f[FDCN_MC_F_KIND] < 0 || f[FDCN_MC_F_KIND] > 4) bad = "flag kind must be 0..4";
    else if (f[FDCN_MC_F_REBATE_AT_HIT] < 0 || f[FDCN_MC_F_REBATE_AT_HIT] > 1)
      bad = "flag rebate_at_hit must be 0 or 1";
    else if (f[FDCN_MC_F_DIV_FIRST] < 0 || f[FDCN_MC_F_DIV_FIRST] > 1)
      bad = "flag dividend_before_monitor must be 0 or 1";
    else if (f[FDCN_MC_F_STREAM] < 0) bad = "flag stream id must be >= 0";
    else if (!(p[FDCN_MC_P_SPOT] > 0.0)) bad = "spot must be positive";
    else if (!(p[FDCN_MC_P_STRIKE] > 0.0)) bad = "strike must be positive";
    else if (f[FDCN_MC_F_KIND] != 0 && !(p[FDCN_MC_P_THRESHOLD] > 0.0))
      bad = "threshold must be positive where a barrier is set";
    if (bad) {
      snprintf(msg, sizeof msg, "%s: contract %d: %s", entry, b, bad);
      return set_error(FDCN_EINVAL, msg);
    }
  }
  return FDCN_OK;
}

extern "C" {

int fdcn_mc_plan(int64_t n_obs, int32_t* blocks_per_contract, int32_t* obs_per_block,
                 int64_t* ws_bytes_per_contract) {
  if (n_obs < 1 || n_obs > ((int64_t)1 << 40))
    return mfail(FDCN_EINVAL, "mc_plan: n_obs must be in 1 .. 2^40");
  const int64_t nb = blocks_for(n_obs);
  if (blocks_per_contract) *blocks_per_contract = (int32_t)nb;
  if (obs_per_block) *obs_per_block = kChunk;
  if (ws_bytes_per_contract) *ws_bytes_per_contract = nb * 2 * (int64_t)sizeof(double);
  return FDCN_OK;
}

int fdcn_mc_barrier_batch_dev(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                              const double* params, const int32_t* flags, const double* step,
                              const double* z, uint64_t seed, int64_t obs_first, double* stats,
                              double* payoff_out, double* workspace, int64_t workspace_bytes,
                              void* stream) {
  int rc = check_sizes(B, n_steps, n_obs, antithetic);
  if (rc) return rc;
  if (!params) return mfail(FDCN_EINVAL, "mc_barrier_batch_dev: params is NULL");
  if (!flags) return mfail(FDCN_EINVAL, "mc_barrier_batch_dev: flags is NULL");
  if (!step) return mfail(FDCN_EINVAL, "mc_barrier_batch_dev: step is NULL");
  if (!stats) return mfail(FDCN_EINVAL, "mc_barrier_batch_dev: stats is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_barrier_batch_dev", "this launch needs (fdcn_mc_plan)", workspace, workspace_bytes,
      blocks_for(n_obs) * 2 * (int64_t)sizeof(double) * B, (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, n_obs, antithetic, params, flags, step, z, seed, obs_first,
                      stats, payoff_out, (double*)ws, (hipStream_t)stream);
      });
}

int fdcn_mc_barrier_batch(int32_t B, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          const double* z, uint64_t seed, int64_t obs_first, double* stats,
                          double* payoff_out) {
  int rc = check_sizes(B, n_steps, n_obs, antithetic);
  if (rc) return rc;
  if (!params) return mfail(FDCN_EINVAL, "mc_barrier_batch: params is NULL");
  if (!flags) return mfail(FDCN_EINVAL, "mc_barrier_batch: flags is NULL");
  if (!step) return mfail(FDCN_EINVAL, "mc_barrier_batch: step is NULL");
  if (!stats) return mfail(FDCN_EINVAL, "mc_barrier_batch: stats is NULL");
  rc = fdcn_internal::mc_check_contracts("mc_barrier_batch", B, params, flags);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_barrier_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_MC_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_MC_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_MC_NSTEP);
  const int rZ = c.in(z, sizeof(double) * (size_t)n_obs * (size_t)n_steps);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_MC_NSTAT);
  const int rY = c.out(payoff_out, sizeof(double) * nb * (size_t)n_obs);
  const int rW = c.scratch(sizeof(double) * 2 * (size_t)blocks_for(n_obs) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, n_obs, antithetic, c.dev<double>(rP), c.dev<int32_t>(rF),
                  c.dev<double>(rS), c.dev<double>(rZ), seed, obs_first, c.dev<double>(rO),
                  c.dev<double>(rY), c.dev<double>(rW), stream);
  });
}

int fdcn_mc_normals(int64_t n_obs, int32_t n_steps, uint64_t seed, int32_t stream_id,
                    int64_t obs_first, double* z) {
  if (n_obs < 1) return mfail(FDCN_EINVAL, "mc_normals: n_obs must be >= 1");
  if (n_steps < 1) return mfail(FDCN_EINVAL, "mc_normals: n_steps must be >= 1");
  if (stream_id < 0) return mfail(FDCN_EINVAL, "mc_normals: stream id must be >= 0");
  if (!z) return mfail(FDCN_EINVAL, "mc_normals: z is NULL");
  const int64_t threads = n_obs * (((int64_t)n_steps + 1) / 2);
  const int64_t grid = (threads + kThreads - 1) / kThreads;
  if (n_obs > ((int64_t)1 << 40) || grid > 0x7fffffffLL)
    return mfail(FDCN_EINVAL, "mc_normals: n_obs * n_steps is beyond one launch's grid");
  fdcn_internal::HostCall c("mc_normals");
  const int rc = c.open();
  if (rc) return rc;
  const int rZ = c.out(z, sizeof(double) * (size_t)n_obs * (size_t)n_steps);
  return c.run([&](hipStream_t stream) {
    hipLaunchKernelGGL(mc_normals_kernel, dim3((uint32_t)grid), dim3(kThreads), 0, stream, n_obs,
                       n_steps, seed, (uint32_t)stream_id, obs_first, c.dev<double>(rZ));
    return hipGetLastError() == hipSuccess ? FDCN_OK
                                           : mfail(FDCN_EHIP, "mc_normals: launch failed");
  });
}

}  // extern "C"
