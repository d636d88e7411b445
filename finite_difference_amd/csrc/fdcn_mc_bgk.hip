// fdcn_mc_bgk.hip -- Monte Carlo paths of the BGK barrier pricer for gfx950.
//
// The path functional of DiscreteBarrierBGKPricer._mc_out_price
// (discrete_barrier_bgk.py:770-878): log-spot as a running sum, a spot only
// on monitored steps and at maturity, an upper and a lower level, a breach
// amount that accumulates (smoothed test) or counts (exact test), a smoothed
// or exact terminal payoff, a rebate at expiry or at the hit.  One launch
// prices B trades x G scenarios; the G scenarios of a trade (a Greeks ladder)
// share the trade's normals.
//
//   bgk_path_kernel<G, ANTI, GEN>  one workgroup = kChunk consecutive
//                                  observations of one trade; a thread takes
//                                  kPerThread of them, draws each normal pair
//                                  once and walks all G scenarios and both
//                                  signs with it; four sums per scenario in
//                                  index order (kept in the thread's LDS
//                                  column), fixed LDS tree, one partial per
//                                  workgroup into the workspace
//   bgk_finalize_kernel            one thread per (trade, scenario) adds the
//                                  partials in block order
//
// No floating-point atomics.  The chunk is a constant, a scenario's
// arithmetic does not depend on G, on its slot or on the trade's position, so
// its four sums are bit-identical under any grouping.
//
// Operation order is the reference's, with separately rounded multiply and
// add (contraction off): on supplied normals logS0 + c is the host engine's
// bit for bit and the two differ only through the device exp.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "fdcn_philox.h"
#include "fdcn_shared.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 16;
constexpr int kChunk = kThreads * kPerThread;  // observations per workgroup
constexpr int kMaxG = FDCN_BGK_MAX_G;
constexpr int kNS = FDCN_BGK_NSTAT;

struct Scenario {
  double log_s0, strike, hu, hd, eps_b, eps_p, rebate;
};

struct Path {
  double c;          // running sum of the log increments
  double breached;   // accumulated breach amount
  double rebate_pv;  // rebate at hit, already discounted
};

// monitored step: the breach amount of spot s, then the rebate at hit
__device__ __forceinline__ void monitor(Path& p, const Scenario& sc, int sides, int rebate_mode,
                                        double df_k) {
  const double s = exp(sc.log_s0 + p.c);
  double event = 0.0;
  if (sc.eps_b > 0.0) {
    if (sides & 1) {
      const double up = s < sc.hu - sc.eps_b
                            ? 0.0
                            : (s > sc.hu + sc.eps_b ? 1.0 : 0.5 + (s - sc.hu) / (2.0 * sc.eps_b));
      event = fmax(event, up);
    }
    if (sides & 2) {
      const double dn = s < sc.hd - sc.eps_b
                            ? 1.0
                            : (s > sc.hd + sc.eps_b ? 0.0 : 0.5 + (sc.hd - s) / (2.0 * sc.eps_b));
      event = fmax(event, dn);
    }
    if (rebate_mode == 2) {
      const double newly = fmax(0.0, event - (p.rebate_pv > 0.0 ? 1.0 : 0.0));
      p.rebate_pv += (newly * sc.rebate) * df_k;
    }
  } else {
    const bool hit = ((sides & 1) && s >= sc.hu) || ((sides & 2) && s <= sc.hd);
    event = hit ? 1.0 : 0.0;
    if (rebate_mode == 2 && hit && p.breached == 0.0) p.rebate_pv = sc.rebate * df_k;
  }
  p.breached += event;
}

// maturity: x = alive * intrinsic (+ rebate * (1 - alive) at expiry)
__device__ __forceinline__ double terminal(const Path& p, const Scenario& sc, bool put,
                                           int rebate_mode, double& alive) {
  const double s_T = exp(sc.log_s0 + p.c);
  alive = fmin(fmax(1.0 - p.breached, 0.0), 1.0);
  const double d = put ? sc.strike - s_T : s_T - sc.strike;
  double intrinsic;
  if (sc.eps_p > 0.0) {
    const double e = sc.eps_p;
    intrinsic = d < -e ? 0.0
                       : (d > e ? d : (0.5 * (d * d) + e * d + 0.5 * (e * e)) / (2.0 * e));
  } else {
    intrinsic = fmax(d, 0.0);
  }
  double x = alive * intrinsic;
  if (rebate_mode == 1) x = x + sc.rebate * (1.0 - alive);
  return x;
}

// A scenario's parameters, read where they are used.  They are uniform across
// the workgroup (scalar loads that hit the scalar cache); the opaque pointer
// keeps the compiler from hoisting all G rows out of the step loop, where 14
// SGPRs a scenario would not fit the scalar register file.
__device__ __forceinline__ Scenario load_scenario(const double* __restrict__ params, size_t row) {
  const double* P = params + row * FDCN_BGK_NPARAM;
  asm volatile("" : "+s"(P));
  Scenario sc;
  sc.log_s0 = P[FDCN_BGK_P_LOG_SPOT];
  sc.strike = P[FDCN_BGK_P_STRIKE];
  sc.hu = P[FDCN_BGK_P_UPPER];
  sc.hd = P[FDCN_BGK_P_LOWER];
  sc.eps_b = P[FDCN_BGK_P_EPS_BARRIER];
  sc.eps_p = P[FDCN_BGK_P_EPS_PAYOFF];
  sc.rebate = P[FDCN_BGK_P_REBATE];
  return sc;
}

struct BgkArgs {
  int32_t n_steps, n_blocks;
  int64_t n_obs, obs_first;
  uint64_t seed;
};

// The arrays are separate __restrict__ arguments: the per-step table and the
// parameters are uniform across a workgroup and read with scalar loads.
// Two workgroups per CU: 256 registers a thread hold the state of eight
// scenarios on both signs without scratch (211 VGPRs at G = 8).
template <int G, bool ANTI, bool GEN>
__global__ void __launch_bounds__(kThreads, 2)
bgk_path_kernel(BgkArgs a, const double* __restrict__ params, const int32_t* __restrict__ flags,
                const double* __restrict__ step, const double* __restrict__ z,
                double* __restrict__ ws, double* __restrict__ payoff_out) {
  constexpr int NS = ANTI ? 2 : 1;
  const int b = blockIdx.x / a.n_blocks;    // trade
  const int blk = blockIdx.x % a.n_blocks;  // chunk of observations
  const int tid = threadIdx.x;
  const int32_t* F = flags + (size_t)b * FDCN_BGK_NFLAG;
  const double* S = step + (size_t)b * G * a.n_steps * FDCN_BGK_NSTEP;
  const bool put = F[FDCN_BGK_F_PUT] != 0;
  const int sides = F[FDCN_BGK_F_SIDES] & 3;  // _dev callers: the host entry rejects the rest
  int rebate_mode = F[FDCN_BGK_F_REBATE_MODE];
  if (rebate_mode < 0 || rebate_mode > 2) rebate_mode = 0;
  const uint32_t stream = (uint32_t)F[FDCN_BGK_F_STREAM];
  const int64_t n_sim = a.n_obs * NS;

  // the thread's four sums per scenario live in its own LDS column: the
  // registers go to the path state
  __shared__ double sh[G][kNS][kThreads];
#pragma unroll
  for (int g = 0; g < G; ++g)
#pragma unroll
    for (int s = 0; s < kNS; ++s) sh[g][s][tid] = 0.0;

  for (int k = 0; k < kPerThread; ++k) {
    const int64_t i = (int64_t)blk * kChunk + (int64_t)k * kThreads + tid;
    if (i >= a.n_obs) break;
    Path p[G][NS];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
      for (int s = 0; s < NS; ++s) p[g][s] = Path{0.0, 0.0, 0.0};
    const double* zi = GEN ? nullptr : z + (size_t)i * a.n_steps;
    for (int m = 0; m < a.n_steps; m += 2) {
      double zz[2] = {0.0, 0.0};
      if (GEN) {
        fdcn_philox::normal_pair((uint64_t)(a.obs_first + i), (uint32_t)(m >> 1), stream, a.seed,
                                 zz[0], zz[1]);
      } else {
        zz[0] = zi[m];
        if (m + 1 < a.n_steps) zz[1] = zi[m + 1];
      }
#pragma unroll 1
      for (int h = 0; h < 2 && m + h < a.n_steps; ++h) {
        const double zh = h ? zz[1] : zz[0];
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const double* row = S + ((size_t)g * a.n_steps + (m + h)) * FDCN_BGK_NSTEP;
          const double drift = row[FDCN_BGK_S_DRIFT];
          const double dz = row[FDCN_BGK_S_DIFF] * zh;
          p[g][0].c += drift + dz;
          if (ANTI) p[g][1].c += drift - dz;  // diff * (-z) exactly
          if (row[FDCN_BGK_S_MONITOR] != 0.0 && sides != 0) {
            const double df_k = row[FDCN_BGK_S_DF_END];
            const Scenario sc = load_scenario(params, (size_t)b * G + g);
#pragma unroll
            for (int s = 0; s < NS; ++s) monitor(p[g][s], sc, sides, rebate_mode, df_k);
          }
        }
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const Scenario sc = load_scenario(params, (size_t)b * G + g);
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        double alive;
        const double x = terminal(p[g][s], sc, put, rebate_mode, alive);
        if (payoff_out) {
          double* o = payoff_out + ((size_t)b * G + g) * 2 * (size_t)n_sim +
                      (size_t)s * (size_t)a.n_obs + (size_t)i;
          o[0] = x;
          o[n_sim] = p[g][s].rebate_pv;
        }
        sh[g][0][tid] += x;
        sh[g][1][tid] += x * x;
        sh[g][2][tid] += p[g][s].rebate_pv;
        sh[g][3][tid] += 1.0 - alive;
      }
    }
  }

  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int s = 0; s < kNS; ++s) sh[g][s][tid] += sh[g][s][tid + off];
    }
    __syncthreads();
  }
  if (tid < G * kNS)
    ws[((size_t)b * a.n_blocks + blk) * G * kNS + tid] = sh[tid / kNS][tid % kNS][0];
}

// stats[b][g][s] = sum over the trade's workgroups, in block order
__global__ void __launch_bounds__(kThreads) bgk_finalize_kernel(int32_t B, int32_t G,
                                                                int32_t n_blocks,
                                                                const double* __restrict__ ws,
                                                                double* __restrict__ stats) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)B * G) return;
  const int64_t b = t / G;
  const int g = (int)(t % G);
  double acc[kNS] = {0.0, 0.0, 0.0, 0.0};
  for (int k = 0; k < n_blocks; ++k) {
    const double* w = ws + ((((size_t)b * n_blocks + k) * G) + g) * kNS;
#pragma unroll
    for (int s = 0; s < kNS; ++s) acc[s] += w[s];
  }
#pragma unroll
  for (int s = 0; s < kNS; ++s) stats[(size_t)t * kNS + s] = acc[s];
}

// ---- host side -------------------------------------------------------------
int bfail(int code, const char* msg) { return fdcn_internal::set_error(code, msg); }

int64_t blocks_for(int64_t n_obs) { return (n_obs + kChunk - 1) / kChunk; }

int64_t ws_bytes(int32_t B, int32_t G, int64_t n_obs) {
  return blocks_for(n_obs) * G * kNS * (int64_t)sizeof(double) * B;
}

// sizes every entry point checks, before any device call
int check_sizes(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs, int32_t antithetic) {
  if (B < 1) return bfail(FDCN_EINVAL, "mc_bgk_batch: B must be >= 1");
  if (G < 1 || G > kMaxG) return bfail(FDCN_EINVAL, "mc_bgk_batch: G must be in 1 .. 8");
  if (n_steps < 1) return bfail(FDCN_EINVAL, "mc_bgk_batch: n_steps must be >= 1");
  if (n_obs < 1) return bfail(FDCN_EINVAL, "mc_bgk_batch: n_obs must be >= 1");
  if (antithetic < 0 || antithetic > 1)
    return bfail(FDCN_EINVAL, "mc_bgk_batch: antithetic must be 0 or 1");
  if (n_obs > ((int64_t)1 << 40) || blocks_for(n_obs) * (int64_t)B > 0x7fffffffLL)
    return bfail(FDCN_EINVAL, "mc_bgk_batch: B * n_obs is beyond one launch's grid");
  return FDCN_OK;
}

int check_trades(int32_t B, int32_t G, const double* params, const int32_t* flags) {
  char msg[160];
  for (int32_t b = 0; b < B; ++b) {
    const int32_t* f = flags + (size_t)b * FDCN_BGK_NFLAG;
    const char* bad = nullptr;
    if (f[FDCN_BGK_F_PUT] < 0 || f[FDCN_BGK_F_PUT] > 1) bad = "flag put must be 0 or 1";
    else if (f[FDCN_BGK_F_SIDES] < 0 || f[FDCN_BGK_F_SIDES] > 3) bad = "flag sides must be 0..3";
    else if (f[FDCN_BGK_F_REBATE_MODE] < 0 || f[FDCN_BGK_F_REBATE_MODE] > 2)
      bad = "flag rebate mode must be 0..2";
    else if (f[FDCN_BGK_F_STREAM] < 0) bad = "flag stream id must be >= 0";
    for (int32_t g = 0; g < G && !bad; ++g) {
      const double* p = params + ((size_t)b * G + g) * FDCN_BGK_NPARAM;
      if (!isfinite(p[FDCN_BGK_P_LOG_SPOT])) bad = "log-spot must be finite";
      else if (!(p[FDCN_BGK_P_STRIKE] > 0.0)) bad = "strike must be positive";
      else if (!(p[FDCN_BGK_P_EPS_BARRIER] >= 0.0)) bad = "barrier epsilon must be >= 0";
      else if (!(p[FDCN_BGK_P_EPS_PAYOFF] >= 0.0)) bad = "payoff epsilon must be >= 0";
      else if ((f[FDCN_BGK_F_SIDES] & 1) && !(p[FDCN_BGK_P_UPPER] > 0.0))
        bad = "upper level must be positive where the upper side is active";
      else if ((f[FDCN_BGK_F_SIDES] & 2) && !(p[FDCN_BGK_P_LOWER] > 0.0))
        bad = "lower level must be positive where the lower side is active";
    }
    if (bad) {
      snprintf(msg, sizeof msg, "mc_bgk_batch: trade %d: %s", b, bad);
      return bfail(FDCN_EINVAL, msg);
    }
  }
  return FDCN_OK;
}

using KernelFn = void (*)(BgkArgs, const double*, const int32_t*, const double*, const double*,
                          double*, double*);

template <int G>
KernelFn pick(bool anti, bool gen) {
  return anti ? (gen ? bgk_path_kernel<G, true, true> : bgk_path_kernel<G, true, false>)
              : (gen ? bgk_path_kernel<G, false, true> : bgk_path_kernel<G, false, false>);
}

// every G of 1..8 has its own instance: no group pays for idle slots
KernelFn kernel_for(int32_t G, bool anti, bool gen) {
  switch (G) {
    case 1: return pick<1>(anti, gen);
    case 2: return pick<2>(anti, gen);
    case 3: return pick<3>(anti, gen);
    case 4: return pick<4>(anti, gen);
    case 5: return pick<5>(anti, gen);
    case 6: return pick<6>(anti, gen);
    case 7: return pick<7>(anti, gen);
    default: return pick<8>(anti, gen);
  }
}

int launch(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs, int32_t antithetic,
           const double* params, const int32_t* flags, const double* step, const double* z,
           uint64_t seed, int64_t obs_first, double* stats, double* payoff_out, double* workspace,
           hipStream_t stream) {
  BgkArgs a;
  a.n_steps = n_steps;
  a.n_blocks = (int32_t)blocks_for(n_obs);
  a.n_obs = n_obs;
  a.obs_first = obs_first;
  a.seed = seed;
  const dim3 grid((uint32_t)((int64_t)a.n_blocks * B)), block(kThreads);
  hipLaunchKernelGGL(kernel_for(G, antithetic != 0, z == nullptr), grid, block, 0, stream, a,
                     params, flags, step, z, workspace, payoff_out);
  if (hipGetLastError() != hipSuccess) return bfail(FDCN_EHIP, "mc_bgk_batch: launch failed");
  const int64_t rows = (int64_t)B * G;
  hipLaunchKernelGGL(bgk_finalize_kernel, dim3((uint32_t)((rows + kThreads - 1) / kThreads)),
                     block, 0, stream, B, G, a.n_blocks, workspace, stats);
  if (hipGetLastError() != hipSuccess) return bfail(FDCN_EHIP, "mc_bgk_batch: launch failed");
  return FDCN_OK;
}

}  // namespace

extern "C" {

int fdcn_mc_bgk_plan(int64_t n_obs, int32_t G, int32_t* blocks_per_trade, int32_t* obs_per_block,
                     int64_t* ws_bytes_per_trade) {
  if (n_obs < 1 || n_obs > ((int64_t)1 << 40))
    return bfail(FDCN_EINVAL, "mc_bgk_plan: n_obs must be in 1 .. 2^40");
  if (G < 1 || G > kMaxG) return bfail(FDCN_EINVAL, "mc_bgk_plan: G must be in 1 .. 8");
  if (blocks_per_trade) *blocks_per_trade = (int32_t)blocks_for(n_obs);
  if (obs_per_block) *obs_per_block = kChunk;
  if (ws_bytes_per_trade) *ws_bytes_per_trade = ws_bytes(1, G, n_obs);
  return FDCN_OK;
}

int fdcn_mc_bgk_batch_dev(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs,
                          int32_t antithetic, const double* params, const int32_t* flags,
                          const double* step, const double* z, uint64_t seed, int64_t obs_first,
                          double* stats, double* payoff_out, double* workspace,
                          int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(B, G, n_steps, n_obs, antithetic);
  if (rc) return rc;
  if (!params) return bfail(FDCN_EINVAL, "mc_bgk_batch_dev: params is NULL");
  if (!flags) return bfail(FDCN_EINVAL, "mc_bgk_batch_dev: flags is NULL");
  if (!step) return bfail(FDCN_EINVAL, "mc_bgk_batch_dev: step is NULL");
  if (!stats) return bfail(FDCN_EINVAL, "mc_bgk_batch_dev: stats is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_bgk_batch_dev", "this launch needs (fdcn_mc_bgk_plan)", workspace, workspace_bytes,
      ws_bytes(B, G, n_obs), (hipStream_t)stream, [&](void* ws) {
        return launch(B, G, n_steps, n_obs, antithetic, params, flags, step, z, seed, obs_first,
                      stats, payoff_out, (double*)ws, (hipStream_t)stream);
      });
}

int fdcn_mc_bgk_batch(int32_t B, int32_t G, int32_t n_steps, int64_t n_obs, int32_t antithetic,
                      const double* params, const int32_t* flags, const double* step,
                      const double* z, uint64_t seed, int64_t obs_first, double* stats,
                      double* payoff_out) {
  int rc = check_sizes(B, G, n_steps, n_obs, antithetic);
  if (rc) return rc;
  if (!params) return bfail(FDCN_EINVAL, "mc_bgk_batch: params is NULL");
  if (!flags) return bfail(FDCN_EINVAL, "mc_bgk_batch: flags is NULL");
  if (!step) return bfail(FDCN_EINVAL, "mc_bgk_batch: step is NULL");
  if (!stats) return bfail(FDCN_EINVAL, "mc_bgk_batch: stats is NULL");
  rc = check_trades(B, G, params, flags);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_bgk_batch");
  if ((rc = c.open())) return rc;
  const size_t rows = (size_t)B * (size_t)G;
  const size_t n_sim = (size_t)n_obs * (antithetic ? 2 : 1);
  const int rP = c.in(params, sizeof(double) * rows * FDCN_BGK_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * (size_t)B * FDCN_BGK_NFLAG);
  const int rS = c.in(step, sizeof(double) * rows * (size_t)n_steps * FDCN_BGK_NSTEP);
  const int rZ = c.in(z, sizeof(double) * (size_t)n_obs * (size_t)n_steps);
  const int rO = c.out(stats, sizeof(double) * rows * FDCN_BGK_NSTAT);
  const int rY = c.out(payoff_out, sizeof(double) * rows * 2 * n_sim);
  const int rW = c.scratch((size_t)ws_bytes(B, G, n_obs));
  return c.run([&](hipStream_t stream) {
    return launch(B, G, n_steps, n_obs, antithetic, c.dev<double>(rP), c.dev<int32_t>(rF),
                  c.dev<double>(rS), c.dev<double>(rZ), seed, obs_first, c.dev<double>(rO),
                  c.dev<double>(rY), c.dev<double>(rW), stream);
  });
}

}  // extern "C"
