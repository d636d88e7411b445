// fdcn_mc_policy.hip -- Monte Carlo lower bound and Andersen-Broadie dual upper
// bound under a given per-step exercise table, for gfx950.
//
// The least-squares Monte Carlo (fdcn_mc_lsm.hip) fits its stopping rule; here
// the rule is an input: a band [X_LO_m, X_HI_m] in the log-spot per step, for
// instance the exercise boundary a Bermudan FD pricer has computed.  Any rule
// gives a lower bound and any rule gives a dual upper bound, so the table can
// drive both.  The rule, the event rules and the Philox mapping are the
// contract of include/fdcn.h (fdcn_mc_policy_batch, fdcn_mc_policy_dual_batch);
// the path step itself is fdcn_mc_policy.h.
//
//   policy_kernel<ANTI>      one workgroup of 256 threads = one sub-run of one
//                            contract = the LSM's price set of that sub-run,
//                            path for path.  A thread walks its 16 slots one
//                            after the other (two at a time under antithetic:
//                            +z and -z of one draw); a wave leaves the step
//                            loop when all its lanes have stopped.  No
//                            regression, so no path state is kept across
//                            slots: the registers are those of one walk.
//   policy_finalize_kernel   one thread per contract adds the sub-run means in
//                            sub-run order.
//   policy_dual_kernel<ANTI> fdcn_mc_dual.hip's dual_kernel with the table in
//                            the place of the coefficient rows: the outer path
//                            walked by every thread alike, n_inner / 256 inner
//                            walks per thread at a start step.
//   policy_dual_finalize_kernel
//
// Step rows and policy rows are uniform across the workgroup at every point of
// every walk (the step index is a loop counter), so they are read with scalar
// loads straight from global memory; LDS holds the reduction row only.  No
// floating-point atomics; multiply and add are rounded separately (contraction
// off), and the sums are the LSM's and the dual's, so a never-stop table
// reproduces those kernels bit for bit.
//
// Both kernels have a second template parameter DIV (the fdcn_mc_policy_div_batch
// and fdcn_mc_policy_dual_div_batch entries): a step may pay a cash dividend
// D_m, read from the row div[b][n_steps] with scalar loads like the step rows,
// so the branch on D_m != 0 is uniform.  Every walk goes forward: after the move
// the spot goes through g (fdcn_mc_div.h), then the step's events see the
// ex-dividend spot.  No per-path state is added; DIV = false is the kernel
// without any of it.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "fdcn_philox.h"
#include "fdcn_shared.h"

#pragma clang fp contract(off)

#include "fdcn_mc_policy.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kPerThread = 16;
constexpr int kSubrun = kThreads * kPerThread;
constexpr int kWsRow = 4;  // lower: sum v, min margin, stops, -; dual: as fdcn_mc_dual.hip
constexpr int kObsBits = 14, kStepBits = 9, kOuterBits = 10;
static_assert(kSubrun == FDCN_LSM_SUBRUN, "fdcn.h");
static_assert((1 << kObsBits) == FDCN_DUAL_MAX_INNER, "fdcn.h");
static_assert((1 << kStepBits) == FDCN_LSM_MAX_STEPS, "fdcn.h");
static_assert((1 << kOuterBits) == FDCN_DUAL_MAX_OUTER, "fdcn.h");
static_assert(FDCN_POLICY_NCOL == 2, "fdcn.h");

using fdcn_philox::normal_pair;
using fdcn_policy::band_margin;
using fdcn_policy::breach;
using fdcn_policy::Contract;
using fdcn_policy::load_contract;
using fdcn_policy::path_step;
using fdcn_policy::payoff;

struct PolicyArgs {
  int32_t n_steps, G;
  int64_t obs_first;
  uint64_t seed;
};

struct DualArgs {
  int32_t n_steps, G, n_outer, n_inner;
  int64_t subrun_first;
  uint64_t seed;
};

// a value every lane holds alike, as the compiler can see it
__device__ __forceinline__ double uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// The fixed tree over the workgroup, v[t] (op) v[t + off] for off = 128 .. 1:
// the two widest levels through LDS, the rest inside wave 0.  Two barriers;
// sh[kThreads] carries the result, so the next call's sh[t] writes cannot pass
// a late reader.
template <bool MIN>
__device__ __forceinline__ double block_reduce(double* sh, double v, int tid) {
  sh[tid] = v;
  __syncthreads();
  if (tid < kWave) {
    const double a = sh[tid], b = sh[tid + 128], c = sh[tid + 64], d = sh[tid + 192];
    double w = MIN ? fmin(fmin(a, b), fmin(c, d)) : (a + b) + (c + d);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const double o = __shfl_down(w, off, kWave);
      w = MIN ? fmin(w, o) : w + o;
    }
    if (tid == 0) sh[kThreads] = w;
  }
  __syncthreads();
  return uniform(sh[kThreads]);
}

// ---- the lower bound --------------------------------------------------------
// 107 / 102 VGPRs (antithetic / not), no scratch: 4 waves per SIMD, against the
// LSM kernel's one.  With dividends 111 / 105, still 4 waves.
template <bool ANTI, bool DIV>
__global__ void __launch_bounds__(kThreads)
policy_kernel(PolicyArgs a, const double* __restrict__ params, const int32_t* __restrict__ flags,
              const double* __restrict__ step, const double* __restrict__ policy,
              double* __restrict__ ws, double* __restrict__ values_out,
              const double* __restrict__ div) {
  constexpr int kObs = ANTI ? kPerThread / 2 : kPerThread;  // observations per thread
  const int b = blockIdx.x / a.G;  // contract
  const int g = blockIdx.x % a.G;  // sub-run
  const int tid = threadIdx.x;
  const int M = a.n_steps;
  const double* P = params + (size_t)b * FDCN_LSM_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_LSM_NFLAG;
  const double* S = step + (size_t)b * M * FDCN_LSM_NSTEP;
  const double* T = policy + (size_t)b * M * FDCN_POLICY_NCOL;
  const double* D = DIV ? div + (size_t)b * M : nullptr;  // uniform, like S
  const Contract c = load_contract(P, F);
  const uint32_t w_price = 2u * (uint32_t)F[FDCN_LSM_F_STREAM] + 1u;  // the LSM's price set
  const double x0 = log(P[FDCN_LSM_P_SPOT]);
  const uint64_t obs0 = (uint64_t)(a.obs_first + (int64_t)g * (kObs * kThreads) + tid);
  double* vout = values_out ? values_out + ((size_t)b * a.G + g) * kSubrun + tid : nullptr;

  __shared__ double sh[kThreads + 1];

  double margin = INFINITY, sum_v = 0.0;
  uint64_t walked = 0;  // not reported: the compiler drops it
  uint32_t stopped = 0;
  for (int j = 0; j < kObs; ++j) {
    const uint64_t obs = obs0 + (uint64_t)(j * kThreads);
    double xa = x0, xb = x0, va = 0.0, vb = 0.0;
    bool da = false, db = !ANTI, ia = false, ib = false;
    for (int i = 0; i < M; i += 2) {
      double zz[2];
      normal_pair(obs, (uint32_t)(i >> 1), w_price, a.seed, zz[0], zz[1]);
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int ii = i + hf;
        if (ii >= M) break;
        const double* ri = S + (size_t)ii * FDCN_LSM_NSTEP;
        const double* ti = T + (size_t)ii * FDCN_POLICY_NCOL;
        const bool last = ii + 1 == M;
        const double dv = DIV ? fdcn_div::div_at(D, ii) : 0.0;
        path_step(c, ri, ti, last, zz[hf], dv, xa, da, ia, va, margin, walked, stopped);
        if (ANTI)
          path_step(c, ri, ti, last, -zz[hf], dv, xb, db, ib, vb, margin, walked, stopped);
      }
      if (da && db) break;
    }
    // slot order: k = j, or k = 2 j (+z) and 2 j + 1 (-z)
    sum_v += va;
    if (ANTI) sum_v += vb;
    if (vout) {
      vout[(size_t)((ANTI ? 2 : 1) * j) * kThreads] = va;
      if (ANTI) vout[(size_t)(2 * j + 1) * kThreads] = vb;
    }
  }

  const double tot_v = block_reduce<false>(sh, sum_v, tid);
  const double tot_margin = block_reduce<true>(sh, margin, tid);
  const double tot_stopped = block_reduce<false>(sh, (double)stopped, tid);  // exact
  if (tid == 0) {
    double* w = ws + ((size_t)b * a.G + g) * kWsRow;
    w[0] = tot_v;
    w[1] = tot_margin;
    w[2] = tot_stopped;
    w[3] = 0.0;
  }
}

__global__ void __launch_bounds__(kThreads)
policy_finalize_kernel(int32_t B, int32_t G, const double* __restrict__ ws,
                       double* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* w = ws + (size_t)b * G * kWsRow;
  double s = 0.0, s2 = 0.0, margin = INFINITY, stopped = 0.0;
  for (int g = 0; g < G; ++g) {
    const double mv = w[kWsRow * g] / (double)kSubrun;
    s += mv;
    s2 += mv * mv;
    margin = fmin(margin, w[kWsRow * g + 1]);
    stopped += w[kWsRow * g + 2];
  }
  const double n = (double)G;
  double* o = stats + (size_t)b * FDCN_POLICY_NSTAT;
  o[FDCN_POLICY_O_PRICE] = s / n;
  o[FDCN_POLICY_O_STDERR] = G > 1 ? sqrt(fmax(0.0, s2 - s * s / n) / (n - 1.0) / n) : 0.0;
  o[FDCN_POLICY_O_SUM] = s;
  o[FDCN_POLICY_O_SUM2] = s2;
  o[FDCN_POLICY_O_MIN_MARGIN] = margin;
  o[FDCN_POLICY_O_EXERCISED] = stopped;
}

// ---- the dual upper bound ---------------------------------------------------
// fdcn_mc_dual.hip's dual_kernel, statement for statement, with the table rule:
// 128 / 125 VGPRs (antithetic / not) under the bound of 4 waves per SIMD, no
// scratch.  The antithetic instance with dividends spills under that bound and
// is bound to 3 waves instead.
template <bool ANTI, bool DIV>
__global__ void __launch_bounds__(kThreads, (ANTI && DIV) ? 3 : 4)
policy_dual_kernel(DualArgs a, const double* __restrict__ params,
                   const int32_t* __restrict__ flags, const double* __restrict__ step,
                   const double* __restrict__ policy, double* __restrict__ ws,
                   double* __restrict__ gap_out, double* __restrict__ cont_out,
                   const double* __restrict__ div) {
  const int b = blockIdx.x / a.G;  // contract
  const int g = blockIdx.x % a.G;  // sub-run
  const int tid = threadIdx.x;
  const int M = a.n_steps;
  const double* P = params + (size_t)b * FDCN_LSM_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_LSM_NFLAG;
  const double* S = step + (size_t)b * M * FDCN_LSM_NSTEP;
  const double* T = policy + (size_t)b * M * FDCN_POLICY_NCOL;
  const double* Dv = DIV ? div + (size_t)b * M : nullptr;  // uniform, like S
  const Contract c = load_contract(P, F);
  const uint32_t sid = (uint32_t)F[FDCN_LSM_F_STREAM];
  const uint32_t w_outer = 0x80000000u + 2u * sid, w_inner = w_outer + 1u;
  const double x0 = log(P[FDCN_LSM_P_SPOT]);
  const uint64_t gs = (uint64_t)(a.subrun_first + (int64_t)g);  // absolute sub-run
  const int n_obs_t = a.n_inner / kThreads / (ANTI ? 2 : 1);     // observations per thread
  const double n_inner_d = (double)a.n_inner;

  __shared__ double sh[kThreads + 1];

  double margin = INFINITY;  // outer decisions (uniform) and this thread's inner ones
  uint64_t walked = 0;       // inner path-steps of this thread
  uint32_t stopped = 0;      // not reported
  double sum_d = 0.0;        // uniform
  int64_t starts = 0;        // uniform

  for (int p = 0; p < a.n_outer; ++p) {
    const uint64_t obs_outer = gs * (uint64_t)a.n_outer + (uint64_t)p;
    const size_t row_out = ((size_t)b * a.G + g) * (size_t)a.n_outer + (size_t)p;
    double* cont = cont_out ? cont_out + row_out * (size_t)M : nullptr;
    double x = x0, r = 0.0, D = -INFINITY;
    bool in = false;
    double z0 = 0.0, z1 = 0.0;
    int i = 0;
    for (; i < M; ++i) {  // step m = i + 1
      if (!(i & 1)) normal_pair(obs_outer, (uint32_t)(i >> 1), w_outer, a.seed, z0, z1);
      const double* row = S + (size_t)i * FDCN_LSM_NSTEP;
      const double* tr = T + (size_t)i * FDCN_POLICY_NCOL;
      x += row[FDCN_LSM_S_DRIFT] + row[FDCN_LSM_S_DIFF] * ((i & 1) ? z1 : z0);
      if (DIV) {  // the dividend, then the step's events on the ex-dividend spot
        const double dv = fdcn_div::div_at(Dv, i);
        if (dv != 0.0) x = fdcn_div::div_forward(x, dv);
      }
      const bool last = i + 1 == M;
      const bool mon = c.use_mon && row[FDCN_LSM_S_MONITOR] != 0.0;
      const bool ex = !last && row[FDCN_LSM_S_EXERCISE] != 0.0;
      double chat = 0.0;
      bool forced = last;
      if (mon || ex || last) {
        const double s = exp(x);
        const double phi = payoff(c, s);
        const bool hit = mon && breach(c, s);
        if (c.ko && hit) forced = true;
        if (c.ki && hit) in = true;
        const bool elig = c.ki ? in : true;
        const double lo = tr[FDCN_POLICY_X_LO], hi = tr[FDCN_POLICY_X_HI];
        // the decision is taken whatever phi is, as in path_step
        if (!forced && ex && elig) margin = fmin(margin, band_margin(x, lo, hi));
        if (!forced && ex && elig && phi > 0.0) {
          // ---- the inner simulation from (x, in) at step m, steps m + 1 .. M
          const uint64_t base =
              ((((gs << kOuterBits) + (uint64_t)p) << kStepBits) + (uint64_t)i) << kObsBits;
          const int n_rem = M - (i + 1);
          double sum = 0.0;
          for (int j = 0; j < n_obs_t; ++j) {
            const uint64_t obs = base + (uint64_t)(j * kThreads + tid);
            double xa = x, xb = x, va = 0.0, vb = 0.0;
            bool da = false, db = !ANTI, ia = in, ib = in;
            for (int t = 0; t < n_rem; t += 2) {
              double zz[2];
              normal_pair(obs, (uint32_t)(t >> 1), w_inner, a.seed, zz[0], zz[1]);
#pragma unroll
              for (int hf = 0; hf < 2; ++hf) {
                if (hf == 1 && t + 1 >= n_rem) break;
                const int ii = i + 1 + t + hf;
                const double* ri = S + (size_t)ii * FDCN_LSM_NSTEP;
                const double* ti = T + (size_t)ii * FDCN_POLICY_NCOL;
                const bool li = ii + 1 == M;
                const double dv = DIV ? fdcn_div::div_at(Dv, ii) : 0.0;
                path_step(c, ri, ti, li, zz[hf], dv, xa, da, ia, va, margin, walked, stopped);
                if (ANTI)
                  path_step(c, ri, ti, li, -zz[hf], dv, xb, db, ib, vb, margin, walked,
                            stopped);
              }
              if (da && db) break;
            }
            sum += va;
            if (ANTI) sum += vb;
          }
          chat = block_reduce<false>(sh, sum, tid) / n_inner_d;
          ++starts;
          // ---- the candidate of step m
          const double Z = phi * row[FDCN_LSM_S_DF_END];
          if (lo <= x && x <= hi) {
            D = fmax(D, 0.0 - r);
            r += Z - chat;
          } else {
            D = fmax(D, (Z - chat) - r);
          }
        }
      }
      if (cont && tid == 0) cont[i] = chat;
      if (forced) {
        D = fmax(D, 0.0 - r);
        break;
      }
    }
    // the steps after a knock-out: no inner simulation
    if (cont)
      for (int k = i + 1 + tid; k < M; k += kThreads) cont[k] = 0.0;
    if (gap_out && tid == 0) gap_out[row_out] = D;
    sum_d += D;
  }

  const double tot_margin = block_reduce<true>(sh, margin, tid);
  const double tot_walked = block_reduce<false>(sh, (double)walked, tid);  // exact below 2^53
  if (tid == 0) {
    double* w = ws + ((size_t)b * a.G + g) * kWsRow;
    w[0] = sum_d;
    w[1] = tot_margin;
    w[2] = (double)starts * (double)a.n_inner;
    w[3] = tot_walked;
  }
}

__global__ void __launch_bounds__(kThreads)
policy_dual_finalize_kernel(int32_t B, int32_t G, int32_t n_outer,
                            const double* __restrict__ ws, double* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* w = ws + (size_t)b * G * kWsRow;
  double s = 0.0, s2 = 0.0, margin = INFINITY, paths = 0.0, steps = 0.0;
  for (int g = 0; g < G; ++g) {
    const double gap = w[kWsRow * g] / (double)n_outer;
    s += gap;
    s2 += gap * gap;
    margin = fmin(margin, w[kWsRow * g + 1]);
    paths += w[kWsRow * g + 2];
    steps += w[kWsRow * g + 3];
  }
  const double n = (double)G;
  double* o = stats + (size_t)b * FDCN_DUAL_NSTAT;
  o[FDCN_DUAL_O_GAP] = s / n;
  o[FDCN_DUAL_O_STDERR] = G > 1 ? sqrt(fmax(0.0, s2 - s * s / n) / (n - 1.0) / n) : 0.0;
  o[FDCN_DUAL_O_SUM] = s;
  o[FDCN_DUAL_O_SUM2] = s2;
  o[FDCN_DUAL_O_MIN_MARGIN] = margin;
  o[FDCN_DUAL_O_INNER_PATHS] = paths;
  o[FDCN_DUAL_O_INNER_STEPS] = steps;
}

// ---- host side -------------------------------------------------------------
int pfail(const char* who, int code, const char* what) {
  char msg[240];
  snprintf(msg, sizeof msg, "%s: %s", who, what);
  return fdcn_internal::set_error(code, msg);
}

int obs_per_subrun(int32_t antithetic) { return antithetic ? kSubrun / 2 : kSubrun; }

// the sizes both bounds share (those of fdcn_mc_lsm_batch)
int check_common(const char* who, int32_t B, int32_t n_steps, int32_t G, int32_t antithetic) {
  if (B < 1) return pfail(who, FDCN_EINVAL, "B must be >= 1");
  if (G < 1) return pfail(who, FDCN_EINVAL, "G must be >= 1");
  if (n_steps < 1 || n_steps > FDCN_LSM_MAX_STEPS)
    return pfail(who, FDCN_EINVAL, "n_steps must be in 1 .. FDCN_LSM_MAX_STEPS (512)");
  if (antithetic < 0 || antithetic > 1)
    return pfail(who, FDCN_EINVAL, "antithetic must be 0 or 1");
  if ((int64_t)B * (int64_t)G > 0x7fffffffLL)
    return pfail(who, FDCN_EINVAL, "B * G is beyond one launch's grid");
  return FDCN_OK;
}

int check_lower_sizes(const char* who, int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                      int64_t obs_first) {
  const int rc = check_common(who, B, n_steps, G, antithetic);
  if (rc) return rc;
  if (obs_first < 0 || obs_first > ((int64_t)1 << 56) ||
      obs_first % obs_per_subrun(antithetic) != 0)
    return pfail(who, FDCN_EINVAL, "obs_first must be a non-negative multiple of the "
                                   "observations per sub-run (fdcn_mc_policy_plan)");
  return FDCN_OK;
}

int check_dual_sizes(const char* who, int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                     int32_t n_outer, int32_t n_inner, int64_t subrun_first) {
  const int rc = check_common(who, B, n_steps, G, antithetic);
  if (rc) return rc;
  if (n_outer < 1 || n_outer > FDCN_DUAL_MAX_OUTER)
    return pfail(who, FDCN_EINVAL, "n_outer must be in 1 .. FDCN_DUAL_MAX_OUTER (1024)");
  const int32_t unit = antithetic ? 2 * kThreads : kThreads;
  if (n_inner < unit || n_inner > FDCN_DUAL_MAX_INNER || n_inner % unit != 0)
    return pfail(who, FDCN_EINVAL, "n_inner must be a multiple of 256 (512 when antithetic) up "
                                   "to FDCN_DUAL_MAX_INNER (16384)");
  if (subrun_first < 0 || subrun_first + (int64_t)G > ((int64_t)1 << 31))
    return pfail(who, FDCN_EINVAL, "subrun_first must be >= 0 and subrun_first + G at most 2^31");
  return FDCN_OK;
}

int check_pointers(const char* who, const void* params, const void* flags, const void* step,
                   const void* policy, const void* stats) {
  const char* bad = !params ? "params is NULL" : !flags ? "flags is NULL"
                    : !step ? "step is NULL" : !policy ? "policy is NULL"
                    : !stats ? "stats is NULL" : nullptr;
  return bad ? pfail(who, FDCN_EINVAL, bad) : FDCN_OK;
}

// the LSM host entry's checks of a contract, a NaN in the table and, for the
// dual (`cashflows`), a negative rebate
int check_contracts(const char* who, int32_t B, int32_t n_steps, const double* params,
                    const int32_t* flags, const double* step, const double* policy,
                    bool cashflows) {
  char msg[160];
  for (int32_t b = 0; b < B; ++b) {
    const int32_t* f = flags + (size_t)b * FDCN_LSM_NFLAG;
    const double* p = params + (size_t)b * FDCN_LSM_NPARAM;
    const double* s = step + (size_t)b * n_steps * FDCN_LSM_NSTEP;
    const double* t = policy + (size_t)b * n_steps * FDCN_POLICY_NCOL;
    const int kind = f[FDCN_LSM_F_KIND];
    const bool lo = kind == 1 || kind == 3 || kind == 4 || kind == 6;
    const bool hi = kind == 2 || kind == 3 || kind == 5 || kind == 6;
    const char* bad = nullptr;
    if (f[FDCN_LSM_F_PUT] < 0 || f[FDCN_LSM_F_PUT] > 1) bad = "flag put must be 0 or 1";
    else if (kind < 0 || kind > 6) bad = "flag kind must be 0..6";
    else if (f[FDCN_LSM_F_STREAM] < 0 || f[FDCN_LSM_F_STREAM] >= (1 << 30))
      bad = "flag stream id must be in 0 .. 2^30 - 1";
    else if (!(p[FDCN_LSM_P_SPOT] > 0.0) || !isfinite(p[FDCN_LSM_P_SPOT]))
      bad = "spot must be positive";
    else if (!(p[FDCN_LSM_P_STRIKE] > 0.0) || !isfinite(p[FDCN_LSM_P_STRIKE]))
      bad = "strike must be positive";
    else if (lo && !(p[FDCN_LSM_P_LOWER] > 0.0)) bad = "lower level must be positive";
    else if (hi && !(p[FDCN_LSM_P_UPPER] > 0.0)) bad = "upper level must be positive";
    else if (lo && hi && !(p[FDCN_LSM_P_LOWER] < p[FDCN_LSM_P_UPPER]))
      bad = "lower level must be below the upper level";
    for (int32_t m = 0; m < n_steps && !bad; ++m) {
      const double* r = s + (size_t)m * FDCN_LSM_NSTEP;
      for (int q = 0; q < FDCN_LSM_NSTEP; ++q)
        if (!isfinite(r[q])) bad = "a step entry is not finite";
      if (bad) break;
      if (!(r[FDCN_LSM_S_DIFF] > 0.0)) bad = "step DIFF must be positive (sigma > 0)";
      else if (!(r[FDCN_LSM_S_ISCALE] > 0.0)) bad = "step ISCALE must be positive";
      else if (cashflows && kind != 0 && r[FDCN_LSM_S_REBATE] < 0.0)
        bad = "a step REBATE is negative (every cashflow must be >= 0)";
      else if (isnan(t[FDCN_POLICY_NCOL * m]) || isnan(t[FDCN_POLICY_NCOL * m + 1]))
        bad = "a policy entry is NaN (+-inf are legal)";
    }
    if (bad) {
      snprintf(msg, sizeof msg, "contract %d: %s", b, bad);
      return pfail(who, FDCN_EINVAL, msg);
    }
  }
  return FDCN_OK;
}

// every dividend finite and >= 0 (a dividend on the last step is legal)
int check_dividends(const char* who, int32_t B, int32_t n_steps, const double* div) {
  char msg[160];
  for (int32_t b = 0; b < B; ++b)
    for (int32_t m = 0; m < n_steps; ++m) {
      const double d = div[(size_t)b * n_steps + m];
      if (isfinite(d) && d >= 0.0) continue;
      snprintf(msg, sizeof msg, "contract %d: the dividend of step %d %s", b, m + 1,
               isfinite(d) ? "is negative" : "is not finite");
      return pfail(who, FDCN_EINVAL, msg);
    }
  return FDCN_OK;
}

int64_t ws_bytes(int32_t G) { return (int64_t)G * kWsRow * (int64_t)sizeof(double); }

// `div` non-null: the DIV instances, an all-zero row included
int launch_lower(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, const double* params,
                 const int32_t* flags, const double* step, const double* policy, uint64_t seed,
                 int64_t obs_first, double* stats, double* values_out, double* workspace,
                 hipStream_t stream, const double* div = nullptr) {
  PolicyArgs a;
  a.n_steps = n_steps;
  a.G = G;
  a.obs_first = obs_first;
  a.seed = seed;
  const dim3 grid((uint32_t)((int64_t)B * G)), block(kThreads);
  auto fn = div ? (antithetic ? policy_kernel<true, true> : policy_kernel<false, true>)
                : (antithetic ? policy_kernel<true, false> : policy_kernel<false, false>);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, a, params, flags, step, policy, workspace,
                     values_out, div);
  if (hipGetLastError() != hipSuccess)
    return pfail("mc_policy_batch", FDCN_EHIP, "launch failed");
  hipLaunchKernelGGL(policy_finalize_kernel, dim3((B + kThreads - 1) / kThreads), block, 0,
                     stream, B, G, workspace, stats);
  if (hipGetLastError() != hipSuccess)
    return pfail("mc_policy_batch", FDCN_EHIP, "launch failed");
  return FDCN_OK;
}

int launch_dual(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                int32_t n_inner, const double* params, const int32_t* flags, const double* step,
                const double* policy, uint64_t seed, int64_t subrun_first, double* stats,
                double* gap_out, double* cont_out, double* workspace, hipStream_t stream,
                const double* div = nullptr) {
  DualArgs a;
  a.n_steps = n_steps;
  a.G = G;
  a.n_outer = n_outer;
  a.n_inner = n_inner;
  a.subrun_first = subrun_first;
  a.seed = seed;
  const dim3 grid((uint32_t)((int64_t)B * G)), block(kThreads);
  auto fn = div ? (antithetic ? policy_dual_kernel<true, true> : policy_dual_kernel<false, true>)
                : (antithetic ? policy_dual_kernel<true, false>
                              : policy_dual_kernel<false, false>);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, a, params, flags, step, policy, workspace,
                     gap_out, cont_out, div);
  if (hipGetLastError() != hipSuccess)
    return pfail("mc_policy_dual_batch", FDCN_EHIP, "launch failed");
  hipLaunchKernelGGL(policy_dual_finalize_kernel, dim3((B + kThreads - 1) / kThreads), block, 0,
                     stream, B, G, n_outer, workspace, stats);
  if (hipGetLastError() != hipSuccess)
    return pfail("mc_policy_dual_batch", FDCN_EHIP, "launch failed");
  return FDCN_OK;
}


// The four lower-bound entries: `with_div` is the div form of the contract (div
// must be there, and a DIV instance runs); div is null otherwise.
int lower_dev(const char* who, bool with_div, int32_t B, int32_t n_steps, int32_t G,
              int32_t antithetic, const double* params, const int32_t* flags,
              const double* step, const double* div, const double* policy, uint64_t seed,
              int64_t obs_first, double* stats, double* values_out, double* workspace,
              int64_t workspace_bytes, void* stream) {
  int rc = check_lower_sizes(who, B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers(who, params, flags, step, policy, stats);
  if (rc) return rc;
  if (with_div && !div) return pfail(who, FDCN_EINVAL, "div is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      who, "this launch needs (fdcn_mc_policy_plan)", workspace, workspace_bytes,
      ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch_lower(B, n_steps, G, antithetic, params, flags, step, policy, seed,
                            obs_first, stats, values_out, (double*)ws, (hipStream_t)stream, div);
      });
}

int lower_host(const char* who, bool with_div, int32_t B, int32_t n_steps, int32_t G,
               int32_t antithetic, const double* params, const int32_t* flags,
               const double* step, const double* div, const double* policy, uint64_t seed,
               int64_t obs_first, double* stats, double* values_out) {
  int rc = check_lower_sizes(who, B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers(who, params, flags, step, policy, stats);
  if (rc) return rc;
  if (with_div && !div) return pfail(who, FDCN_EINVAL, "div is NULL");
  rc = check_contracts(who, B, n_steps, params, flags, step, policy, false);
  if (rc) return rc;
  if (with_div && (rc = check_dividends(who, B, n_steps, div))) return rc;
  fdcn_internal::HostCall c(who);
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rT = c.in(policy, sizeof(double) * nb * (size_t)n_steps * FDCN_POLICY_NCOL);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_POLICY_NSTAT);
  const int rY = c.out(values_out, sizeof(double) * nb * (size_t)G * kSubrun);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  const int rD = c.in(div, sizeof(double) * nb * (size_t)n_steps);  // no room where null
  return c.run([&](hipStream_t stream) {
    return launch_lower(B, n_steps, G, antithetic, c.dev<double>(rP), c.dev<int32_t>(rF),
                        c.dev<double>(rS), c.dev<double>(rT), seed, obs_first,
                        c.dev<double>(rO), c.dev<double>(rY), c.dev<double>(rW), stream,
                        c.dev<double>(rD));
  });
}

// The four dual entries, in the same way.
int dual_dev(const char* who, bool with_div, int32_t B, int32_t n_steps, int32_t G,
             int32_t antithetic, int32_t n_outer, int32_t n_inner, const double* params,
             const int32_t* flags, const double* step, const double* div, const double* policy,
             uint64_t seed, int64_t subrun_first, double* stats, double* gap_out,
             double* cont_out, double* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_dual_sizes(who, B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers(who, params, flags, step, policy, stats);
  if (rc) return rc;
  if (with_div && !div) return pfail(who, FDCN_EINVAL, "div is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      who, "this launch needs (fdcn_mc_policy_dual_plan)", workspace, workspace_bytes,
      ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch_dual(B, n_steps, G, antithetic, n_outer, n_inner, params, flags, step,
                           policy, seed, subrun_first, stats, gap_out, cont_out, (double*)ws,
                           (hipStream_t)stream, div);
      });
}

int dual_host(const char* who, bool with_div, int32_t B, int32_t n_steps, int32_t G,
              int32_t antithetic, int32_t n_outer, int32_t n_inner, const double* params,
              const int32_t* flags, const double* step, const double* div, const double* policy,
              uint64_t seed, int64_t subrun_first, double* stats, double* gap_out,
              double* cont_out) {
  int rc = check_dual_sizes(who, B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers(who, params, flags, step, policy, stats);
  if (rc) return rc;
  if (with_div && !div) return pfail(who, FDCN_EINVAL, "div is NULL");
  rc = check_contracts(who, B, n_steps, params, flags, step, policy, true);
  if (rc) return rc;
  if (with_div && (rc = check_dividends(who, B, n_steps, div))) return rc;
  fdcn_internal::HostCall c(who);
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B, rows = nb * (size_t)G * (size_t)n_outer;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rT = c.in(policy, sizeof(double) * nb * (size_t)n_steps * FDCN_POLICY_NCOL);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_DUAL_NSTAT);
  const int rG = c.out(gap_out, sizeof(double) * rows);
  const int rY = c.out(cont_out, sizeof(double) * rows * (size_t)n_steps);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  const int rD = c.in(div, sizeof(double) * nb * (size_t)n_steps);  // no room where null
  return c.run([&](hipStream_t stream) {
    return launch_dual(B, n_steps, G, antithetic, n_outer, n_inner, c.dev<double>(rP),
                       c.dev<int32_t>(rF), c.dev<double>(rS), c.dev<double>(rT), seed,
                       subrun_first, c.dev<double>(rO), c.dev<double>(rG), c.dev<double>(rY),
                       c.dev<double>(rW), stream, c.dev<double>(rD));
  });
}

}  // namespace

extern "C" {

int fdcn_mc_policy_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t* obs_per_sub,
                        int64_t* ws_bytes_per_contract, int64_t* values_per_contract) {
  const int rc = check_lower_sizes("mc_policy_plan", 1, n_steps, G, antithetic, 0);
  if (rc) return rc;
  if (obs_per_sub) *obs_per_sub = obs_per_subrun(antithetic);
  if (ws_bytes_per_contract) *ws_bytes_per_contract = ws_bytes(G);
  if (values_per_contract) *values_per_contract = (int64_t)G * kSubrun;
  return FDCN_OK;
}

int fdcn_mc_policy_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                             const double* params, const int32_t* flags, const double* step,
                             const double* policy, uint64_t seed, int64_t obs_first,
                             double* stats, double* values_out, double* workspace,
                             int64_t workspace_bytes, void* stream) {
  return lower_dev("mc_policy_batch_dev", false, B, n_steps, G, antithetic, params, flags, step,
                   nullptr, policy, seed, obs_first, stats, values_out, workspace,
                   workspace_bytes, stream);
}

int fdcn_mc_policy_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                         const double* params, const int32_t* flags, const double* step,
                         const double* policy, uint64_t seed, int64_t obs_first, double* stats,
                         double* values_out) {
  return lower_host("mc_policy_batch", false, B, n_steps, G, antithetic, params, flags, step,
                    nullptr, policy, seed, obs_first, stats, values_out);
}

int fdcn_mc_policy_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                 const double* params, const int32_t* flags, const double* step,
                                 const double* div, const double* policy, uint64_t seed,
                                 int64_t obs_first, double* stats, double* values_out,
                                 double* workspace, int64_t workspace_bytes, void* stream) {
  return lower_dev("mc_policy_div_batch_dev", true, B, n_steps, G, antithetic, params, flags,
                   step, div, policy, seed, obs_first, stats, values_out, workspace,
                   workspace_bytes, stream);
}

int fdcn_mc_policy_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                             const double* params, const int32_t* flags, const double* step,
                             const double* div, const double* policy, uint64_t seed,
                             int64_t obs_first, double* stats, double* values_out) {
  return lower_host("mc_policy_div_batch", true, B, n_steps, G, antithetic, params, flags, step,
                    div, policy, seed, obs_first, stats, values_out);
}

int fdcn_mc_policy_dual_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                             int32_t n_inner, int64_t* ws_bytes_per_contract,
                             int64_t* gap_per_contract, int64_t* cont_per_contract) {
  const int rc =
      check_dual_sizes("mc_policy_dual_plan", 1, n_steps, G, antithetic, n_outer, n_inner, 0);
  if (rc) return rc;
  if (ws_bytes_per_contract) *ws_bytes_per_contract = ws_bytes(G);
  if (gap_per_contract) *gap_per_contract = (int64_t)G * n_outer;
  if (cont_per_contract) *cont_per_contract = (int64_t)G * n_outer * n_steps;
  return FDCN_OK;
}

int fdcn_mc_policy_dual_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                  int32_t n_outer, int32_t n_inner, const double* params,
                                  const int32_t* flags, const double* step,
                                  const double* policy, uint64_t seed, int64_t subrun_first,
                                  double* stats, double* gap_out, double* cont_out,
                                  double* workspace, int64_t workspace_bytes, void* stream) {
  return dual_dev("mc_policy_dual_batch_dev", false, B, n_steps, G, antithetic, n_outer, n_inner,
                  params, flags, step, nullptr, policy, seed, subrun_first, stats, gap_out,
                  cont_out, workspace, workspace_bytes, stream);
}

int fdcn_mc_policy_dual_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                              int32_t n_outer, int32_t n_inner, const double* params,
                              const int32_t* flags, const double* step, const double* policy,
                              uint64_t seed, int64_t subrun_first, double* stats,
                              double* gap_out, double* cont_out) {
  return dual_host("mc_policy_dual_batch", false, B, n_steps, G, antithetic, n_outer, n_inner,
                   params, flags, step, nullptr, policy, seed, subrun_first, stats, gap_out,
                   cont_out);
}

int fdcn_mc_policy_dual_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                      int32_t n_outer, int32_t n_inner, const double* params,
                                      const int32_t* flags, const double* step,
                                      const double* div, const double* policy, uint64_t seed,
                                      int64_t subrun_first, double* stats, double* gap_out,
                                      double* cont_out, double* workspace,
                                      int64_t workspace_bytes, void* stream) {
  return dual_dev("mc_policy_dual_div_batch_dev", true, B, n_steps, G, antithetic, n_outer,
                  n_inner, params, flags, step, div, policy, seed, subrun_first, stats, gap_out,
                  cont_out, workspace, workspace_bytes, stream);
}

int fdcn_mc_policy_dual_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                  int32_t n_outer, int32_t n_inner, const double* params,
                                  const int32_t* flags, const double* step, const double* div,
                                  const double* policy, uint64_t seed, int64_t subrun_first,
                                  double* stats, double* gap_out, double* cont_out) {
  return dual_host("mc_policy_dual_div_batch", true, B, n_steps, G, antithetic, n_outer,
                   n_inner, params, flags, step, div, policy, seed, subrun_first, stats, gap_out,
                   cont_out);
}

}  // extern "C"
