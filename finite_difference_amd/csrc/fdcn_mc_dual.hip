// fdcn_mc_dual.hip -- Andersen-Broadie dual upper bound for the least-squares
// Monte Carlo of fdcn_mc_lsm.hip, for gfx950.
//
// The policy a sub-run of the LSM has fitted (its coefficient rows) drives a
// nested simulation: outer paths walk forward, and wherever the holder may stop
// n_inner fresh paths follow the policy from there to estimate its continuation
// value.  The gap D >= 0 of every outer path, added to the LSM's lower bound, is
// an upper bound in expectation whatever the policy; the estimator, the event
// rules and the Philox mapping are the contract of include/fdcn.h
// (fdcn_mc_lsm_dual_batch).
//
//   dual_kernel<ANTI, DIV>
//                         one workgroup of 256 threads = one sub-run of one
//                         contract.  The outer path is walked by every thread
//                         alike (no thread index enters it, so its branches
//                         are uniform and the barriers inside them are safe);
//                         at a start step each thread runs n_inner / 256 inner
//                         paths one after the other (two at a time under
//                         antithetic: +z and -z of one draw) and keeps one
//                         running sum.  A wave leaves an inner walk when all
//                         its lanes have stopped.  Two barriers and one fixed
//                         tree per start step.
//   dual_finalize_kernel  one thread per contract adds the sub-run gaps in
//                         sub-run order.
//
// The step rows of the contract and the coefficient rows of the sub-run are
// uniform across the workgroup at every point of both walks (the step index is
// a loop counter), so they are read with scalar loads straight from global
// memory, as fdcn_mc_lsm.hip reads its step table: 64 steps are 4.5 KB + 2.5 KB,
// inside the scalar cache, the operands arrive in SGPRs, and LDS holds the
// reduction row only, so it never limits the occupancy.  No floating-point
// atomics; multiply and add are rounded separately (contraction off), so the
// NumPy host engine (mc_american.host_dual_subruns) differs only through exp /
// log / the normals and not through summation order.
//
// DIV = true (fdcn_mc_lsm_dual_div_batch): a step may pay a cash dividend D_m,
// read from the row div[b][n_steps] with scalar loads like the step rows (both
// walks index it by their loop counter), so the branch on D_m != 0 is uniform.
// Both walks only go forward: after the move the spot goes through g
// (fdcn_mc_div.h), then the step's events see the ex-dividend spot.  No per-path
// state is added; DIV = false is the kernel without any of it.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/fdcn.h"
#include "fdcn_philox.h"
#include "fdcn_shared.h"

#pragma clang fp contract(off)

#include "fdcn_mc_div.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWsRow = 4;  // per sub-run: sum D, min margin, inner paths, inner path-steps
// the inner observation index (fdcn.h): three fixed-width fields under the sub-run
constexpr int kObsBits = 14, kStepBits = 9, kOuterBits = 10;
static_assert((1 << kObsBits) == FDCN_DUAL_MAX_INNER, "fdcn.h");
static_assert((1 << kStepBits) == FDCN_LSM_MAX_STEPS, "fdcn.h");
static_assert((1 << kOuterBits) == FDCN_DUAL_MAX_OUTER, "fdcn.h");

using fdcn_div::div_at;
using fdcn_div::div_forward;
using fdcn_philox::normal_pair;

struct DualArgs {
  int32_t n_steps, G, n_outer, n_inner;
  int64_t subrun_first;
  uint64_t seed;
};

struct Contract {
  double strike, lower, upper;
  bool put, ko, ki, has_lo, has_hi;
};

__device__ __forceinline__ double payoff(const Contract& c, double s) {
  return c.put ? fmax(c.strike - s, 0.0) : fmax(s - c.strike, 0.0);
}

__device__ __forceinline__ bool breach(const Contract& c, double s) {
  return (c.has_lo && s <= c.lower) || (c.has_hi && s >= c.upper);
}

__device__ __forceinline__ double cubic(const double* c, double u) {
  return c[0] + u * (c[1] + u * (c[2] + u * c[3]));
}

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

// One step of an inner path: phase C of fdcn_mc_lsm.hip on step row r, fit cc,
// dividend dv of the step (uniform; 0.0 for none, and in the instances without
// dividends a constant, so the map folds away).
__device__ __forceinline__ void inner_step(const Contract& c, const double* r, const double* cc,
                                           bool last, bool use_mon, double z, double dv,
                                           double& x, bool& done, bool& in, double& val,
                                           double& margin, uint64_t& walked) {
  if (done) return;
  ++walked;
  x += r[FDCN_LSM_S_DRIFT] + r[FDCN_LSM_S_DIFF] * z;
  if (dv != 0.0) x = div_forward(x, dv);  // a step without a flag still pays
  const bool mon = use_mon && r[FDCN_LSM_S_MONITOR] != 0.0;
  const bool fitted = !last && r[FDCN_LSM_S_EXERCISE] != 0.0 && cc[4] != 0.0;
  if (!(mon || fitted || last)) return;
  const double dfe = r[FDCN_LSM_S_DF_END], reb = r[FDCN_LSM_S_REBATE];
  const double s = exp(x);
  const double phi = payoff(c, s);
  const bool hit = mon && breach(c, s);
  if (c.ko && hit) {
    val = fmax(phi, reb) * dfe;
    done = true;
    return;
  }
  if (c.ki && hit) in = true;
  const bool elig = c.ki ? in : true;
  if (last) {
    val = (elig ? phi : reb) * dfe;
    done = true;
  } else if (fitted && elig && phi > 0.0) {
    const double u = (x - r[FDCN_LSM_S_CENTRE]) * r[FDCN_LSM_S_ISCALE];
    const double fit = cubic(cc, u);
    margin = fmin(margin, fabs(phi - fit));
    if (phi > fit) {
      val = phi * dfe;
      done = true;
    }
  }
}

// 4 waves per SIMD: the antithetic instance needs 131 VGPRs without the bound,
// 128 with it, and neither spills.  The antithetic instance with dividends
// spills under that bound (the map's exp and log are live beside two paths), so
// it alone is bound to 3 waves.
template <bool ANTI, bool DIV>
__global__ void __launch_bounds__(kThreads, (ANTI && DIV) ? 3 : 4)
dual_kernel(DualArgs a, const double* __restrict__ params, const int32_t* __restrict__ flags,
            const double* __restrict__ step, const double* __restrict__ coef,
            double* __restrict__ ws, double* __restrict__ gap_out, double* __restrict__ cont_out,
            const double* __restrict__ div) {
  const int b = blockIdx.x / a.G;  // contract
  const int g = blockIdx.x % a.G;  // sub-run
  const int tid = threadIdx.x;
  const int M = a.n_steps;
  const double* P = params + (size_t)b * FDCN_LSM_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_LSM_NFLAG;
  const double* S = step + (size_t)b * M * FDCN_LSM_NSTEP;
  const double* C = coef + ((size_t)b * a.G + g) * (size_t)M * FDCN_LSM_NCOEF;
  const double* D = DIV ? div + (size_t)b * M : nullptr;  // uniform, like S
  Contract c;
  c.strike = P[FDCN_LSM_P_STRIKE];
  c.lower = P[FDCN_LSM_P_LOWER];
  c.upper = P[FDCN_LSM_P_UPPER];
  c.put = F[FDCN_LSM_F_PUT] != 0;
  int kind = F[FDCN_LSM_F_KIND];
  if (kind < 0 || kind > 6) kind = 0;  // _dev callers: the host entry rejects these
  c.ko = kind >= 1 && kind <= 3;
  c.ki = kind >= 4;
  c.has_lo = kind == 1 || kind == 3 || kind == 4 || kind == 6;
  c.has_hi = kind == 2 || kind == 3 || kind == 5 || kind == 6;
  const bool use_mon = kind != 0;
  const uint32_t sid = (uint32_t)F[FDCN_LSM_F_STREAM];
  const uint32_t w_outer = 0x80000000u + 2u * sid, w_inner = w_outer + 1u;
  const double x0 = log(P[FDCN_LSM_P_SPOT]);
  const uint64_t gs = (uint64_t)(a.subrun_first + (int64_t)g);  // absolute sub-run
  const int n_obs_t = a.n_inner / kThreads / (ANTI ? 2 : 1);     // observations per thread
  const double n_inner_d = (double)a.n_inner;

  __shared__ double sh[kThreads + 1];

  double margin = INFINITY;  // outer decisions (uniform) and this thread's inner ones
  uint64_t walked = 0;       // inner path-steps of this thread
  double sum_d = 0.0;        // uniform
  int64_t starts = 0;        // uniform

  for (int p = 0; p < a.n_outer; ++p) {
    const uint64_t obs_outer = gs * (uint64_t)a.n_outer + (uint64_t)p;
    const size_t row_out = ((size_t)b * a.G + g) * (size_t)a.n_outer + (size_t)p;
    double* cont = cont_out ? cont_out + row_out * (size_t)M : nullptr;
    double x = x0, r = 0.0, gap = -INFINITY;
    bool in = false;
    double z0 = 0.0, z1 = 0.0;
    int i = 0;
    for (; i < M; ++i) {  // step m = i + 1
      if (!(i & 1)) normal_pair(obs_outer, (uint32_t)(i >> 1), w_outer, a.seed, z0, z1);
      const double* row = S + (size_t)i * FDCN_LSM_NSTEP;
      const double* cc = C + (size_t)i * FDCN_LSM_NCOEF;
      x += row[FDCN_LSM_S_DRIFT] + row[FDCN_LSM_S_DIFF] * ((i & 1) ? z1 : z0);
      if (DIV) {  // the dividend, then the step's events on the ex-dividend spot
        const double dv = div_at(D, i);
        if (dv != 0.0) x = div_forward(x, dv);
      }
      const bool last = i + 1 == M;
      const bool mon = use_mon && row[FDCN_LSM_S_MONITOR] != 0.0;
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
                const double* ci = C + (size_t)ii * FDCN_LSM_NCOEF;
                const bool li = ii + 1 == M;
                const double dv = DIV ? div_at(D, ii) : 0.0;
                inner_step(c, ri, ci, li, use_mon, zz[hf], dv, xa, da, ia, va, margin, walked);
                if (ANTI)
                  inner_step(c, ri, ci, li, use_mon, -zz[hf], dv, xb, db, ib, vb, margin,
                             walked);
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
          bool stops = false;
          if (cc[4] != 0.0) {
            const double u = (x - row[FDCN_LSM_S_CENTRE]) * row[FDCN_LSM_S_ISCALE];
            const double fit = cubic(cc, u);
            margin = fmin(margin, fabs(phi - fit));
            stops = phi > fit;
          }
          if (stops) {
            gap = fmax(gap, 0.0 - r);
            r += Z - chat;
          } else {
            gap = fmax(gap, (Z - chat) - r);
          }
        }
      }
      if (cont && tid == 0) cont[i] = chat;
      if (forced) {
        gap = fmax(gap, 0.0 - r);
        break;
      }
    }
    // the steps after a knock-out: no inner simulation
    if (cont)
      for (int k = i + 1 + tid; k < M; k += kThreads) cont[k] = 0.0;
    if (gap_out && tid == 0) gap_out[row_out] = gap;
    sum_d += gap;
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
dual_finalize_kernel(int32_t B, int32_t G, int32_t n_outer, const double* __restrict__ ws,
                     double* __restrict__ stats) {
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
int dfail(int code, const char* msg) { return fdcn_internal::set_error(code, msg); }

int check_sizes(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                int32_t n_inner, int64_t subrun_first) {
  if (B < 1) return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: B must be >= 1");
  if (G < 1) return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: G must be >= 1");
  if (n_steps < 1 || n_steps > FDCN_LSM_MAX_STEPS)
    return dfail(FDCN_EINVAL,
                 "mc_lsm_dual_batch: n_steps must be in 1 .. FDCN_LSM_MAX_STEPS (512)");
  if (antithetic < 0 || antithetic > 1)
    return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: antithetic must be 0 or 1");
  if ((int64_t)B * (int64_t)G > 0x7fffffffLL)
    return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: B * G is beyond one launch's grid");
  if (n_outer < 1 || n_outer > FDCN_DUAL_MAX_OUTER)
    return dfail(FDCN_EINVAL,
                 "mc_lsm_dual_batch: n_outer must be in 1 .. FDCN_DUAL_MAX_OUTER (1024)");
  const int32_t unit = antithetic ? 2 * kThreads : kThreads;
  if (n_inner < unit || n_inner > FDCN_DUAL_MAX_INNER || n_inner % unit != 0)
    return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: n_inner must be a multiple of 256 (512 when "
                              "antithetic) up to FDCN_DUAL_MAX_INNER (16384)");
  if (subrun_first < 0 || subrun_first + (int64_t)G > ((int64_t)1 << 31))
    return dfail(FDCN_EINVAL, "mc_lsm_dual_batch: subrun_first must be >= 0 and subrun_first + "
                              "G at most 2^31");
  return FDCN_OK;
}

int check_pointers(const char* who, const void* params, const void* flags, const void* step,
                   const void* coef, const void* stats) {
  char msg[96];
  const char* bad = !params ? "params" : !flags ? "flags" : !step ? "step" : !coef ? "coef"
                    : !stats ? "stats" : nullptr;
  if (!bad) return FDCN_OK;
  snprintf(msg, sizeof msg, "%s: %s is NULL", who, bad);
  return dfail(FDCN_EINVAL, msg);
}

// the LSM host entry's checks of a contract, a negative rebate and the
// coefficient rows
int check_contracts(int32_t B, int32_t n_steps, int32_t G, const double* params,
                    const int32_t* flags, const double* step, const double* coef) {
  char msg[200];
  for (int32_t b = 0; b < B; ++b) {
    const int32_t* f = flags + (size_t)b * FDCN_LSM_NFLAG;
    const double* p = params + (size_t)b * FDCN_LSM_NPARAM;
    const double* s = step + (size_t)b * n_steps * FDCN_LSM_NSTEP;
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
      else if (kind != 0 && r[FDCN_LSM_S_REBATE] < 0.0)
        bad = "a step REBATE is negative (every cashflow must be >= 0)";
    }
    const double* cf = coef + (size_t)b * G * n_steps * FDCN_LSM_NCOEF;
    for (size_t q = 0; q < (size_t)G * n_steps * FDCN_LSM_NCOEF && !bad; ++q)
      if (!isfinite(cf[q])) bad = "a coefficient is not finite";
    if (bad) {
      snprintf(msg, sizeof msg, "mc_lsm_dual_batch: contract %d: %s", b, bad);
      return dfail(FDCN_EINVAL, msg);
    }
  }
  return FDCN_OK;
}

// every dividend finite and >= 0 (a dividend on the last step is legal)
int check_dividends(int32_t B, int32_t n_steps, const double* div) {
  char msg[200];
  for (int32_t b = 0; b < B; ++b)
    for (int32_t m = 0; m < n_steps; ++m) {
      const double d = div[(size_t)b * n_steps + m];
      if (isfinite(d) && d >= 0.0) continue;
      snprintf(msg, sizeof msg, "mc_lsm_dual_div_batch: contract %d: the dividend of step %d %s",
               b, m + 1, isfinite(d) ? "is negative" : "is not finite");
      return dfail(FDCN_EINVAL, msg);
    }
  return FDCN_OK;
}

int64_t ws_bytes(int32_t G) { return (int64_t)G * kWsRow * (int64_t)sizeof(double); }

int launch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
           int32_t n_inner, const double* params, const int32_t* flags, const double* step,
           const double* coef, uint64_t seed, int64_t subrun_first, double* stats,
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
  // the div entries always run a DIV instance, an all-zero row included
  auto fn = div ? (antithetic ? dual_kernel<true, true> : dual_kernel<false, true>)
                : (antithetic ? dual_kernel<true, false> : dual_kernel<false, false>);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, a, params, flags, step, coef, workspace,
                     gap_out, cont_out, div);
  if (hipGetLastError() != hipSuccess)
    return dfail(FDCN_EHIP, "mc_lsm_dual_batch: launch failed");
  hipLaunchKernelGGL(dual_finalize_kernel, dim3((B + kThreads - 1) / kThreads), block, 0, stream,
                     B, G, n_outer, workspace, stats);
  if (hipGetLastError() != hipSuccess)
    return dfail(FDCN_EHIP, "mc_lsm_dual_batch: launch failed");
  return FDCN_OK;
}

}  // namespace

extern "C" {

int fdcn_mc_lsm_dual_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t n_outer,
                          int32_t n_inner, int64_t* ws_bytes_per_contract,
                          int64_t* gap_per_contract, int64_t* cont_per_contract) {
  const int rc = check_sizes(1, n_steps, G, antithetic, n_outer, n_inner, 0);
  if (rc) return rc;
  if (ws_bytes_per_contract) *ws_bytes_per_contract = ws_bytes(G);
  if (gap_per_contract) *gap_per_contract = (int64_t)G * n_outer;
  if (cont_per_contract) *cont_per_contract = (int64_t)G * n_outer * n_steps;
  return FDCN_OK;
}

int fdcn_mc_lsm_dual_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                               int32_t n_outer, int32_t n_inner, const double* params,
                               const int32_t* flags, const double* step, const double* coef,
                               uint64_t seed, int64_t subrun_first, double* stats,
                               double* gap_out, double* cont_out, double* workspace,
                               int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_dual_batch_dev", params, flags, step, coef, stats);
  if (rc) return rc;
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_lsm_dual_batch_dev", "this launch needs (fdcn_mc_lsm_dual_plan)", workspace,
      workspace_bytes, ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, G, antithetic, n_outer, n_inner, params, flags, step, coef,
                      seed, subrun_first, stats, gap_out, cont_out, (double*)ws,
                      (hipStream_t)stream);
      });
}

int fdcn_mc_lsm_dual_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                           int32_t n_outer, int32_t n_inner, const double* params,
                           const int32_t* flags, const double* step, const double* coef,
                           uint64_t seed, int64_t subrun_first, double* stats, double* gap_out,
                           double* cont_out) {
  int rc = check_sizes(B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_dual_batch", params, flags, step, coef, stats);
  if (rc) return rc;
  rc = check_contracts(B, n_steps, G, params, flags, step, coef);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_lsm_dual_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B, rows = nb * (size_t)G * (size_t)n_outer;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rC = c.in(coef, sizeof(double) * nb * (size_t)G * n_steps * FDCN_LSM_NCOEF);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_DUAL_NSTAT);
  const int rG = c.out(gap_out, sizeof(double) * rows);
  const int rY = c.out(cont_out, sizeof(double) * rows * (size_t)n_steps);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, G, antithetic, n_outer, n_inner, c.dev<double>(rP),
                  c.dev<int32_t>(rF), c.dev<double>(rS), c.dev<double>(rC), seed, subrun_first,
                  c.dev<double>(rO), c.dev<double>(rG), c.dev<double>(rY), c.dev<double>(rW),
                  stream);
  });
}

int fdcn_mc_lsm_dual_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                                   int32_t n_outer, int32_t n_inner, const double* params,
                                   const int32_t* flags, const double* step, const double* div,
                                   const double* coef, uint64_t seed, int64_t subrun_first,
                                   double* stats, double* gap_out, double* cont_out,
                                   double* workspace, int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_dual_div_batch_dev", params, flags, step, coef, stats);
  if (rc) return rc;
  if (!div) return dfail(FDCN_EINVAL, "mc_lsm_dual_div_batch_dev: div is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_lsm_dual_div_batch_dev", "this launch needs (fdcn_mc_lsm_dual_plan)", workspace,
      workspace_bytes, ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, G, antithetic, n_outer, n_inner, params, flags, step, coef,
                      seed, subrun_first, stats, gap_out, cont_out, (double*)ws,
                      (hipStream_t)stream, div);
      });
}

int fdcn_mc_lsm_dual_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                               int32_t n_outer, int32_t n_inner, const double* params,
                               const int32_t* flags, const double* step, const double* div,
                               const double* coef, uint64_t seed, int64_t subrun_first,
                               double* stats, double* gap_out, double* cont_out) {
  int rc = check_sizes(B, n_steps, G, antithetic, n_outer, n_inner, subrun_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_dual_div_batch", params, flags, step, coef, stats);
  if (rc) return rc;
  if (!div) return dfail(FDCN_EINVAL, "mc_lsm_dual_div_batch: div is NULL");
  rc = check_contracts(B, n_steps, G, params, flags, step, coef);
  if (rc) return rc;
  rc = check_dividends(B, n_steps, div);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_lsm_dual_div_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B, rows = nb * (size_t)G * (size_t)n_outer;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rD = c.in(div, sizeof(double) * nb * (size_t)n_steps);
  const int rC = c.in(coef, sizeof(double) * nb * (size_t)G * n_steps * FDCN_LSM_NCOEF);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_DUAL_NSTAT);
  const int rG = c.out(gap_out, sizeof(double) * rows);
  const int rY = c.out(cont_out, sizeof(double) * rows * (size_t)n_steps);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, G, antithetic, n_outer, n_inner, c.dev<double>(rP),
                  c.dev<int32_t>(rF), c.dev<double>(rS), c.dev<double>(rC), seed, subrun_first,
                  c.dev<double>(rO), c.dev<double>(rG), c.dev<double>(rY), c.dev<double>(rW),
                  stream, c.dev<double>(rD));
  });
}

}  // extern "C"
