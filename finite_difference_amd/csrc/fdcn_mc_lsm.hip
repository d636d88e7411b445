// fdcn_mc_lsm.hip -- least-squares Monte Carlo (Longstaff-Schwartz) for American
// and Bermudan options with discretely monitored barriers, for gfx950.
//
// The statistical cross-check of the early-exercise FD pricers (american.py,
// american_barrier.py, american_knockin.py); the algorithm, the event rules and
// the Philox mapping are the contract of include/fdcn.h (fdcn_mc_lsm_batch).
//
//   lsm_kernel<ANTI, DIV>
//                        one workgroup = one sub-run = kSubrun paths of one
//                        contract, kPerThread per thread, all path state in
//                        registers.  Phase A walks the fit set forward (first
//                        breach step per path), phase B walks it backward
//                        (normals regenerated from the counter) with one cubic
//                        least-squares fit per exercise step: twelve sums per
//                        thread in slot order, a fixed LDS tree, a 4 x 4
//                        Cholesky on every lane; phase C applies the fitted
//                        stopping rule to an independent path set.  One
//                        partial row per sub-run into the workspace.
//   lsm_finalize_kernel  one thread per contract adds the sub-run means in
//                        sub-run order.
//
// The coefficient rows live in LDS between phases B and C (uniform reads are
// broadcasts); coef_out is their optional dump.  The per-step table is uniform
// across the workgroup and read with scalar loads.  No floating-point atomics;
// multiply and add are rounded separately (contraction off), so the NumPy host
// engine (mc_american.py) differs only through exp / log and summation order.
//
// DIV = true (fdcn_mc_lsm_div_batch): a step may pay a cash dividend D_m, read
// from the row div[b][n_steps] with scalar loads like the step table, so the
// branch on D_m != 0 is uniform.  The spot goes through g(s) = s - D (s >= 2 D),
// s / 2 (below) after the move in phases A and C and through g's inverse before
// the backward move in phase B: no per-path state is added.  DIV = false is the
// kernel without any of it.
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
constexpr int kPerThread = 16;
constexpr int kSubrun = kThreads * kPerThread;  // paths per workgroup
constexpr int kNSum = 12;                       // moments of one fit
constexpr int kWsRow = 4;  // per sub-run: sum v, fit-set sum cf, invalid steps, min margin
static_assert(kSubrun == FDCN_LSM_SUBRUN, "fdcn.h");

using fdcn_div::div_backward;  // the dividend map on the log-spot and its inverse
using fdcn_div::div_forward;
using fdcn_philox::normal_pair;

struct LsmArgs {
  int32_t n_steps, G;
  int64_t obs_first;
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

// sh[j][0] = sum over the workgroup of sh[j][tid], j < n: the fixed tree
template <bool MIN>
__device__ __forceinline__ void tree(double (*sh)[kThreads], int n, int tid) {
  __syncthreads();
  for (int off = kThreads / 2; off > 0; off >>= 1) {
    if (tid < off)
      for (int j = 0; j < n; ++j)
        sh[j][tid] = MIN ? fmin(sh[j][tid], sh[j][tid + off]) : sh[j][tid] + sh[j][tid + off];
    __syncthreads();
  }
}

// Unpivoted Cholesky of the normal matrix a_ij = s[i + j] (i, j = 0..3), right
// side t[0..3]; false where a pivot is not positive relative to its diagonal.
__device__ __forceinline__ bool solve_cubic(const double* s, const double* t, double* c) {
  constexpr double kTol = 1e-12;
  const double d0 = s[0];
  if (!(d0 > kTol * s[0])) return false;
  const double l00 = sqrt(d0);
  const double l10 = s[1] / l00, l20 = s[2] / l00, l30 = s[3] / l00;
  const double d1 = s[2] - l10 * l10;
  if (!(d1 > kTol * s[2])) return false;
  const double l11 = sqrt(d1);
  const double l21 = (s[3] - l20 * l10) / l11, l31 = (s[4] - l30 * l10) / l11;
  const double d2 = s[4] - l20 * l20 - l21 * l21;
  if (!(d2 > kTol * s[4])) return false;
  const double l22 = sqrt(d2);
  const double l32 = (s[5] - l30 * l20 - l31 * l21) / l22;
  const double d3 = s[6] - l30 * l30 - l31 * l31 - l32 * l32;
  if (!(d3 > kTol * s[6])) return false;
  const double l33 = sqrt(d3);
  const double y0 = t[0] / l00;
  const double y1 = (t[1] - l10 * y0) / l11;
  const double y2 = (t[2] - l20 * y0 - l21 * y1) / l22;
  const double y3 = (t[3] - l30 * y0 - l31 * y1 - l32 * y2) / l33;
  c[3] = y3 / l33;
  c[2] = (y2 - l32 * c[3]) / l22;
  c[1] = (y1 - l21 * c[2] - l31 * c[3]) / l11;
  c[0] = (y0 - l10 * c[1] - l20 * c[2] - l30 * c[3]) / l00;
  return true;
}

template <bool ANTI, bool DIV>
__global__ void __launch_bounds__(kThreads)
lsm_kernel(LsmArgs a, const double* __restrict__ params, const int32_t* __restrict__ flags,
           const double* __restrict__ step, double* __restrict__ ws,
           double* __restrict__ values_out, double* __restrict__ coef_out,
           const double* __restrict__ div) {
  constexpr int kObs = ANTI ? kPerThread / 2 : kPerThread;  // observations per thread
  constexpr int kSigns = ANTI ? 2 : 1;
  const int b = blockIdx.x / a.G;  // contract
  const int g = blockIdx.x % a.G;  // sub-run
  const int tid = threadIdx.x;
  const int M = a.n_steps;
  const double* P = params + (size_t)b * FDCN_LSM_NPARAM;
  const int32_t* F = flags + (size_t)b * FDCN_LSM_NFLAG;
  const double* S = step + (size_t)b * M * FDCN_LSM_NSTEP;
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
  const uint32_t sid = (uint32_t)F[FDCN_LSM_F_STREAM];
  const uint32_t w_fit = 2u * sid, w_price = 2u * sid + 1u;
  const double x0 = log(P[FDCN_LSM_P_SPOT]);
  // observation j of this thread: obs0 + j * kThreads
  const uint64_t obs0 =
      (uint64_t)(a.obs_first + (int64_t)g * (kObs * kThreads) + tid);

  __shared__ double sh[kNSum][kThreads];
  __shared__ double coef[FDCN_LSM_MAX_STEPS][FDCN_LSM_NCOEF];
  for (int i = tid; i < M * FDCN_LSM_NCOEF; i += kThreads) (&coef[0][0])[i] = 0.0;

  double x[kPerThread];
  int h[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    x[k] = x0;
    h[k] = M + 1;
  }

  // ---- A: fit set forward ---------------------------------------------------
  for (int i = 0; i < M; i += 2) {
    const double* r0 = S + (size_t)i * FDCN_LSM_NSTEP;
    const bool two = i + 1 < M;
    const double* r1 = two ? r0 + FDCN_LSM_NSTEP : r0;
    const double dr0 = r0[FDCN_LSM_S_DRIFT], df0 = r0[FDCN_LSM_S_DIFF];
    const double dr1 = r1[FDCN_LSM_S_DRIFT], df1 = r1[FDCN_LSM_S_DIFF];
    const bool mon0 = kind != 0 && r0[FDCN_LSM_S_MONITOR] != 0.0;
    const bool mon1 = kind != 0 && r1[FDCN_LSM_S_MONITOR] != 0.0;
    const double dv0 = DIV ? D[i] : 0.0, dv1 = DIV && two ? D[i + 1] : 0.0;
#pragma unroll
    for (int j = 0; j < kObs; ++j) {
      double z0, z1;
      normal_pair(obs0 + (uint64_t)(j * kThreads), (uint32_t)(i >> 1), w_fit, a.seed, z0, z1);
#pragma unroll
      for (int sg = 0; sg < kSigns; ++sg) {
        const int k = kSigns * j + sg;
        x[k] += dr0 + df0 * (sg ? -z0 : z0);
        if (DIV && dv0 != 0.0) x[k] = div_forward(x[k], dv0);
        if (mon0 && h[k] > M && breach(c, exp(x[k]))) h[k] = i + 1;
        if (two) {
          x[k] += dr1 + df1 * (sg ? -z1 : z1);
          if (DIV && dv1 != 0.0) x[k] = div_forward(x[k], dv1);
          if (mon1 && h[k] > M && breach(c, exp(x[k]))) h[k] = i + 2;
        }
      }
    }
  }

  // ---- B: fit set backward --------------------------------------------------
  double cf[kPerThread], zk[kObs];
  double margin = INFINITY;
  int n_invalid = 0;
  __syncthreads();  // coef zeroed
  for (int m = M; m >= 1; --m) {
    const double* r = S + (size_t)(m - 1) * FDCN_LSM_NSTEP;
    const bool ex = m < M && r[FDCN_LSM_S_EXERCISE] != 0.0;
    const bool mon = kind != 0 && r[FDCN_LSM_S_MONITOR] != 0.0;
    const double reb = r[FDCN_LSM_S_REBATE];
    if (m == M || ex || (c.ko && mon)) {
      const double centre = r[FDCN_LSM_S_CENTRE], iscale = r[FDCN_LSM_S_ISCALE];
      double phi[kPerThread], u[kPerThread];
      double sm[kNSum];
      unsigned part = 0;  // slots that take part in this step's fit
#pragma unroll
      for (int q = 0; q < kNSum; ++q) sm[q] = 0.0;
#pragma unroll
      for (int k = 0; k < kPerThread; ++k) {
        phi[k] = payoff(c, exp(x[k]));
        u[k] = (x[k] - centre) * iscale;
        if (m == M) {
          if (c.ko) cf[k] = h[k] == m ? fmax(phi[k], reb) : phi[k];
          else if (c.ki) cf[k] = h[k] <= m ? phi[k] : reb;
          else cf[k] = phi[k];
        } else if (c.ko && h[k] == m) {
          cf[k] = fmax(phi[k], reb);
        }
        const bool elig = c.ko ? m < h[k] : (c.ki ? m >= h[k] : true);
        if (ex && elig && phi[k] > 0.0) {
          const double u1 = u[k], u2 = u1 * u1, u3 = u2 * u1;
          sm[0] += 1.0;
          sm[1] += u1;
          sm[2] += u2;
          sm[3] += u3;
          sm[4] += u2 * u2;
          sm[5] += u3 * u2;
          sm[6] += u3 * u3;
          sm[7] += cf[k];
          sm[8] += u1 * cf[k];
          sm[9] += u2 * cf[k];
          sm[10] += u3 * cf[k];
          sm[11] += 1.0;
          part |= 1u << k;
        }
      }
      if (ex) {  // uniform across the workgroup
#pragma unroll
        for (int q = 0; q < kNSum; ++q) sh[q][tid] = sm[q];
        tree<false>(sh, kNSum, tid);
#pragma unroll
        for (int q = 0; q < kNSum; ++q) sm[q] = sh[q][0];
        __syncthreads();  // sh is free again
        double cc[4] = {0.0, 0.0, 0.0, 0.0};
        const bool valid = sm[11] >= (double)FDCN_LSM_MIN_FIT && solve_cubic(sm, sm + 7, cc);
        if (valid) {
#pragma unroll
          for (int k = 0; k < kPerThread; ++k) {
            if (part & (1u << k)) {
              const double fit = cubic(cc, u[k]);
              margin = fmin(margin, fabs(phi[k] - fit));
              if (phi[k] > fit) cf[k] = phi[k];
            }
          }
        } else {
          ++n_invalid;
        }
        if (tid == 0) {
          double* row = coef[m - 1];
          row[0] = cc[0];
          row[1] = cc[1];
          row[2] = cc[2];
          row[3] = cc[3];
          row[4] = valid ? 1.0 : 0.0;
        }
      }
    }
    // back to t_{m-1}
    const double dr = r[FDCN_LSM_S_DRIFT], df = r[FDCN_LSM_S_DIFF];
    const double dfs = r[FDCN_LSM_S_DF_STEP];
    const int i = m - 1;
    const double dv = DIV ? D[i] : 0.0;
    const bool fresh = (i & 1) || i == M - 1;  // else z0 of the pair drawn for step i + 1
#pragma unroll
    for (int j = 0; j < kObs; ++j) {
      double z;
      if (fresh) {
        double z0, z1;
        normal_pair(obs0 + (uint64_t)(j * kThreads), (uint32_t)(i >> 1), w_fit, a.seed, z0, z1);
        z = (i & 1) ? z1 : z0;
        zk[j] = z0;
      } else {
        z = zk[j];
      }
#pragma unroll
      for (int sg = 0; sg < kSigns; ++sg) {
        const int k = kSigns * j + sg;
        if (DIV && dv != 0.0) x[k] = div_backward(x[k], dv);
        x[k] -= dr + df * (sg ? -z : z);
        cf[k] *= dfs;
      }
    }
  }
  double sum_fit = 0.0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) sum_fit += cf[k];
  __syncthreads();  // coef complete

  // ---- C: price set forward -------------------------------------------------
  double val[kPerThread];
  bool done[kPerThread], in[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    x[k] = x0;
    val[k] = 0.0;
    done[k] = false;
    in[k] = false;
  }
  for (int i = 0; i < M; i += 2) {
    const bool two = i + 1 < M;
#pragma unroll
    for (int j = 0; j < kObs; ++j) {
      double zz[2];
      normal_pair(obs0 + (uint64_t)(j * kThreads), (uint32_t)(i >> 1), w_price, a.seed, zz[0],
                  zz[1]);
#pragma unroll
      for (int sg = 0; sg < kSigns; ++sg) {
        const int k = kSigns * j + sg;
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
          if (hf == 1 && !two) break;
          const int m = i + hf + 1;
          const double* r = S + (size_t)(m - 1) * FDCN_LSM_NSTEP;
          const double* cc = coef[m - 1];
          x[k] += r[FDCN_LSM_S_DRIFT] + r[FDCN_LSM_S_DIFF] * (sg ? -zz[hf] : zz[hf]);
          if (DIV) {
            const double dv = D[m - 1];
            if (dv != 0.0) x[k] = div_forward(x[k], dv);
          }
          const bool mon = kind != 0 && r[FDCN_LSM_S_MONITOR] != 0.0;
          const bool fitted = m < M && r[FDCN_LSM_S_EXERCISE] != 0.0 && cc[4] != 0.0;
          if (!(mon || fitted || m == M) || done[k]) continue;
          const double dfe = r[FDCN_LSM_S_DF_END], reb = r[FDCN_LSM_S_REBATE];
          const double s = exp(x[k]);
          const double phi = payoff(c, s);
          const bool hit = mon && breach(c, s);
          if (c.ko && hit) {
            val[k] = fmax(phi, reb) * dfe;
            done[k] = true;
            continue;
          }
          if (c.ki && hit) in[k] = true;
          const bool elig = c.ki ? in[k] : true;
          if (m == M) {
            val[k] = (elig ? phi : reb) * dfe;
            done[k] = true;
          } else if (fitted && elig && phi > 0.0) {
            const double u = (x[k] - r[FDCN_LSM_S_CENTRE]) * r[FDCN_LSM_S_ISCALE];
            const double fit = cubic(cc, u);
            margin = fmin(margin, fabs(phi - fit));
            if (phi > fit) {
              val[k] = phi * dfe;
              done[k] = true;
            }
          }
        }
      }
    }
  }
  double sum_v = 0.0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    sum_v += val[k];
    if (values_out)
      values_out[((size_t)b * a.G + g) * kSubrun + (size_t)k * kThreads + tid] = val[k];
  }
  if (coef_out) {
    double* o = coef_out + ((size_t)b * a.G + g) * (size_t)M * FDCN_LSM_NCOEF;
    for (int i = tid; i < M * FDCN_LSM_NCOEF; i += kThreads) o[i] = (&coef[0][0])[i];
  }

  sh[0][tid] = sum_v;
  sh[1][tid] = sum_fit;
  tree<false>(sh, 2, tid);
  const double tot_v = sh[0][0], tot_fit = sh[1][0];
  __syncthreads();
  sh[0][tid] = margin;
  tree<true>(sh, 1, tid);
  if (tid == 0) {
    double* w = ws + ((size_t)b * a.G + g) * kWsRow;
    w[0] = tot_v;
    w[1] = tot_fit;  // cf was carried back to valuation by the last pass of B
    w[2] = (double)n_invalid;
    w[3] = sh[0][0];
  }
}

__global__ void __launch_bounds__(kThreads) lsm_finalize_kernel(int32_t B, int32_t G,
                                                                const double* __restrict__ ws,
                                                                double* __restrict__ stats) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* w = ws + (size_t)b * G * kWsRow;
  double s = 0.0, s2 = 0.0, f = 0.0, f2 = 0.0, inval = 0.0, margin = INFINITY;
  for (int g = 0; g < G; ++g) {
    const double mv = w[kWsRow * g] / (double)kSubrun;
    const double mf = w[kWsRow * g + 1] / (double)kSubrun;
    s += mv;
    s2 += mv * mv;
    f += mf;
    f2 += mf * mf;
    inval += w[kWsRow * g + 2];
    margin = fmin(margin, w[kWsRow * g + 3]);
  }
  const double n = (double)G;
  double* o = stats + (size_t)b * FDCN_LSM_NSTAT;
  o[FDCN_LSM_O_PRICE] = s / n;
  o[FDCN_LSM_O_STDERR] = G > 1 ? sqrt(fmax(0.0, s2 - s * s / n) / (n - 1.0) / n) : 0.0;
  o[FDCN_LSM_O_FIT_VALUE] = f / n;
  o[FDCN_LSM_O_FIT_STDERR] = G > 1 ? sqrt(fmax(0.0, f2 - f * f / n) / (n - 1.0) / n) : 0.0;
  o[FDCN_LSM_O_SUM] = s;
  o[FDCN_LSM_O_SUM2] = s2;
  o[FDCN_LSM_O_INVALID] = inval;
  o[FDCN_LSM_O_MIN_MARGIN] = margin;
}

// ---- host side -------------------------------------------------------------
int lfail(int code, const char* msg) { return fdcn_internal::set_error(code, msg); }

int obs_per_subrun(int32_t antithetic) { return antithetic ? kSubrun / 2 : kSubrun; }

int check_sizes(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, int64_t obs_first) {
  if (B < 1) return lfail(FDCN_EINVAL, "mc_lsm_batch: B must be >= 1");
  if (G < 1) return lfail(FDCN_EINVAL, "mc_lsm_batch: G must be >= 1");
  if (n_steps < 1 || n_steps > FDCN_LSM_MAX_STEPS)
    return lfail(FDCN_EINVAL, "mc_lsm_batch: n_steps must be in 1 .. FDCN_LSM_MAX_STEPS (512)");
  if (antithetic < 0 || antithetic > 1)
    return lfail(FDCN_EINVAL, "mc_lsm_batch: antithetic must be 0 or 1");
  if ((int64_t)B * (int64_t)G > 0x7fffffffLL)
    return lfail(FDCN_EINVAL, "mc_lsm_batch: B * G is beyond one launch's grid");
  if (obs_first < 0 || obs_first > ((int64_t)1 << 56) ||
      obs_first % obs_per_subrun(antithetic) != 0)
    return lfail(FDCN_EINVAL, "mc_lsm_batch: obs_first must be a non-negative multiple of the "
                              "observations per sub-run (fdcn_mc_lsm_plan)");
  return FDCN_OK;
}

int check_pointers(const char* who, const void* params, const void* flags, const void* step,
                   const void* stats) {
  char msg[96];
  const char* bad = !params ? "params" : !flags ? "flags" : !step ? "step" : !stats ? "stats"
                                                                                    : nullptr;
  if (!bad) return FDCN_OK;
  snprintf(msg, sizeof msg, "%s: %s is NULL", who, bad);
  return lfail(FDCN_EINVAL, msg);
}

int check_contracts(int32_t B, int32_t n_steps, const double* params, const int32_t* flags,
                    const double* step) {
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
    }
    if (bad) {
      snprintf(msg, sizeof msg, "mc_lsm_batch: contract %d: %s", b, bad);
      return lfail(FDCN_EINVAL, msg);
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
      snprintf(msg, sizeof msg, "mc_lsm_div_batch: contract %d: the dividend of step %d %s", b,
               m + 1, isfinite(d) ? "is negative" : "is not finite");
      return lfail(FDCN_EINVAL, msg);
    }
  return FDCN_OK;
}

int64_t ws_bytes(int32_t G) { return (int64_t)G * kWsRow * (int64_t)sizeof(double); }

int launch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic, const double* params,
           const int32_t* flags, const double* step, uint64_t seed, int64_t obs_first,
           double* stats, double* values_out, double* coef_out, double* workspace,
           hipStream_t stream, const double* div = nullptr) {
  LsmArgs a;
  a.n_steps = n_steps;
  a.G = G;
  a.obs_first = obs_first;
  a.seed = seed;
  const dim3 grid((uint32_t)((int64_t)B * G)), block(kThreads);
  // the div entries always run a DIV instance, an all-zero row included
  auto fn = div ? (antithetic ? lsm_kernel<true, true> : lsm_kernel<false, true>)
                : (antithetic ? lsm_kernel<true, false> : lsm_kernel<false, false>);
  hipLaunchKernelGGL(fn, grid, block, 0, stream, a, params, flags, step, workspace, values_out,
                     coef_out, div);
  if (hipGetLastError() != hipSuccess) return lfail(FDCN_EHIP, "mc_lsm_batch: launch failed");
  hipLaunchKernelGGL(lsm_finalize_kernel, dim3((B + kThreads - 1) / kThreads), block, 0, stream,
                     B, G, workspace, stats);
  if (hipGetLastError() != hipSuccess) return lfail(FDCN_EHIP, "mc_lsm_batch: launch failed");
  return FDCN_OK;
}

}  // namespace

extern "C" {

int fdcn_mc_lsm_plan(int32_t n_steps, int32_t G, int32_t antithetic, int32_t* obs_per_sub,
                     int64_t* ws_bytes_per_contract, int64_t* values_per_contract,
                     int64_t* coef_per_contract) {
  const int rc = check_sizes(1, n_steps, G, antithetic, 0);
  if (rc) return rc;
  if (obs_per_sub) *obs_per_sub = obs_per_subrun(antithetic);
  if (ws_bytes_per_contract) *ws_bytes_per_contract = ws_bytes(G);
  if (values_per_contract) *values_per_contract = (int64_t)G * kSubrun;
  if (coef_per_contract) *coef_per_contract = (int64_t)G * n_steps * FDCN_LSM_NCOEF;
  return FDCN_OK;
}

int fdcn_mc_lsm_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          uint64_t seed, int64_t obs_first, double* stats, double* values_out,
                          double* coef_out, double* workspace, int64_t workspace_bytes,
                          void* stream) {
  int rc = check_sizes(B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_batch_dev", params, flags, step, stats);
  if (rc) return rc;
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_lsm_batch_dev", "this launch needs (fdcn_mc_lsm_plan)", workspace, workspace_bytes,
      ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, G, antithetic, params, flags, step, seed, obs_first, stats,
                      values_out, coef_out, (double*)ws, (hipStream_t)stream);
      });
}

int fdcn_mc_lsm_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                      const double* params, const int32_t* flags, const double* step,
                      uint64_t seed, int64_t obs_first, double* stats, double* values_out,
                      double* coef_out) {
  int rc = check_sizes(B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_batch", params, flags, step, stats);
  if (rc) return rc;
  rc = check_contracts(B, n_steps, params, flags, step);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_lsm_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_LSM_NSTAT);
  const int rY = c.out(values_out, sizeof(double) * nb * (size_t)G * kSubrun);
  const int rC = c.out(coef_out, sizeof(double) * nb * (size_t)G * n_steps * FDCN_LSM_NCOEF);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, G, antithetic, c.dev<double>(rP), c.dev<int32_t>(rF),
                  c.dev<double>(rS), seed, obs_first, c.dev<double>(rO), c.dev<double>(rY),
                  c.dev<double>(rC), c.dev<double>(rW), stream);
  });
}

int fdcn_mc_lsm_div_batch_dev(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                              const double* params, const int32_t* flags, const double* step,
                              const double* div, uint64_t seed, int64_t obs_first, double* stats,
                              double* values_out, double* coef_out, double* workspace,
                              int64_t workspace_bytes, void* stream) {
  int rc = check_sizes(B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_div_batch_dev", params, flags, step, stats);
  if (rc) return rc;
  if (!div) return lfail(FDCN_EINVAL, "mc_lsm_div_batch_dev: div is NULL");
  return fdcn_call::with_workspace<fdcn_internal::HipCall>(
      "mc_lsm_div_batch_dev", "this launch needs (fdcn_mc_lsm_plan)", workspace, workspace_bytes,
      ws_bytes(G) * B, (hipStream_t)stream, [&](void* ws) {
        return launch(B, n_steps, G, antithetic, params, flags, step, seed, obs_first, stats,
                      values_out, coef_out, (double*)ws, (hipStream_t)stream, div);
      });
}

int fdcn_mc_lsm_div_batch(int32_t B, int32_t n_steps, int32_t G, int32_t antithetic,
                          const double* params, const int32_t* flags, const double* step,
                          const double* div, uint64_t seed, int64_t obs_first, double* stats,
                          double* values_out, double* coef_out) {
  int rc = check_sizes(B, n_steps, G, antithetic, obs_first);
  if (rc) return rc;
  rc = check_pointers("mc_lsm_div_batch", params, flags, step, stats);
  if (rc) return rc;
  if (!div) return lfail(FDCN_EINVAL, "mc_lsm_div_batch: div is NULL");
  rc = check_contracts(B, n_steps, params, flags, step);
  if (rc) return rc;
  rc = check_dividends(B, n_steps, div);
  if (rc) return rc;
  fdcn_internal::HostCall c("mc_lsm_div_batch");
  if ((rc = c.open())) return rc;
  const size_t nb = (size_t)B;
  const int rP = c.in(params, sizeof(double) * nb * FDCN_LSM_NPARAM);
  const int rF = c.in(flags, sizeof(int32_t) * nb * FDCN_LSM_NFLAG);
  const int rS = c.in(step, sizeof(double) * nb * (size_t)n_steps * FDCN_LSM_NSTEP);
  const int rD = c.in(div, sizeof(double) * nb * (size_t)n_steps);
  const int rO = c.out(stats, sizeof(double) * nb * FDCN_LSM_NSTAT);
  const int rY = c.out(values_out, sizeof(double) * nb * (size_t)G * kSubrun);
  const int rC = c.out(coef_out, sizeof(double) * nb * (size_t)G * n_steps * FDCN_LSM_NCOEF);
  const int rW = c.scratch((size_t)ws_bytes(G) * nb);
  return c.run([&](hipStream_t stream) {
    return launch(B, n_steps, G, antithetic, c.dev<double>(rP), c.dev<int32_t>(rF),
                  c.dev<double>(rS), seed, obs_first, c.dev<double>(rO), c.dev<double>(rY),
                  c.dev<double>(rC), c.dev<double>(rW), stream, c.dev<double>(rD));
  });
}

}  // extern "C"
