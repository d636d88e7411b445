/*
 * fdcn_oracle_ext.c -- the plan-level solvers of fdcn_oracle.c (its section 2:
 * bnd_value, thomas_const, build_matrices, plan_solve_one; Crank-Nicolson
 * with knock-outs and Ikonen-Toivanen) written once over a REAL type.
 *
 * TEST INFRASTRUCTURE ONLY, under the rule of fdcn_oracle.c's header: only
 * tests/ may load these libraries, and only as the checker.
 *
 * Every floating-point expression keeps the operand order of fdcn_oracle.c.
 * The plan arrays are fp64 by definition (include/fdcn.h); each value is
 * converted to REAL as it is read and only the arithmetic is widened.  The
 * results come back as two fp64 arrays: hi = (double)x, lo = (double)(x - hi),
 * so no extended-precision memory layout crosses the library boundary.
 *
 * Builds (oracle/Makefile), one shared library each:
 *   -DEXT_F64  -ffp-contract=off          bit-identical to oracle_*_batch
 *   -DEXT_F64  -ffp-contract=fast -mfma   the same march with fused a*b+c
 *   -DEXT_LD                              long double (>= 64-bit significand)
 *   -DEXT_QUAD                            __float128, libquadmath (optional)
 *   -DEXT_F64 -DEXT_CONVERGED -ffp-contract=fast -mfma
 *       the march kernels' reassociation of the solve (fdcn_kernels.hip, header
 *       comment and make_phase), run sequentially: A = L U + kappa e0 e0^T with
 *       the converged LU factors, every coefficient pre-divided by the root r
 *       and rounded once per phase, two first-order recurrences, and the
 *       Sherman-Morrison correction over the whole grid (no 1e-18 cut-off, no
 *       chunked scan).  In exact arithmetic it is the Thomas solve.
 *   ... -DEXT_RECOVERY in addition
 *       the same with the kernels' split / recovery form of the Crank-Nicolson
 *       right-hand side (see plan_solve_one).
 *
 * oracle_ext_vc_batch (every build): section 3 of fdcn_oracle.c, the spot-space
 * march with per-row coefficients, over REAL; its `order` argument selects the
 * Thomas march (0, bit-identical to oracle_vc_batch in the f64 build) or the
 * sequential restatement of csrc/fdcn_vc.hip's ordering (1 stencil form,
 * 2 pointwise form), see vc_solve_one.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/fdcn.h"

#if defined(EXT_QUAD)
#include <quadmath.h>
typedef __float128 REAL;
#define EXT_EXP expq
#define EXT_SQRT sqrtq
#define EXT_MANT_DIG FLT128_MANT_DIG
#elif defined(EXT_LD)
typedef long double REAL;
#define EXT_EXP expl
#define EXT_SQRT sqrtl
#define EXT_MANT_DIG LDBL_MANT_DIG
_Static_assert(LDBL_MANT_DIG >= 64, "long double must carry at least a 64-bit significand");
#elif defined(EXT_F64)
typedef double REAL;
#define EXT_EXP exp
#define EXT_SQRT sqrt
#define EXT_MANT_DIG DBL_MANT_DIG
#else
#error "define one of EXT_F64, EXT_LD, EXT_QUAD"
#endif

#define R(x) ((REAL)(x))

#ifndef EXT_CONVERGED
static void thomas_const(REAL AL, REAL AC, REAL AU, const REAL* rhs, int n, REAL* cp,
                         REAL* dp, REAL* x) {
  REAL denom = AC;
  cp[0] = AU / denom;
  dp[0] = rhs[0] / denom;
  for (int i = 1; i < n; ++i) {
    denom = AC - AL * cp[i - 1];
    if (i < n - 1) cp[i] = AU / denom;
    dp[i] = (rhs[i] - AL * dp[i - 1]) / denom;
  }
  x[n - 1] = dp[n - 1];
  for (int i = n - 2; i >= 0; --i) x[i] = dp[i] - cp[i] * x[i + 1];
}
#endif

#ifdef EXT_CONVERGED
/* make_phase() of fdcn_kernels.hip: the per-theta constants, each rounded once */
typedef struct { REAL bl, bc, bu, fm, bm, inv_r, kappa; } phase_t;

static phase_t make_phase(REAL AL, REAL AC, REAL AU, REAL BL, REAL BC, REAL BU) {
  const REAL disc = AC * AC - R(4.0) * AL * AU;
  const REAL r = R(0.5) * (AC + EXT_SQRT(disc));
  phase_t p;
  p.inv_r = R(1.0) / r;
  p.bl = BL * p.inv_r;
  p.bc = BC * p.inv_r;
  p.bu = BU * p.inv_r;
  p.fm = -AL * p.inv_r;
  p.bm = -AU * p.inv_r;
  p.kappa = AL * AU * p.inv_r;
  return p;
}

/* y = (L U)^-1 g for g already divided by r: forward then backward recurrence */
static void converged_lu(const phase_t* p, const REAL* g, int n, REAL* w, REAL* y) {
  w[0] = g[0];
  for (int i = 1; i < n; ++i) w[i] = g[i] + p->fm * w[i - 1];
  y[n - 1] = w[n - 1];
  for (int i = n - 2; i >= 0; --i) y[i] = w[i] + p->bm * y[i + 1];
}
#endif

static void build_matrices(REAL theta, REAL dt, REAL a, REAL c, REAL bcoef, REAL* AL,
                           REAL* AC, REAL* AU, REAL* BL, REAL* BC, REAL* BU) {
  *AL = -theta * dt * a;
  *AC = R(1.0) - theta * dt * bcoef;
  *AU = -theta * dt * c;
  *BL = (R(1.0) - theta) * dt * a;
  *BC = R(1.0) + (R(1.0) - theta) * dt * bcoef;
  *BU = (R(1.0) - theta) * dt * c;
}

static REAL bnd_value(int form, REAL c0, REAL e0, REAL c1, REAL e1, REAL tau) {
  if (form == 1) return c0 * EXT_EXP(e0 * tau) * c1 * EXT_EXP(e1 * tau);
  return c0 * EXT_EXP(e0 * tau) + c1 * EXT_EXP(e1 * tau);
}

static void plan_solve_one(int it_mode, int n_nodes, int n_time, int n_ranna,
                           const double* P, const int32_t* I, const double* v_init,
                           const double* payoff, const int32_t* mon_step,
                           const double* mon_rebate, double* out_hi, double* out_lo,
                           REAL* work) {
  const int n = n_nodes - 2;
  REAL* V = work;
  REAL* rhs = V + n_nodes;
  REAL* cp = rhs + n;
  REAL* dp = cp + n;
  REAL* xs = dp + n;
  REAL* lam = xs + n;
  for (int j = 0; j < n_nodes; ++j) V[j] = R(v_init[j]);
  if (it_mode)
    for (int j = 0; j < n; ++j) lam[j] = R(0.0);
  const REAL dt = R(P[FDCN_P_DT]), a = R(P[FDCN_P_A]), c = R(P[FDCN_P_C]),
             bcoef = R(P[FDCN_P_BC]);
  int mon_pos = I[FDCN_I_MON_START];
  const int mon_end = mon_pos + I[FDCN_I_MON_COUNT];
  const int ko_lo = I[FDCN_I_KO_LO], ko_hi = I[FDCN_I_KO_HI];
  REAL tau = R(P[FDCN_P_TAU0]);
#ifdef EXT_RECOVERY
  int ko_prev = 0;
#endif
  for (int m = 0; m < n_time; ++m) {
    const REAL theta = m < n_ranna ? R(1.0) : R(0.5);
    REAL AL, AC, AU, BL, BC, BU;
    build_matrices(theta, dt, a, c, bcoef, &AL, &AC, &AU, &BL, &BC, &BU);
    if (I[FDCN_I_TAU_MODE] == 1) tau = tau + dt;
    else tau = R(P[FDCN_P_TAU0]) + (REAL)(m + 1) * dt;
    const REAL lo = bnd_value(I[FDCN_I_LO_FORM], R(P[FDCN_P_LO_C0]), R(P[FDCN_P_LO_E0]),
                              R(P[FDCN_P_LO_C1]), R(P[FDCN_P_LO_E1]), tau);
    const REAL hi = bnd_value(I[FDCN_I_HI_FORM], R(P[FDCN_P_HI_C0]), R(P[FDCN_P_HI_E0]),
                              R(P[FDCN_P_HI_C1]), R(P[FDCN_P_HI_E1]), tau);
#ifdef EXT_CONVERGED
    {
      /* cp: z = (L U)^-1 e0 (rebuilt per step here; the kernel tabulates it per
       * theta), dp: the forward pass, lam + n: unused by this build */
      const phase_t p = make_phase(AL, AC, AU, BL, BC, BU);
      const REAL dts = dt * p.inv_r;
#ifdef EXT_RECOVERY
      /* B = I/theta - c2 A with c2 = (1 - theta)/theta, and A V = the previous
       * step's rhs (before the Dirichlet terms were folded in), so within a
       * phase and after a step without a knock-out the kernels' split and
       * recovery forms take rhs/r = s V - c2 (previous rhs/r), s = 1/(theta r),
       * instead of the stencil.  lam holds the previous rhs/r (CN only). */
      if (!it_mode && m > 0 && m != n_ranna && !ko_prev) {
        const REAL sc = p.inv_r / theta, c2 = (R(1.0) - theta) / theta;
        for (int j = 0; j < n; ++j) rhs[j] = sc * V[j + 1] - c2 * lam[j];
      } else
#endif
      for (int j = 1; j <= n; ++j)
        rhs[j - 1] = p.bl * V[j - 1] + p.bc * V[j] + p.bu * V[j + 1] +
                     (it_mode ? dts * lam[j - 1] : R(0.0));
#ifdef EXT_RECOVERY
      if (!it_mode) memcpy(lam, rhs, sizeof(REAL) * (size_t)n);
#endif
      rhs[0] += p.fm * lo;
      rhs[n - 1] += p.bm * hi;
      converged_lu(&p, rhs, n, dp, xs);
      for (int j = 0; j < n; ++j) rhs[j] = R(0.0);
      rhs[0] = p.inv_r;
      converged_lu(&p, rhs, n, dp, cp);
      const REAL g = p.kappa * xs[0] / (R(1.0) + p.kappa * cp[0]);
      for (int j = 0; j < n; ++j) xs[j] -= g * cp[j];
    }
#else
    if (it_mode)
      for (int j = 1; j <= n; ++j)
        rhs[j - 1] = BL * V[j - 1] + BC * V[j] + BU * V[j + 1] + dt * lam[j - 1];
    else
      for (int j = 1; j <= n; ++j) rhs[j - 1] = BL * V[j - 1] + BC * V[j] + BU * V[j + 1];
    rhs[0] -= AL * lo;
    rhs[n - 1] -= AU * hi;
    thomas_const(AL, AC, AU, rhs, n, cp, dp, xs);
#endif
    if (it_mode) {
      for (int k = 0; k < n; ++k) {
        REAL tv = xs[k], pk = R(payoff[k + 1]), lo_ = lam[k];
        REAL cand = tv - dt * lo_;
        REAL ln = lo_ + (pk - tv) / dt;
        if (ln < R(0.0)) ln = R(0.0);
        lam[k] = ln;
        xs[k] = pk > cand ? pk : cand;
      }
    }
    V[0] = lo;
    V[n_nodes - 1] = hi;
    memcpy(V + 1, xs, sizeof(REAL) * (size_t)n);
#ifdef EXT_RECOVERY
    ko_prev = 0;
#endif
    if (mon_pos < mon_end && mon_step[mon_pos] == m + 1) {
#ifdef EXT_RECOVERY
      ko_prev = 1;
#endif
      const REAL reb = R(mon_rebate[mon_pos]);
      for (int j = 0; j < n_nodes; ++j)
        if (j <= ko_lo || j >= ko_hi) V[j] = reb;
      ++mon_pos;
    }
    while (mon_pos < mon_end && mon_step[mon_pos] <= m + 1) ++mon_pos;
  }
  for (int j = 0; j < n_nodes; ++j) {
    const double h = (double)V[j];
    out_hi[j] = h;
    out_lo[j] = (double)(V[j] - R(h));
  }
}

static int plan_batch(int it_mode, int32_t B, int32_t n_nodes, int32_t n_time,
                      int32_t n_ranna, const double* params, const int32_t* iparams,
                      const double* v_init, const double* payoff, const int32_t* mon_step,
                      const double* mon_rebate, double* out_hi, double* out_lo, int nthreads) {
  if (B < 0 || n_nodes < 4 || n_time < 0) return FDCN_EINVAL;
  const size_t wlen = (size_t)n_nodes + 5 * (size_t)n_nodes;
  int err = 0;
#ifdef _OPENMP
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel num_threads(nthreads)
#endif
  {
    REAL* work = (REAL*)malloc(sizeof(REAL) * wlen);
    if (!work) {
      err = FDCN_ENOMEM;
    } else {
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
      for (int32_t bi = 0; bi < B; ++bi)
        plan_solve_one(it_mode, n_nodes, n_time, n_ranna, params + (size_t)bi * FDCN_NPARAM,
                       iparams + (size_t)bi * FDCN_NIPARAM, v_init + (size_t)bi * n_nodes,
                       it_mode ? payoff + (size_t)bi * n_nodes : NULL, mon_step, mon_rebate,
                       out_hi + (size_t)bi * n_nodes, out_lo + (size_t)bi * n_nodes, work);
      free(work);
    }
  }
  (void)nthreads;
  return err;
}

int oracle_ext_cn_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                        const double* params, const int32_t* iparams, const double* v_init,
                        int32_t n_mon, const int32_t* mon_step, const double* mon_rebate,
                        double* out_hi, double* out_lo, int32_t nthreads) {
  (void)n_mon;
  return plan_batch(0, B, n_nodes, n_time, n_ranna, params, iparams, v_init, NULL, mon_step,
                    mon_rebate, out_hi, out_lo, nthreads);
}

int oracle_ext_it_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                        const double* params, const int32_t* iparams, const double* v_init,
                        const double* payoff, double* out_hi, double* out_lo,
                        int32_t nthreads) {
  return plan_batch(1, B, n_nodes, n_time, n_ranna, params, iparams, v_init, payoff, NULL,
                    NULL, out_hi, out_lo, nthreads);
}

/* ---------------------------------------------------------------------- */
/* spot-space CN with per-row coefficients: vc_solve_one of fdcn_oracle.c  */
/* over REAL (order 0), on the plan arrays of fdcn_vc_batch.              */
/*                                                                        */
/* order 1 / 2: the ordering of csrc/fdcn_vc.hip restated sequentially,   */
/* with no scans.  Per phase the Thomas pivots beta_i are taken once and  */
/* the rows stored scaled, g = 1/beta, f = -sub g, e = -sup/beta, each    */
/* rounded once; g is folded into the explicit rows; the Dirichlet values */
/* enter as the carries g_0 lo and g_N hi of the two recurrences.         */
/*   1  stencil form:   d_i = (A V_{i-1} + B V_i + C V_{i+1}) + f_i d_{i-1} */
/*                      x_i = d_i + e_i x_{i+1},  A = a g, B = b g, C = c g */
/*   2  pointwise form: alpha from the candidate row (n/2, 1, n-2) with   */
/*      the fewest residual rows; B = g (b - alpha main); residual rows   */
/*      add g (a - alpha sub) V_{i-1} + g (c - alpha sup) V_{i+1}; the    */
/*      carries are g_0 lo - alpha V_0 and g_N hi - alpha V_N; x = alpha  */
/*      V + u.  (The kernel keeps at most two residual rows and sends the */
/*      rest to the stencil form; this restatement takes any number.)     */
/* Products written a * b + c contract under -ffp-contract=fast as the    */
/* kernels' fma() calls do.  In exact arithmetic all three are the same   */
/* solve.                                                                 */
/* ---------------------------------------------------------------------- */
static REAL vc_row_ratio(const double* P, int n, int i) {
  const REAL sub = R(P[i]), sup = R(P[2 * n + i]);
  if (sub != R(0.0)) return R(P[3 * n + i]) / sub;
  return sup != R(0.0) ? R(P[5 * n + i]) / sup : R(0.0);
}

/* per phase, scaled rows: cA, cB, cC, cf, ce of n each, then g (n); *alpha */
static void vc_factor_phase(int order, int n, const double* P, REAL* C, REAL* alpha) {
  const double *sub = P, *mn = P + n, *sup = P + 2 * n;
  const double *ae = P + 3 * n, *be = P + 4 * n, *ce = P + 5 * n;
  REAL *cA = C, *cB = C + n, *cC = C + 2 * n, *cf = C + 3 * n, *cE = C + 4 * n, *g = C + 5 * n;
  REAL al = R(0.0);
  if (order == 2) {
    const int cand[3] = {n / 2, 1, n - 2};
    int best = n + 1;
    for (int k = 0; k < 3; ++k) {
      const REAL a_k = vc_row_ratio(P, n, cand[k]);
      int cnt = 0;
      for (int i = 1; i < n - 1; ++i)
        if (R(ae[i]) - a_k * R(sub[i]) != R(0.0) || R(ce[i]) - a_k * R(sup[i]) != R(0.0)) ++cnt;
      if (cnt < best) {
        best = cnt;
        al = a_k;
      }
    }
  }
  *alpha = al;
  REAL cs = R(0.0);
  for (int i = 0; i < n; ++i) {
    const REAL beta = i == 0 ? R(mn[0]) : R(mn[i]) - R(sub[i]) * cs;
    g[i] = R(1.0) / beta;
    cs = i < n - 1 ? R(sup[i]) / beta : R(0.0);
    const int interior = i > 0 && i < n - 1;
    if (order == 2) {
      cA[i] = interior ? g[i] * (R(ae[i]) - al * R(sub[i])) : R(0.0);
      cB[i] = interior ? g[i] * (R(be[i]) - al * R(mn[i])) : R(0.0);
      cC[i] = interior ? g[i] * (R(ce[i]) - al * R(sup[i])) : R(0.0);
    } else {
      cA[i] = interior ? R(ae[i]) * g[i] : R(0.0);
      cB[i] = interior ? R(be[i]) * g[i] : R(0.0);
      cC[i] = interior ? R(ce[i]) * g[i] : R(0.0);
    }
    cf[i] = interior ? -R(sub[i]) * g[i] : R(0.0);
    cE[i] = interior ? -cs : R(0.0);
  }
}

static void vc_solve_one(int order, int n, int n_time, int n_ranna, const double* D,
                         const double* bnd, const double* v_init, const int32_t* I,
                         const int32_t* mon_step, const double* mon_rebate, double* out_hi,
                         double* out_lo, REAL* work) {
  REAL* V = work;
  REAL* rhs = V + n;
  REAL* cs = rhs + n;
  REAL* ds = cs + n;
  REAL* x = ds + n;
  REAL* fac = x + n; /* order 1 / 2: two phases of 6 n scaled rows */
  REAL alpha[2] = {R(0.0), R(0.0)};
  for (int j = 0; j < n; ++j) V[j] = R(v_init[j]);
  if (order) {
    if (n_ranna > 0) vc_factor_phase(order, n, D, fac, &alpha[0]);
    if (n_ranna < n_time)
      vc_factor_phase(order, n, D + (size_t)FDCN_VC_NDIAG * n, fac + 6 * (size_t)n, &alpha[1]);
  }
  int mon_pos = I[FDCN_I_MON_START];
  const int mon_end = mon_pos + I[FDCN_I_MON_COUNT];
  const int ko_lo = I[FDCN_I_KO_LO], ko_hi = I[FDCN_I_KO_HI];
  for (int m = 0; m < n_time; ++m) {
    const int ph = m < n_ranna ? 0 : 1;
    if (order) {
      const REAL* C = fac + (size_t)ph * 6 * n;
      const REAL *cA = C, *cB = C + n, *cC = C + 2 * n, *cf = C + 3 * n, *cE = C + 4 * n,
                 *g = C + 5 * n;
      const REAL al = alpha[ph];
      const REAL x0 = g[0] * R(bnd[2 * (size_t)m]), xN = g[n - 1] * R(bnd[2 * (size_t)m + 1]);
      if (order == 2) {
        for (int i = 1; i < n - 1; ++i) {
          rhs[i] = cB[i] * V[i];
          if (cA[i] != R(0.0) || cC[i] != R(0.0))
            rhs[i] = cA[i] * V[i - 1] + (cC[i] * V[i + 1] + rhs[i]);
        }
        ds[0] = -al * V[0] + x0;
        x[n - 1] = -al * V[n - 1] + xN;
      } else {
        for (int i = 1; i < n - 1; ++i)
          rhs[i] = cC[i] * V[i + 1] + (cB[i] * V[i] + cA[i] * V[i - 1]);
        ds[0] = x0;
        x[n - 1] = xN;
      }
      for (int i = 1; i < n - 1; ++i) ds[i] = cf[i] * ds[i - 1] + rhs[i];
      for (int i = n - 2; i >= 1; --i) x[i] = cE[i] * x[i + 1] + ds[i];
      if (order == 2)
        for (int i = 1; i < n - 1; ++i) x[i] = al * V[i] + x[i];
      x[0] = x0;
      x[n - 1] = xN;
    } else {
      const double* P = D + (size_t)ph * FDCN_VC_NDIAG * n;
      const double *sub = P, *main_ = P + n, *sup = P + 2 * n;
      const double *ae = P + 3 * n, *be = P + 4 * n, *ce = P + 5 * n;
      rhs[0] = R(bnd[2 * (size_t)m]);
      rhs[n - 1] = R(bnd[2 * (size_t)m + 1]);
      for (int i = 1; i < n - 1; ++i)
        rhs[i] = R(ae[i]) * V[i - 1] + R(be[i]) * V[i] + R(ce[i]) * V[i + 1];
      REAL beta = R(main_[0]);
      cs[0] = R(sup[0]) / beta;
      ds[0] = rhs[0] / beta;
      for (int i = 1; i < n; ++i) {
        beta = R(main_[i]) - R(sub[i]) * cs[i - 1];
        cs[i] = (i < n - 1) ? R(sup[i]) / beta : R(0.0);
        ds[i] = (rhs[i] - R(sub[i]) * ds[i - 1]) / beta;
      }
      x[n - 1] = ds[n - 1];
      for (int i = n - 2; i >= 0; --i) x[i] = ds[i] - cs[i] * x[i + 1];
    }
    memcpy(V, x, sizeof(REAL) * (size_t)n);
    if (mon_pos < mon_end && mon_step[mon_pos] == m + 1) {
      const REAL reb = R(mon_rebate[mon_pos]);
      for (int j = 0; j < n; ++j)
        if (j <= ko_lo || j >= ko_hi) V[j] = reb;
      ++mon_pos;
    }
    while (mon_pos < mon_end && mon_step[mon_pos] <= m + 1) ++mon_pos;
  }
  for (int j = 0; j < n; ++j) {
    const double h = (double)V[j];
    out_hi[j] = h;
    out_lo[j] = (double)(V[j] - R(h));
  }
}

int oracle_ext_vc_batch(int32_t B, int32_t n_nodes, int32_t n_time, int32_t n_ranna,
                        const double* diag, const double* bnd, const double* v_init,
                        const int32_t* iparams, int32_t n_mon, const int32_t* mon_step,
                        const double* mon_rebate, double* out_hi, double* out_lo,
                        int32_t order, int32_t nthreads) {
  (void)n_mon;
  if (B < 0 || n_nodes < 3 || n_time < 0 || order < 0 || order > 2) return FDCN_EINVAL;
  int err = 0;
#ifdef _OPENMP
  if (nthreads < 1) nthreads = 1;
#pragma omp parallel num_threads(nthreads)
#endif
  {
    REAL* work = (REAL*)malloc(sizeof(REAL) * 17 * (size_t)n_nodes);
    if (!work) {
      err = FDCN_ENOMEM;
    } else {
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 1)
#endif
      for (int32_t b = 0; b < B; ++b)
        vc_solve_one(order, n_nodes, n_time, n_ranna,
                     diag + (size_t)b * 2 * FDCN_VC_NDIAG * n_nodes,
                     bnd + (size_t)b * 2 * (size_t)n_time, v_init + (size_t)b * n_nodes,
                     iparams + (size_t)b * FDCN_NIPARAM, mon_step, mon_rebate,
                     out_hi + (size_t)b * n_nodes, out_lo + (size_t)b * n_nodes, work);
      free(work);
    }
  }
  (void)nthreads;
  return err;
}

/* significand bits of REAL (53, 64 on x86, 113) */
int oracle_ext_mant_dig(void) { return EXT_MANT_DIG; }
