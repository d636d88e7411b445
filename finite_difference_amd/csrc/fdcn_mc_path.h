// fdcn_mc_path.h -- the path functional of the discrete-barrier Monte Carlo
// kernels (fdcn_mc.hip: Philox normals, one per step; fdcn_mc_qmc.hip: Sobol
// points through a Brownian-bridge table).  Both walk the same contract over
// the same per-step table in the reference's operation order (simulate_payoffs,
// mc_discrete_barrier_option.py:314-387); they differ only in where the
// exponent of a step comes from.
#ifndef FDCN_MC_PATH_H
#define FDCN_MC_PATH_H

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/fdcn.h"

// multiply and add rounded separately, as NumPy rounds them
#pragma clang fp contract(off)

namespace fdcn_mc_path {

struct Contract {
  double spot, strike, df_T, thr, rebate, floor;
  int kind;  // 0 none, 1 down-out, 2 up-out, 3 down-in, 4 up-in
  bool put, down, rebate_at_hit, div_first;
};

struct Path {
  double s, hit_df;
  bool untouched;  // no monitored breach so far
};

// params / flags rows of one contract (enum fdcn_mc_param / fdcn_mc_flag)
__device__ __forceinline__ Contract load_contract(const double* __restrict__ P,
                                                  const int32_t* __restrict__ F) {
  Contract c;
  c.spot = P[FDCN_MC_P_SPOT];
  c.strike = P[FDCN_MC_P_STRIKE];
  c.df_T = P[FDCN_MC_P_DF_T];
  c.thr = P[FDCN_MC_P_THRESHOLD];
  c.rebate = P[FDCN_MC_P_REBATE];
  c.floor = P[FDCN_MC_P_FLOOR];
  c.put = F[FDCN_MC_F_PUT] != 0;
  c.kind = F[FDCN_MC_F_KIND];
  if (c.kind < 0 || c.kind > 4) c.kind = 0;  // _dev callers: the host entries reject these
  c.down = c.kind == 1 || c.kind == 3;
  c.rebate_at_hit = F[FDCN_MC_F_REBATE_AT_HIT] != 0;
  c.div_first = F[FDCN_MC_F_DIV_FIRST] != 0;
  return c;
}

// what follows a step's move: dividend, monitor test, the hit's discount factor
__device__ __forceinline__ void events(Path& p, const Contract& c, const double* __restrict__ st) {
  const double div = st[2];
  if (c.div_first && div != 0.0) p.s = fmax(p.s - div, c.floor);
  if (c.kind != 0 && st[3] != 0.0) {
    const bool breached = c.down ? p.s <= c.thr : p.s >= c.thr;
    if (breached && p.untouched) {
      p.hit_df = st[4];  // the first hit's own discount factor
      p.untouched = false;
    }
  }
  if (!c.div_first && div != 0.0) p.s = fmax(p.s - div, c.floor);
}

// step row: drift, diff, cash dividend, monitor flag, df at the step's end
__device__ __forceinline__ void advance(Path& p, const Contract& c, const double* __restrict__ st,
                                        double z) {
  p.s *= exp(st[0] + st[1] * z);
  events(p, c, st);
}

// the same step with the Brownian increment dw = W[m] - W[m-1] already scaled
// (the DIFF column is not read)
__device__ __forceinline__ void advance_by(Path& p, const Contract& c,
                                           const double* __restrict__ st, double dw) {
  p.s *= exp(st[0] + dw);
  events(p, c, st);
}

__device__ __forceinline__ double payoff(const Path& p, const Contract& c) {
  const double vanilla = c.put ? fmax(c.strike - p.s, 0.0) : fmax(p.s - c.strike, 0.0);
  const double pv = c.df_T * vanilla;
  if (c.kind == 0) return pv;
  if (c.kind <= 2)  // knock-out: survivors the vanilla, the others the rebate
    return p.untouched ? pv : c.rebate * (c.rebate_at_hit ? p.hit_df : c.df_T);
  return p.untouched ? 0.0 : pv;  // knock-in
}

}  // namespace fdcn_mc_path

namespace fdcn_internal {
// the per-contract checks of the host entries (fdcn_mc.hip): flags in range,
// spot, strike and a set barrier's threshold positive.  FDCN_OK, or
// FDCN_EINVAL with "<entry>: contract <b>: <reason>" recorded.
int mc_check_contracts(const char* entry, int32_t B, const double* params, const int32_t* flags);
}  // namespace fdcn_internal

#endif  // FDCN_MC_PATH_H
