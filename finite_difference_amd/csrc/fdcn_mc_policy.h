// fdcn_mc_policy.h -- the one path-step functional of the table-policy Monte
// Carlo (include/fdcn.h, fdcn_mc_policy_batch): phase C of fdcn_mc_lsm.hip with
// the fitted rule replaced by a band [X_LO_m, X_HI_m] in the log-spot.  Shared
// by the lower-bound kernel and by the inner walks of the table-policy dual
// (both in fdcn_mc_policy.hip), so the two cannot drift apart.
//
// The band is compared in x, so exp is evaluated only where something reads
// the spot: a MONITOR step of a barrier contract, an in-band decision (phi > 0
// is the last condition of the rule), maturity and a step that pays a cash
// dividend (the map g works on the spot).  Include after a
// `#pragma clang fp contract(off)`: every operation is rounded separately.
#pragma once

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "../../include/fdcn.h"
#include "fdcn_mc_div.h"

namespace fdcn_policy {

struct Contract {
  double strike, lower, upper;
  bool put, ko, ki, has_lo, has_hi, use_mon;
};

// KIND outside 0..6 reads as 0 (_dev callers: the host entries reject it)
__device__ __forceinline__ Contract load_contract(const double* P, const int32_t* F) {
  Contract c;
  c.strike = P[FDCN_LSM_P_STRIKE];
  c.lower = P[FDCN_LSM_P_LOWER];
  c.upper = P[FDCN_LSM_P_UPPER];
  c.put = F[FDCN_LSM_F_PUT] != 0;
  int kind = F[FDCN_LSM_F_KIND];
  if (kind < 0 || kind > 6) kind = 0;
  c.ko = kind >= 1 && kind <= 3;
  c.ki = kind >= 4;
  c.has_lo = kind == 1 || kind == 3 || kind == 4 || kind == 6;
  c.has_hi = kind == 2 || kind == 3 || kind == 5 || kind == 6;
  c.use_mon = kind != 0;
  return c;
}

__device__ __forceinline__ double payoff(const Contract& c, double s) {
  return c.put ? fmax(c.strike - s, 0.0) : fmax(s - c.strike, 0.0);
}

__device__ __forceinline__ bool breach(const Contract& c, double s) {
  return (c.has_lo && s <= c.lower) || (c.has_hi && s >= c.upper);
}

// distance of x to the finite ends of the band; an infinite end is infinitely
// far (x is finite), so +inf if neither is finite
__device__ __forceinline__ double band_margin(double x, double lo, double hi) {
  return fmin(fabs(x - lo), fabs(x - hi));
}

// One step of a path under the table rule: step row r, policy row pr
// (FDCN_POLICY_X_LO, FDCN_POLICY_X_HI).  `stopped` counts the stops of the rule
// itself, `walked` the steps of paths still alive.  dv is the step's cash
// dividend (uniform; 0.0 for none): paid after the move and before every event,
// on a step without a flag too, through one exp and one log (fdcn_mc_div.h).
// Callers without dividends pass the constant 0.0 and the map folds away.
__device__ __forceinline__ void path_step(const Contract& c, const double* r, const double* pr,
                                          bool last, double z, double dv, double& x, bool& done,
                                          bool& in, double& val, double& margin,
                                          uint64_t& walked, uint32_t& stopped) {
  if (done) return;
  ++walked;
  x += r[FDCN_LSM_S_DRIFT] + r[FDCN_LSM_S_DIFF] * z;
  if (dv != 0.0) x = fdcn_div::div_forward(x, dv);
  const bool mon = c.use_mon && r[FDCN_LSM_S_MONITOR] != 0.0;
  const bool ex = !last && r[FDCN_LSM_S_EXERCISE] != 0.0;
  if (!(mon || ex || last)) return;
  double lo = INFINITY, hi = -INFINITY;
  if (ex) {
    lo = pr[FDCN_POLICY_X_LO];
    hi = pr[FDCN_POLICY_X_HI];
  }
  const bool inband = lo <= x && x <= hi;
  if (!(mon || last)) {  // an EXERCISE step without an event: the spot is read in band only
    const bool elig = c.ki ? in : true;
    if (!(elig && inband)) {
      if (elig) margin = fmin(margin, band_margin(x, lo, hi));
      return;
    }
  }
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
  } else if (ex && elig) {
    margin = fmin(margin, band_margin(x, lo, hi));
    if (inband && phi > 0.0) {
      val = phi * dfe;
      done = true;
      ++stopped;
    }
  }
}

}  // namespace fdcn_policy
