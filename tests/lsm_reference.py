"""The least-squares Monte Carlo contract of include/fdcn.h (fdcn_mc_lsm_batch)
restated in mpmath at 50 digits, for one sub-run: the independent reference of
test_lsm_edges_host.py and test_gpu_lsm_edges.py.

Written from the header's text, not from the kernel or from
mc_american.host_subruns, and shaped differently on purpose:

* the whole forward walk x_0 .. x_M of every path is stored (the header's
  backward walk `x -= ...` is exact here, so it is the same number), and s,
  phi, u are functions of it;
* h is a per-path scan for the first monitored breach;
* a path's cashflow is kept as (stopping step, amount paid there); "cf
  discounted to t_m" is the amount times the product of DF_STEP over the steps
  between -- there is no running multiply;
* the fit is the solution of the exact normal equations by mpmath's lu_solve;
  the validity rule uses the pivots of the exact matrix (d_j of the Cholesky =
  the pivots of elimination without exchanges);
* the price set is walked path by path.

Only the float64 normals are shared with the engines (mc_barrier.philox_normals:
the Philox mapping and the Box-Muller are tested against the device in
test_gpu_mc.py).  The path-to-observation mapping is restated here from the
header's sentence.

Every number of a step table is taken as the float64 it is.  Sums are rounded
to 50 digits; a DIFF below 1e-60 is therefore absorbed here as it is in
float64 (lsm_edge_cases.py uses that for its equal-regressor step).
"""
import functools

import mpmath as mp
import numpy as np

from finite_difference_amd import capi
from finite_difference_amd.mc_barrier import philox_normals

DPS = 50
N_PATHS = 4096     # FDCN_LSM_SUBRUN
N_THREADS = 256    # "slot k = p / 256 of thread p % 256"
MIN_FIT = 64       # FDCN_LSM_MIN_FIT
PIVOT_TOL = "1e-12"
KNOCK_OUT, KNOCK_IN = (1, 2, 3), (4, 5, 6)
HAS_LOWER, HAS_UPPER = (1, 3, 4, 6), (2, 3, 5, 6)

CENSUS_PATH_KEYS = (
    "ko_hit_maturity_phi_gt_rebate", "ko_hit_maturity_phi_lt_rebate",
    "ko_hit_early_phi_gt_rebate", "ko_hit_early_phi_lt_rebate",
    "breach_return_rebreach", "first_breach_lower", "first_breach_upper",
    "ki_exercise_at_breach_step", "ki_never_in_rebate",
    "eligible_itm_hold", "eligible_itm_exercise", "otm_at_exercise_step",
    "price_itm_past_invalid_step_stops_later")
CENSUS_STEP_KEYS = ("steps_with_64_paths", "steps_with_63_paths", "steps_pivot_invalid")


def _at_50_digits(fn):
    @functools.wraps(fn)
    def run(*a, **kw):
        with mp.workdps(DPS):
            return fn(*a, **kw)
    return run


def observation_of_path(p, antithetic):
    """(observation within the sub-run, sign) of path p."""
    k, t = p // N_THREADS, p % N_THREADS
    if not antithetic:
        return p, 1.0
    return (k // 2) * N_THREADS + t, (1.0 if k % 2 == 0 else -1.0)


def subrun_normals(n_steps, antithetic, seed, word, first_obs):
    """float64 z [N_PATHS, n_steps] in path order; observation i of the
    sub-run is global observation first_obs + i."""
    per = N_PATHS // 2 if antithetic else N_PATHS
    z = philox_normals(per, n_steps, seed, word, first_obs)
    out = np.empty((N_PATHS, n_steps))
    for p in range(N_PATHS):
        o, sign = observation_of_path(p, antithetic)
        out[p] = sign * z[o]
    return out


class _Table:
    """The step table by the header's step number m = 1 .. M."""

    def __init__(self, c):
        S = np.asarray(c.step, dtype=float)
        self.M = S.shape[0]
        col = lambda j: [None] + [mp.mpf(float(v)) for v in S[:, j]]  # noqa: E731
        self.drift, self.diff = col(capi.LSM_S_DRIFT), col(capi.LSM_S_DIFF)
        self.df_step, self.df_end = col(capi.LSM_S_DF_STEP), col(capi.LSM_S_DF_END)
        self.rebate = col(capi.LSM_S_REBATE)
        self.centre, self.iscale = col(capi.LSM_S_CENTRE), col(capi.LSM_S_ISCALE)
        self.kind = int(c.flags[capi.LSM_F_KIND])
        self.put = bool(c.flags[capi.LSM_F_PUT])
        self.monitor = [False] + [bool(v != 0.0) and self.kind != 0
                                  for v in S[:, capi.LSM_S_MONITOR]]
        # maturity always exercises, and is never a fitted step
        self.exercise = [False] + [bool(v != 0.0) for v in S[:, capi.LSM_S_EXERCISE]]
        self.exercise[self.M] = False
        self.spot = mp.mpf(float(c.params[capi.LSM_P_SPOT]))
        self.strike = mp.mpf(float(c.params[capi.LSM_P_STRIKE]))
        self.lower = mp.mpf(float(c.params[capi.LSM_P_LOWER]))
        self.upper = mp.mpf(float(c.params[capi.LSM_P_UPPER]))
        self.ko, self.ki = self.kind in KNOCK_OUT, self.kind in KNOCK_IN

    def discount(self, a, b):
        """From t_b back to t_a (a <= b): the product of DF_STEP_{a+1 .. b}."""
        d = mp.mpf(1)
        for j in range(a + 1, b + 1):
            d *= self.df_step[j]
        return d

    def side(self, s):
        """0 inside, 1 at or beyond the lower level, 2 at or beyond the upper."""
        if self.kind in HAS_LOWER and s <= self.lower:
            return 1
        if self.kind in HAS_UPPER and s >= self.upper:
            return 2
        return 0

    def payoff(self, s):
        v = self.strike - s if self.put else s - self.strike
        return v if v > 0 else mp.mpf(0)

    def regressor(self, x, m):
        return (x - self.centre[m]) * self.iscale[m]


class _PathSet:
    """x, s, phi [N_PATHS][0 .. M], the side breached per monitored step and
    the first breach step h (M + 1: none)."""

    def __init__(self, T, z):
        M = T.M
        x0 = mp.log(T.spot)
        self.x, self.s, self.phi, self.sides, self.h = [], [], [], [], []
        for p in range(N_PATHS):
            x = [x0]
            for m in range(1, M + 1):
                x.append(x[-1] + (T.drift[m] + T.diff[m] * mp.mpf(float(z[p, m - 1]))))
            s = [mp.exp(v) for v in x]
            sides = [0] + [T.side(s[m]) if T.monitor[m] else 0 for m in range(1, M + 1)]
            self.x.append(x)
            self.s.append(s)
            self.phi.append([T.payoff(v) for v in s])
            self.sides.append(sides)
            self.h.append(next((m for m in range(1, M + 1) if sides[m]), M + 1))

    def returns_and_breaches_again(self, T, p):
        seen_return = False
        for m in range(self.h[p] + 1, T.M + 1):
            if not T.monitor[m]:
                continue
            if self.sides[p][m] == 0:
                seen_return = True
            elif seen_return:
                return True
        return False


def solve_normal_equations(us, ys):
    """The cubic least-squares fit of ys on us through the exact normal
    equations.  -> (coefficients or None where the matrix is singular, pivot
    ratios d_j / a_jj [4], a ratio after a zero pivot is None)."""
    pw = [[mp.mpf(1), u, u * u, u * u * u] for u in us]
    mom = [mp.fsum((r[min(k, 3)] * r[k - min(k, 3)] for r in pw)) for k in range(7)]
    rhs = [mp.fsum(r[i] * y for r, y in zip(pw, ys)) for i in range(4)]
    A = mp.matrix(4, 4)
    for i in range(4):
        for j in range(4):
            A[i, j] = mom[i + j]
    W = A.copy()
    ratios = [None] * 4
    for j in range(4):
        if A[j, j] == 0:
            break
        ratios[j] = W[j, j] / A[j, j]
        if W[j, j] <= 0:
            break
        for i in range(j + 1, 4):
            f = W[i, j] / W[j, j]
            for k in range(j, 4):
                W[i, k] -= f * W[j, k]
    if any(r is None or r <= 0 for r in ratios):
        return None, ratios
    c = mp.lu_solve(A, mp.matrix(rhs))
    return [c[k] for k in range(4)], ratios


def cubic(c, u):
    return c[0] + u * (c[1] + u * (c[2] + u * c[3]))


@_at_50_digits
def reference_subrun(c, subrun, antithetic, seed, stream_id, obs_first=0):
    """Sub-run `subrun` of contract c (an LsmContract) of a launch whose first
    observation is obs_first.  -> dict:

    coef [M][4] mpf (zeros without a valid fit), valid [M] bool, fitted [M] bool
    (an EXERCISE step before maturity), count [M], ratios [M][4] (float or
    None), fit_paths {m: [p]}, fit_u {m: [mpf]}, fit_gap {m: [phi - fit]} (valid
    fits), fit_cf {m: [mpf]} (the fit's right-hand side), price_decisions
    [(p, m, u, phi - fit)], values [N] mpf, stops [N] int, fit_stops [N],
    fit_mean, price_mean, invalid, min_margin, census {key: [fit set, price set]}
    (step keys: a number), z_fit / z_price (the float64 normals), x_fit / x_price
    (the walks).  Step-indexed lists have row m - 1 for step m."""
    T = _Table(c)
    M = T.M
    per = N_PATHS // 2 if antithetic else N_PATHS
    first = int(obs_first) + int(subrun) * per
    z_fit = subrun_normals(M, antithetic, seed, 2 * int(stream_id), first)
    z_price = subrun_normals(M, antithetic, seed, 2 * int(stream_id) + 1, first)
    zero = mp.mpf(0)
    cen = {k: [0, 0] for k in CENSUS_PATH_KEYS}
    cen.update({k: 0 for k in CENSUS_STEP_KEYS})

    def eligible(m, h):
        return m < h if T.ko else (m >= h if T.ki else True)

    # ---- the fit set: A (the walk) and B (backward induction)
    fs = _PathSet(T, z_fit)
    stop, amount, voluntary = [M] * N_PATHS, [zero] * N_PATHS, [False] * N_PATHS
    for p in range(N_PATHS):
        phi, h = fs.phi[p][M], fs.h[p]
        if T.ko:
            amount[p] = max(phi, T.rebate[M]) if h == M else phi
        elif T.ki:
            amount[p] = phi if h <= M else T.rebate[M]
        else:
            amount[p] = phi
    coef = [[zero] * 4 for _ in range(M)]
    valid, count, ratios = [False] * M, [0] * M, [[None] * 4 for _ in range(M)]
    fit_paths, fit_u, fit_gap, fit_cf = {}, {}, {}, {}
    margins = []
    for m in range(M - 1, 0, -1):
        if T.ko:
            for p in range(N_PATHS):
                if fs.h[p] == m:
                    stop[p], amount[p], voluntary[p] = m, max(fs.phi[p][m], T.rebate[m]), False
        if not T.exercise[m]:
            continue
        alive = [p for p in range(N_PATHS) if eligible(m, fs.h[p])]
        cen["otm_at_exercise_step"][0] += sum(1 for p in alive if fs.phi[p][m] == 0)
        part = [p for p in alive if fs.phi[p][m] > 0]
        us = [T.regressor(fs.x[p][m], m) for p in part]
        ys = [amount[p] * T.discount(m, stop[p]) for p in part]
        count[m - 1] = len(part)
        fit_paths[m], fit_u[m], fit_cf[m] = part, us, ys
        cc, rr = solve_normal_equations(us, ys) if part else (None, [None] * 4)
        ratios[m - 1] = [None if r is None else float(r) for r in rr]
        pivots_ok = cc is not None and all(r > mp.mpf(PIVOT_TOL) for r in rr)
        ok = len(part) >= MIN_FIT and pivots_ok
        valid[m - 1] = ok
        cen["steps_with_64_paths"] += len(part) == MIN_FIT
        cen["steps_with_63_paths"] += len(part) == MIN_FIT - 1
        cen["steps_pivot_invalid"] += len(part) >= MIN_FIT and not pivots_ok
        if not ok:
            continue
        coef[m - 1] = cc
        gaps = [fs.phi[p][m] - cubic(cc, u) for p, u in zip(part, us)]
        fit_gap[m] = gaps
        for p, g in zip(part, gaps):
            margins.append(abs(g))
            if g > 0:  # phi > fit(u), strictly
                stop[p], amount[p], voluntary[p] = m, fs.phi[p][m], True
                cen["eligible_itm_exercise"][0] += 1
            else:
                cen["eligible_itm_hold"][0] += 1
    fit_mean = mp.fsum(amount[p] * T.discount(0, stop[p]) for p in range(N_PATHS)) / N_PATHS
    _path_census(T, fs, stop, voluntary, cen, 0)

    # ---- the price set: C, path by path
    ps = _PathSet(T, z_price)
    values, stops, pvol = [zero] * N_PATHS, [0] * N_PATHS, [False] * N_PATHS
    decisions = []
    for p in range(N_PATHS):
        knocked_in, passed_invalid_itm = False, False
        for m in range(1, M + 1):
            phi, side = ps.phi[p][m], ps.sides[p][m]
            if T.ko and side:
                values[p], stops[p] = max(phi, T.rebate[m]) * T.df_end[m], m
                break
            if T.ki and side:
                knocked_in = True  # eligible from m on, m included
            may = knocked_in or not T.ki
            if m == M:
                values[p], stops[p] = (phi if may else T.rebate[M]) * T.df_end[M], M
                break
            if not T.exercise[m] or not may:
                continue
            if phi == 0:
                cen["otm_at_exercise_step"][1] += 1
                continue
            if not valid[m - 1]:
                passed_invalid_itm = True
                continue
            u = T.regressor(ps.x[p][m], m)
            g = phi - cubic(coef[m - 1], u)
            decisions.append((p, m, u, g))
            margins.append(abs(g))
            if g > 0:
                values[p], stops[p], pvol[p] = phi * T.df_end[m], m, True
                cen["eligible_itm_exercise"][1] += 1
                cen["price_itm_past_invalid_step_stops_later"][1] += passed_invalid_itm
                break
            cen["eligible_itm_hold"][1] += 1
    _path_census(T, ps, stops, pvol, cen, 1)
    return dict(
        coef=coef, valid=valid, fitted=[T.exercise[m] for m in range(1, M + 1)], count=count,
        ratios=ratios, fit_paths=fit_paths, fit_u=fit_u, fit_gap=fit_gap, fit_cf=fit_cf,
        price_decisions=decisions, values=values, stops=stops, fit_stops=stop,
        fit_mean=fit_mean, price_mean=mp.fsum(values) / N_PATHS,
        invalid=sum(1 for m in range(1, M) if T.exercise[m] and not valid[m - 1]),
        min_margin=min(margins) if margins else mp.inf, census=cen, z_fit=z_fit, z_price=z_price,
        x_fit=fs.x, x_price=ps.x, h_fit=fs.h, h_price=ps.h)


def _path_census(T, S, stop, voluntary, cen, which):
    """The event branches of one path set from its walks, first breaches,
    stopping steps and whether the stop was a voluntary exercise."""
    M = T.M
    for p in range(N_PATHS):
        h = S.h[p]
        if h <= M:
            if T.kind in (3, 6):
                cen["first_breach_lower" if S.sides[p][h] == 1 else "first_breach_upper"][which] += 1
            if S.returns_and_breaches_again(T, p):
                cen["breach_return_rebreach"][which] += 1
        if T.ko and h <= M and stop[p] == h and not voluntary[p]:
            when = "maturity" if h == M else "early"
            if S.phi[p][h] > T.rebate[h]:
                cen[f"ko_hit_{when}_phi_gt_rebate"][which] += 1
            elif S.phi[p][h] < T.rebate[h]:
                cen[f"ko_hit_{when}_phi_lt_rebate"][which] += 1
        if T.ki:
            if h > M:
                cen["ki_never_in_rebate"][which] += 1
            elif voluntary[p] and stop[p] == h:
                cen["ki_exercise_at_breach_step"][which] += 1
