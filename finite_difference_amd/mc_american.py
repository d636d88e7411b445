"""Least-squares Monte Carlo (Longstaff-Schwartz) for American and Bermudan
options with discretely monitored barriers: the independent statistical
cross-check of the early-exercise FD pricers (american.py,
american_barrier.py, american_knockin.py), as mc_barrier.py is of the
European barrier engines.

The events are the FD pricers' own.  A knock-out path ends at its first
monitored breach h (``s <= lower`` or ``s >= upper``) with
``max(payoff, R)`` paid there -- the exercise floor of american_barrier.py,
R = barrier.rebate_value -- and may be exercised before it.  A knock-in path
may be exercised from its hit step on, that step included, and is paid the
rebate at maturity if it never knocked in (american_knockin.py); ``rebate_at_hit``
is refused there as the FD class refuses it.  Voluntary exercise happens on
the steps flagged EXERCISE only (Bermudan); maturity always exercises.

Cash dividends are opt-in (``cash_dividends="path"``; the default "refuse"
refuses them).  A step may then pay a dividend D after its move and before its
events, through the invertible map g(s) = s - D (s >= 2 D), s / 2 (below) of
include/fdcn.h; the planner orders the events of a dividend date as the FD
classes do.

The estimator is the out-of-sample one: a sub-run of 4 096 paths fits a
cubic in the standardised log-spot per exercise date on one path set and
applies the fitted stopping rule to an independent set.  That is biased low
(a sub-optimal policy), the sign a cross-check wants; the textbook in-sample
value is biased high by more than a percent at this fit size and is reported
as a diagnostic only (``fit_value``).  A contract is G sub-runs; its price is
the mean of their means and its standard error comes from their spread.

* ``engine="hip"``: libfdcn's kernel (csrc/fdcn_mc_lsm.hip), one workgroup per
  sub-run, B contracts per launch;
* ``engine="host"``: NumPy, the same algorithm in the same operation order per
  path on the same Philox streams (include/fdcn.h), so the two agree path for
  path up to exp / log and summation order.

The lower bound has an upper one beside it (``mc_american_bounds_batch``,
``price_american_mc_bounds``): the Andersen-Broadie dual bound.  The policy a
sub-run has fitted drives a nested simulation -- outer paths, and at every
date on which the holder may stop, inner paths that follow the policy from
there -- which gives a gap >= 0 such that price + gap is an upper bound in
expectation whatever the policy (include/fdcn.h, fdcn_mc_lsm_dual_batch;
csrc/fdcn_mc_dual.hip on the device, ``host_dual_subruns`` in NumPy).
``brackets`` is the comparison of an FD price with the two bounds.  Cash
dividends are opt-in there too (``cash_dividends="path"``): both walks of the
dual pay a step's dividend after its move and before its events
(fdcn_mc_lsm_dual_div_batch); by default a contract that carries them is
refused.

Both bounds also run under a *given* exercise rule instead of the fitted one
(``mc_policy_batch``, ``mc_policy_bounds_batch``): an ``ExercisePolicy`` is a
band in the log-spot per step, and ``policy_from_pricer`` builds it from the
exercise boundary a BermudanFDMPricer has computed.  Any rule gives a lower
bound and any rule gives a dual upper bound, so the FD boundary can drive
both without circularity: a wrong boundary shows as a low lower bound and a
wide gap, not as agreement (include/fdcn.h, fdcn_mc_policy_batch;
csrc/fdcn_mc_policy.hip; ``host_policy_subruns`` in NumPy).  With
``cash_dividends="path"`` the table bounds take dividend contracts as well, and
``policy_from_pricer`` a Bermudan pricer with dividends in its life (DESIGN
section 13.5).

A missing GPU under ``engine="hip"`` is an error, never a silent fallback.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import capi
from .barrier import rebate_value
from .mc_barrier import philox4x32_10, philox_normals

__all__ = ["LsmContract", "LsmConfig", "plan_american_contract", "contract_from_pricer",
           "simulate_lsm", "price_american_mc", "mc_american_batch", "merge_lsm_stats",
           "DualConfig", "host_dual_subruns", "simulate_dual", "mc_american_bounds_batch",
           "price_american_mc_bounds", "merge_dual_stats", "brackets",
           "ExercisePolicy", "policy_from_pricer", "host_policy_subruns",
           "host_policy_dual_subruns", "simulate_policy", "simulate_policy_dual",
           "mc_policy_batch", "price_policy_mc", "mc_policy_bounds_batch",
           "price_policy_mc_bounds", "merge_policy_stats"]

_KO = ("down-and-out", "up-and-out", "double-out")
_KI = ("down-and-in", "up-and-in", "double-in")
_LOWER = ("down-and-out", "double-out", "down-and-in", "double-in")
_UPPER = ("up-and-out", "double-out", "up-and-in", "double-in")
_MERGE = 1e-12  # times closer than this are one step
_THREADS = 256
_TINY_DIFF = 1e-300  # DIFF of a zero-length step: x absorbs the move
_LN2 = 0.6931471805599453  # include/fdcn.h
_CASH_DIVIDENDS = ("refuse", "path")


@dataclass
class LsmContract:
    """One contract as the engines take it (include/fdcn.h, fdcn_mc_lsm_*)."""
    params: np.ndarray   # [LSM_NPARAM]
    flags: np.ndarray    # [LSM_NFLAG] int32 (stream id 0; set per launch)
    step: np.ndarray     # [n_steps, LSM_NSTEP]
    times: np.ndarray    # [n_steps] t_m
    barrier_type: str
    fixed_price: Optional[float] = None  # answered without a launch (contract_from_pricer)
    div: Optional[np.ndarray] = None     # [n_steps] cash dividend per step (None: none)

    @property
    def n_steps(self) -> int:
        return self.step.shape[0]

    @property
    def has_dividends(self) -> bool:
        """An all-zero `div` takes the entry without dividends."""
        return self.div is not None and bool(np.any(np.asarray(self.div) != 0.0))

    def div_row(self) -> np.ndarray:
        if self.div is None:
            return np.zeros(self.n_steps)
        d = np.asarray(self.div, dtype=float)
        if d.shape != (self.n_steps,):
            raise ValueError("LsmContract.div must be shaped [n_steps]")
        return d


@dataclass(frozen=True)
class LsmConfig:
    n_subruns: int = 32
    antithetic: bool = True
    seed: int = 42


def _step_grid(T: float, exercise: Sequence[float], monitor: Sequence[float],
               other: Sequence[float] = ()):
    """Sorted union of the exercise and monitor times in (0, T] and T itself,
    times within _MERGE of each other merged (into T at the end); the flags.
    `other` times (dividend dates) become steps without a flag."""
    marks = [(float(t), 0) for t in exercise] + [(float(t), 1) for t in monitor] + [(T, 2)]
    marks += [(float(t), 3) for t in other]
    marks = sorted((T if abs(t - T) <= _MERGE else t, w) for t, w in marks
                   if 0.0 < t <= T + _MERGE)
    times: List[float] = []
    flags: List[List[bool]] = []
    for t, w in marks:
        if not times or t - times[-1] > _MERGE:
            times.append(t)
            flags.append([False, False])
        if w < 2:
            flags[-1][w] = True
    return np.array(times), np.array(flags, dtype=bool)


def plan_american_contract(*, spot: float, strike: float, vol: float, option_type: str,
                           discount_rate: float, carry_rate: float, time_to_expiry: float,
                           barrier_type: str = "none", lower_barrier: Optional[float] = None,
                           upper_barrier: Optional[float] = None,
                           monitor_times: Sequence[float] = (), rebate_amount: float = 0.0,
                           rebate_at_hit: bool = False, n_exercise: int = 64,
                           exercise_times: Optional[Sequence[float]] = None,
                           dividends: Sequence = (),
                           cash_dividends: str = "refuse") -> LsmContract:
    """Everything the engines need for one contract: the checks, the step grid
    (the sorted union of k T / n_exercise, or `exercise_times`, and the
    monitor times in (0, T]) and the per-step table.  Rates are continuously
    compounded; times are year fractions from valuation.

    `dividends`, pairs (time, cash), are refused unless cash_dividends="path".
    Then those inside (0, T) join the step grid (the others are dropped, as the
    FD pricers drop them), same-date amounts added.  With exercise dates of the
    American kind (k T / n_exercise, n_exercise > 0) a dividend date t_d is two
    steps: the first ends at t_d with an EXERCISE flag and no MONITOR flag --
    the exercise on the cum-dividend spot --, the second has zero length
    (DRIFT 0, DIFF 1e-300, DF_STEP 1), pays the dividend and carries the
    date's MONITOR flag and a second EXERCISE flag, both on the ex-dividend
    spot.  With `exercise_times` (Bermudan) or n_exercise = 0 it is one step:
    the dividend first, then the date's own events on the ex-dividend spot; a
    date that is neither an exercise nor a monitoring date is a step without a
    flag.  CENTRE is rolled through the dividend map, ISCALE is not."""
    if _check_cash_dividends(cash_dividends) == "refuse" and len(dividends):
        raise ValueError("cash dividends are not supported by the least-squares Monte Carlo.")
    if not (spot > 0.0 and strike > 0.0):
        raise ValueError("spot and strike must be positive.")
    if not vol > 0.0:
        raise ValueError("vol must be positive.")
    T = float(time_to_expiry)
    if not T > 0.0:
        raise ValueError("time_to_expiry must be positive.")
    if option_type not in ("call", "put"):
        raise ValueError("option_type must be 'call' or 'put'.")
    bt = str(barrier_type).lower()
    if bt not in capi.LSM_KIND:
        raise ValueError(f"unknown barrier_type {barrier_type!r}")
    if bt in _KI and rebate_at_hit:
        raise ValueError("rebate_at_hit=True: a knock-in rebate is paid at maturity, if the "
                         "option never knocked in.")
    if bt in _LOWER and not (lower_barrier is not None and lower_barrier > 0.0):
        raise ValueError(f"{bt} needs a positive lower_barrier.")
    if bt in _UPPER and not (upper_barrier is not None and upper_barrier > 0.0):
        raise ValueError(f"{bt} needs a positive upper_barrier.")
    if bt in _LOWER and bt in _UPPER and not lower_barrier < upper_barrier:
        raise ValueError("lower_barrier must be below upper_barrier.")
    american = False  # a dividend date is exercised cum- and ex-dividend
    if exercise_times is None:
        n_ex = int(n_exercise)
        if n_ex < 0:
            raise ValueError("n_exercise must be >= 0.")
        exercise_times = [k * T / n_ex for k in range(1, n_ex + 1)]
        american = n_ex > 0
    cash: List[tuple] = []
    for t_d, amount in dividends:
        t_d, amount = float(t_d), float(amount)
        if not (math.isfinite(amount) and amount >= 0.0):
            raise ValueError("a cash dividend must be finite and >= 0.")
        if amount > 0.0 and 0.0 < t_d < T - _MERGE:
            cash.append((t_d, amount))
    if sum(a for _, a in cash) >= spot:
        raise ValueError("the cash dividends inside the life sum to the spot or more.")
    times, fl = _step_grid(T, exercise_times, monitor_times if bt != "none" else (),
                           [t_d for t_d, _ in cash])
    paid = np.zeros(times.shape[0])
    for t_d, amount in cash:
        paid[int(np.argmin(np.abs(times - t_d)))] += amount
    # rows (t, zero-length, exercise, monitor, dividend)
    rows: List[tuple] = []
    for m in range(times.shape[0]):
        t, ex, mon, d = float(times[m]), bool(fl[m, 0]), bool(fl[m, 1]), float(paid[m])
        if american and d > 0.0:
            rows.append((t, False, True, False, 0.0))
            rows.append((t, True, True, mon, d))
        else:
            rows.append((t, False, ex, mon, d))
    M = len(rows)
    if M > capi.LSM_MAX_STEPS:
        raise ValueError(f"{M} steps: the least-squares Monte Carlo takes at most "
                         f"{capi.LSM_MAX_STEPS}.")
    r, q = float(discount_rate), float(carry_rate)
    S = np.zeros((M, capi.LSM_NSTEP))
    div = np.zeros(M)
    base = math.log(spot)  # the centre after the last dividend
    prev, sum_drift, sum_var = 0.0, 0.0, 0.0
    for m, (t, zero, ex, mon, d) in enumerate(rows):
        if zero:
            drift, diff, df_step = 0.0, _TINY_DIFF, 1.0
        else:
            dt = t - prev
            drift = (q - 0.5 * vol * vol) * dt
            diff = vol * math.sqrt(dt)
            df_step = math.exp(-r * dt)
        sum_drift += drift
        sum_var += diff * diff
        S[m, capi.LSM_S_DRIFT] = drift
        S[m, capi.LSM_S_DIFF] = diff
        S[m, capi.LSM_S_DF_STEP] = df_step
        S[m, capi.LSM_S_DF_END] = math.exp(-r * t)
        S[m, capi.LSM_S_EXERCISE] = 1.0 if ex else 0.0
        S[m, capi.LSM_S_MONITOR] = 1.0 if mon else 0.0
        if bt != "none":
            S[m, capi.LSM_S_REBATE] = rebate_value(float(rebate_amount),
                                                   bool(rebate_at_hit) and bt in _KO, q, T - t)
        if d > 0.0:  # the centre goes through the dividend map like a path
            div[m] = d
            base = float(_div_forward(np.float64(base + sum_drift), d))
            sum_drift = 0.0
        S[m, capi.LSM_S_CENTRE] = base + sum_drift
        S[m, capi.LSM_S_ISCALE] = 1.0 / math.sqrt(sum_var)
        prev = t
    params = np.array([spot, strike, lower_barrier if bt in _LOWER else 0.0,
                       upper_barrier if bt in _UPPER else 0.0], dtype=float)
    flags = np.array([option_type == "put", capi.LSM_KIND[bt], 0], dtype=np.int32)
    return LsmContract(params=params, flags=flags, step=S,
                       times=np.array([row[0] for row in rows]), barrier_type=bt,
                       div=div if cash_dividends == "path" else None)


def contract_from_pricer(p, n_exercise: int = 64, cash_dividends: str = "refuse") -> LsmContract:
    """The contract an AmericanFDMPricer, AmericanBarrierFDMPricer or
    AmericanKnockInFDMPricer prices: its snapped spot and strike (the FD price
    is the price at those), sigma, the continuously compounded discount and
    carry rates, the barrier keywords and the monitoring times of
    `_monitor_taus`.  A pricer with a dividend in (valuation, maturity) is
    refused, unless cash_dividends="path": then the dividends of
    `_div_times_tau` go on the path (plan_american_contract).  An
    `already_hit` pricer, and a knock-in that can never knock in,
    carry the pricer's own answer in `fixed_price` and are never launched; an
    `already_in` pricer is the vanilla contract.  A BermudanFDMPricer
    (bermudan.py) gives its own exercise dates as `exercise_times`
    (`n_exercise` is ignored); one with a monitoring date inside the life that
    is not an exercise date is refused."""
    divs = p._div_times_tau()
    if _check_cash_dividends(cash_dividends) == "refuse" and divs:
        raise ValueError("cash dividends are not supported by the least-squares Monte Carlo.")
    if p.spot_snapped is None and p.strike_snapped is None:
        p._build_log_grid()
    spot = p.spot_snapped if p.snap_spot_to_grid and p.spot_snapped is not None else p.spot
    T = p.time_to_expiry
    bt = getattr(p, "barrier_type", "none")
    fixed = None
    if bt in _KO and p.already_hit:
        fixed = float(p.rebate_amount)
    elif bt in _KI and p.already_in:
        bt = "none"
    elif bt in _KI and p._skip_solve():
        fixed = float(p._never_in()["price"])
    mon: List[float] = []
    if bt != "none":
        taus, at_maturity = p._monitor_taus()
        mon = sorted(T - tau for tau in taus) + ([T] if at_maturity else [])
    exercise = None
    if hasattr(p, "_exercise_taus"):  # BermudanFDMPricer: its own exercise dates
        ex_taus = {tau for tau, _ in p._exercise_taus()}
        if bt != "none" and any(tau not in ex_taus for tau in p._monitor_taus()[0]):
            raise ValueError("a monitoring date inside the life is not an exercise date: the "
                             "least-squares Monte Carlo pays max(payoff, rebate) at every "
                             "breach, the Bermudan FD rule only on a date that is both.")
        exercise = sorted(T - tau for tau in ex_taus)
    c = plan_american_contract(
        spot=float(spot), strike=float(p._strike_for_pde()), vol=p.sigma,
        option_type=p.option_type, discount_rate=p.discount_rate_nacc,
        carry_rate=p.carry_rate_nacc, time_to_expiry=T, barrier_type=bt,
        lower_barrier=getattr(p, "lower_barrier", None) if bt in _LOWER else None,
        upper_barrier=getattr(p, "upper_barrier", None) if bt in _UPPER else None,
        monitor_times=mon, rebate_amount=getattr(p, "rebate_amount", 0.0),
        rebate_at_hit=getattr(p, "rebate_at_hit", False) and bt in _KO, n_exercise=n_exercise,
        exercise_times=exercise, dividends=[(T - tau, cash) for tau, cash in divs],
        cash_dividends=cash_dividends)
    c.fixed_price = fixed
    return c


# ---------------------------------------------------------------------------
# the host engine
# ---------------------------------------------------------------------------
def obs_per_subrun(antithetic: bool) -> int:
    return capi.LSM_SUBRUN // 2 if antithetic else capi.LSM_SUBRUN


def _path_normals(n_steps: int, seed: int, word: int, obs_first: int, antithetic: bool):
    """z [LSM_SUBRUN, n_steps] of one sub-run, in path order (include/fdcn.h:
    path p is slot k = p / 256 of thread p % 256)."""
    z = philox_normals(obs_per_subrun(antithetic), n_steps, seed, word, obs_first)
    if not antithetic:
        return z
    p = np.arange(capi.LSM_SUBRUN)
    k, tid = p // _THREADS, p % _THREADS
    return z[(k // 2) * _THREADS + tid] * np.where(k % 2 == 1, -1.0, 1.0)[:, None]


def _check_cash_dividends(mode) -> str:
    if mode not in _CASH_DIVIDENDS:
        raise ValueError(f"cash_dividends must be 'refuse' or 'path', not {mode!r}")
    return mode


def _div_forward(x: np.ndarray, d: float) -> np.ndarray:
    """The dividend map g on the log-spot (include/fdcn.h), the kernel's
    operations."""
    s = np.exp(x)
    with np.errstate(all="ignore"):
        return np.where(s >= 2.0 * d, np.log(s - d), x - _LN2)


def _div_backward(x: np.ndarray, d: float) -> np.ndarray:
    """g's inverse on the log-spot."""
    s = np.exp(x)
    return np.where(s >= d, np.log(s + d), x + _LN2)


def _cholesky_cubic(sm: np.ndarray):
    """The kernel's unpivoted 4 x 4 Cholesky on the rows of sm [g, 12], in its
    operation order -> (c [g, 4], valid [g])."""
    s = [sm[:, k] for k in range(7)]
    t = [sm[:, 7 + k] for k in range(4)]
    tol = 1e-12
    with np.errstate(all="ignore"):
        ok = sm[:, 11] >= float(capi.LSM_MIN_FIT)
        d0 = s[0]
        ok = ok & (d0 > tol * s[0])
        l00 = np.sqrt(d0)
        l10, l20, l30 = s[1] / l00, s[2] / l00, s[3] / l00
        d1 = s[2] - l10 * l10
        ok = ok & (d1 > tol * s[2])
        l11 = np.sqrt(d1)
        l21, l31 = (s[3] - l20 * l10) / l11, (s[4] - l30 * l10) / l11
        d2 = s[4] - l20 * l20 - l21 * l21
        ok = ok & (d2 > tol * s[4])
        l22 = np.sqrt(d2)
        l32 = (s[5] - l30 * l20 - l31 * l21) / l22
        d3 = s[6] - l30 * l30 - l31 * l31 - l32 * l32
        ok = ok & (d3 > tol * s[6])
        l33 = np.sqrt(d3)
        y0 = t[0] / l00
        y1 = (t[1] - l10 * y0) / l11
        y2 = (t[2] - l20 * y0 - l21 * y1) / l22
        y3 = (t[3] - l30 * y0 - l31 * y1 - l32 * y2) / l33
        c3 = y3 / l33
        c2 = (y2 - l32 * c3) / l22
        c1 = (y1 - l21 * c2 - l31 * c3) / l11
        c0 = (y0 - l10 * c1 - l20 * c2 - l30 * c3) / l00
    c = np.stack([c0, c1, c2, c3], axis=1)
    c[~ok] = 0.0
    return c, ok


def _cubic(c: np.ndarray, u: np.ndarray) -> np.ndarray:
    c0, c1, c2, c3 = (c[:, k][:, None] for k in range(4))
    return c0 + u * (c1 + u * (c2 + u * c3))


def host_subruns(c: LsmContract, subruns: Sequence[int], antithetic: bool, seed: int,
                 stream_id: int, *, want_fit: bool = False) -> dict:
    """The sub-runs `subruns` of contract c on the host: the kernel's three
    phases on arrays [g, LSM_SUBRUN].  -> values [g, LSM_SUBRUN] (price set),
    fit_mean [g], coef [g, n_steps, LSM_NCOEF], invalid [g], margin [g]; with
    want_fit also fit_u [g, n_steps, LSM_SUBRUN], the regressor of the paths of
    each fit (NaN elsewhere)."""
    P, F, S = c.params, c.flags, c.step
    M, ng, n = c.n_steps, len(subruns), capi.LSM_SUBRUN
    strike, lower, upper = float(P[capi.LSM_P_STRIKE]), float(P[capi.LSM_P_LOWER]), \
        float(P[capi.LSM_P_UPPER])
    put, kind = bool(F[capi.LSM_F_PUT]), int(F[capi.LSM_F_KIND])
    ko, ki = 1 <= kind <= 3, kind >= 4
    has_lo, has_hi = kind in (1, 3, 4, 6), kind in (2, 3, 5, 6)
    x0 = float(np.log(P[capi.LSM_P_SPOT]))
    per = obs_per_subrun(antithetic)

    def payoff(s):
        return np.maximum(strike - s, 0.0) if put else np.maximum(s - strike, 0.0)

    def breach(s):
        out = np.zeros(s.shape, dtype=bool)
        if has_lo:
            out |= s <= lower
        if has_hi:
            out |= s >= upper
        return out

    def normals(word):
        return np.stack([_path_normals(M, seed, word, int(g) * per, antithetic) for g in subruns])

    drift, diff = S[:, capi.LSM_S_DRIFT], S[:, capi.LSM_S_DIFF]
    mon = (S[:, capi.LSM_S_MONITOR] != 0.0) & (kind != 0)
    exr = S[:, capi.LSM_S_EXERCISE] != 0.0
    exr[M - 1] = False  # maturity is not a fitted step
    reb, dfs, dfe = S[:, capi.LSM_S_REBATE], S[:, capi.LSM_S_DF_STEP], S[:, capi.LSM_S_DF_END]
    centre, iscale = S[:, capi.LSM_S_CENTRE], S[:, capi.LSM_S_ISCALE]
    D = c.div_row()  # after the move, before the step's events; undone first going back

    # ---- A: fit set forward
    Z = normals(2 * int(stream_id))
    x = np.full((ng, n), x0)
    h = np.full((ng, n), M + 1, dtype=np.int64)
    for m in range(1, M + 1):
        i = m - 1
        x = x + (drift[i] + diff[i] * Z[:, :, i])
        if D[i] != 0.0:
            x = _div_forward(x, D[i])
        if mon[i]:
            h = np.where(breach(np.exp(x)) & (h > M), m, h)

    # ---- B: fit set backward
    coef = np.zeros((ng, M, capi.LSM_NCOEF))
    invalid = np.zeros(ng, dtype=np.int64)
    margin = np.full(ng, np.inf)
    fit_u = np.full((ng, M, n), np.nan) if want_fit else None
    cf = np.zeros((ng, n))
    for m in range(M, 0, -1):
        i = m - 1
        if m == M or exr[i] or (ko and mon[i]):
            phi = payoff(np.exp(x))
            u = (x - centre[i]) * iscale[i]
            if m == M:
                if ko:
                    cf = np.where(h == m, np.maximum(phi, reb[i]), phi)
                elif ki:
                    cf = np.where(h <= m, phi, reb[i])
                else:
                    cf = phi.copy()
            elif ko:
                cf = np.where(h == m, np.maximum(phi, reb[i]), cf)
            if exr[i]:
                elig = (m < h) if ko else ((m >= h) if ki else np.ones((ng, n), dtype=bool))
                part = elig & (phi > 0.0)
                u2 = u * u
                u3 = u2 * u
                terms = [np.ones_like(u), u, u2, u3, u2 * u2, u3 * u2, u3 * u3, cf, u * cf,
                         u2 * cf, u3 * cf, np.ones_like(u)]
                sm = np.stack([np.sum(np.where(part, t, 0.0), axis=1) for t in terms], axis=1)
                cc, valid = _cholesky_cubic(sm)
                fit = _cubic(cc, u)
                take = part & valid[:, None]
                if take.any():
                    gap = np.where(take, np.abs(phi - fit), np.inf)
                    margin = np.minimum(margin, gap.min(axis=1))
                cf = np.where(take & (phi > fit), phi, cf)
                invalid += ~valid
                coef[:, i, :4] = cc
                coef[:, i, 4] = valid
                if want_fit:
                    fit_u[:, i, :] = np.where(take, u, np.nan)
        if D[i] != 0.0:
            x = _div_backward(x, D[i])
        x = x - (drift[i] + diff[i] * Z[:, :, i])
        cf = cf * dfs[i]
    fit_mean = np.sum(cf, axis=1) / float(n)

    # ---- C: price set forward
    Z = normals(2 * int(stream_id) + 1)
    x = np.full((ng, n), x0)
    val = np.zeros((ng, n))
    done = np.zeros((ng, n), dtype=bool)
    inn = np.zeros((ng, n), dtype=bool)
    for m in range(1, M + 1):
        i = m - 1
        x = x + (drift[i] + diff[i] * Z[:, :, i])
        if D[i] != 0.0:
            x = _div_forward(x, D[i])
        fitted = (coef[:, i, 4] != 0.0)[:, None] & bool(exr[i])
        if not (mon[i] or m == M or fitted.any()):
            continue
        s = np.exp(x)
        phi = payoff(s)
        hit = breach(s) if mon[i] else np.zeros((ng, n), dtype=bool)
        if ko:
            k = hit & ~done
            val = np.where(k, np.maximum(phi, reb[i]) * dfe[i], val)
            done |= k
        if ki:
            inn |= hit
        elig = inn if ki else np.ones((ng, n), dtype=bool)
        if m == M:
            val = np.where(~done, np.where(elig, phi, reb[i]) * dfe[i], val)
            done[:] = True
        else:
            cand = ~done & fitted & elig & (phi > 0.0)
            if cand.any():
                u = (x - centre[i]) * iscale[i]
                fit = _cubic(coef[:, i, :4], u)
                gap = np.where(cand, np.abs(phi - fit), np.inf)
                margin = np.minimum(margin, gap.min(axis=1))
                go = cand & (phi > fit)
                val = np.where(go, phi * dfe[i], val)
                done |= go
    out = dict(values=val, fit_mean=fit_mean, coef=coef, invalid=invalid, margin=margin)
    if want_fit:
        out["fit_u"] = fit_u
    return out


def _finalize(means: np.ndarray, fit_means: np.ndarray, invalid: float, margin: float):
    """One row of stats [LSM_NSTAT] from the sub-run means, the finalize
    kernel's formulas."""
    G = means.shape[0]
    n = float(G)
    s, s2 = float(np.sum(means)), float(np.sum(means * means))
    f, f2 = float(np.sum(fit_means)), float(np.sum(fit_means * fit_means))

    def se(a, a2):
        return math.sqrt(max(0.0, a2 - a * a / n) / (n - 1.0) / n) if G > 1 else 0.0
    return np.array([s / n, se(s, s2), f / n, se(f, f2), s, s2, float(invalid), float(margin)])


def merge_lsm_stats(parts) -> Dict[str, float]:
    """Price and standard error of the union of disjoint sub-run ranges of one
    contract, from their (G, sum, sum of squares) of the sub-run means --
    tuples, or the result dicts of mc_american_batch.  Ranks that shard a
    contract's sub-runs (subrun_range) gather these three numbers, as
    merge_mc_stats does for observations."""
    G, s, s2 = 0, 0.0, 0.0
    for part in parts:
        if isinstance(part, dict):
            part = (part["n_subruns"], part["sum_mean"], part["sum_mean2"])
        G += int(part[0])
        s += float(part[1])
        s2 += float(part[2])
    if G <= 0:
        raise ValueError("merge_lsm_stats: no sub-runs")
    n = float(G)
    stderr = math.sqrt(max(0.0, s2 - s * s / n) / (n - 1.0) / n) if G > 1 else 0.0
    return {"price": s / n, "stderr": stderr, "n_subruns": G, "sum_mean": s, "sum_mean2": s2}


def _stack(group: Sequence[LsmContract], stream_ids: Sequence[int]):
    P = np.stack([c.params for c in group])
    F = np.stack([c.flags for c in group]).astype(np.int32)
    F[:, capi.LSM_F_STREAM] = np.asarray(stream_ids, dtype=np.int32)
    S = np.stack([c.step for c in group])
    return P, F, S


def simulate_lsm(group: Sequence[LsmContract], n_subruns: int, antithetic: bool, *,
                 engine: str = "hip", seed: int = 0, stream_ids: Optional[Sequence[int]] = None,
                 subrun_first: int = 0, want_values: bool = False, want_coef: bool = False,
                 host_chunk: int = 16) -> dict:
    """Run sub-runs subrun_first .. subrun_first + n_subruns - 1 of contracts
    that share n_steps.  -> {"stats": [B, LSM_NSTAT]} plus "values"
    [B, n_subruns * LSM_SUBRUN] and "coef" [B, n_subruns, n_steps, LSM_NCOEF]
    where asked for.  The Philox stream id of a contract is its index in
    `group`, or stream_ids[index]."""
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    B = len(group)
    if B < 1:
        raise ValueError("simulate_lsm: no contracts")
    n_steps = group[0].n_steps
    if any(c.n_steps != n_steps for c in group):
        raise ValueError("simulate_lsm: the contracts of a launch share n_steps")
    if n_steps > capi.LSM_MAX_STEPS:
        raise ValueError(f"simulate_lsm: at most {capi.LSM_MAX_STEPS} steps")
    G = int(n_subruns)
    if G < 1:
        raise ValueError("simulate_lsm: n_subruns must be >= 1")
    first = int(subrun_first)
    if first != subrun_first or first < 0:
        raise ValueError("simulate_lsm: subrun_first must be a whole, non-negative number of "
                         "sub-runs (a shard starts on a sub-run)")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError("simulate_lsm: one stream id per contract")
    if any(not 0 <= s < 2 ** 30 for s in ids):
        raise ValueError("simulate_lsm: stream ids must be in 0 .. 2^30 - 1")
    antithetic = bool(antithetic)
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)
        # one contract with a dividend sends the launch through the div entry
        div = (np.stack([c.div_row() for c in group]) if any(c.has_dividends for c in group)
               else None)
        stats, val, coef = capi.mc_lsm_batch(P, F, S, G, antithetic, seed=seed,
                                             obs_first=first * obs_per_subrun(antithetic),
                                             want_values=want_values, want_coef=want_coef,
                                             div=div)
        out = {"stats": stats}
        if want_values:
            out["values"] = val
        if want_coef:
            out["coef"] = coef
        return out
    stats = np.empty((B, capi.LSM_NSTAT))
    val = np.empty((B, G * capi.LSM_SUBRUN)) if want_values else None
    coef = np.empty((B, G, n_steps, capi.LSM_NCOEF)) if want_coef else None
    for b, c in enumerate(group):
        means, fits = np.empty(G), np.empty(G)
        invalid, margin = 0, math.inf
        for lo in range(0, G, max(1, int(host_chunk))):
            hi = min(G, lo + max(1, int(host_chunk)))
            r = host_subruns(c, range(first + lo, first + hi), antithetic, seed, ids[b])
            means[lo:hi] = np.sum(r["values"], axis=1) / float(capi.LSM_SUBRUN)
            fits[lo:hi] = r["fit_mean"]
            invalid += int(r["invalid"].sum())
            margin = min(margin, float(r["margin"].min()))
            if want_values:
                val[b, lo * capi.LSM_SUBRUN:hi * capi.LSM_SUBRUN] = r["values"].reshape(-1)
            if want_coef:
                coef[b, lo:hi] = r["coef"]
        stats[b] = _finalize(means, fits, invalid, margin)
    out = {"stats": stats}
    if want_values:
        out["values"] = val
    if want_coef:
        out["coef"] = coef
    return out


def _result(c: LsmContract, cfg: LsmConfig, G: int, st: Optional[np.ndarray]) -> dict:
    if st is None:  # answered by the pricer's own rule, nothing simulated
        price = float(c.fixed_price)
        st = np.array([price, 0.0, price, 0.0, price * G, price * price * G, 0.0, math.inf])
        n_paths = 0
    else:
        n_paths = G * capi.LSM_SUBRUN
    price, stderr = float(st[capi.LSM_O_PRICE]), float(st[capi.LSM_O_STDERR])
    return {
        "price": price,
        "stderr": stderr,
        "ci_95": (price - 1.96 * stderr, price + 1.96 * stderr),
        "fit_value": float(st[capi.LSM_O_FIT_VALUE]),
        "fit_stderr": float(st[capi.LSM_O_FIT_STDERR]),
        "n_paths": int(n_paths),
        "n_subruns": int(G),
        "steps": int(c.n_steps),
        "invalid_fit_steps": int(st[capi.LSM_O_INVALID]),
        "min_margin": float(st[capi.LSM_O_MIN_MARGIN]),
        "barrier_type": c.barrier_type,
        "sum_mean": float(st[capi.LSM_O_SUM]),
        "sum_mean2": float(st[capi.LSM_O_SUM2]),
    }


def mc_american_batch(contracts: Sequence, cfg: LsmConfig = LsmConfig(), *, engine: str = "hip",
                      stream_ids: Optional[Sequence[int]] = None,
                      subrun_range: Optional[range] = None,
                      cash_dividends: str = "refuse") -> List[dict]:
    """Price many contracts, one launch per distinct (step count, has
    dividends).  `contracts`: LsmContract objects, or the keyword arguments of
    plan_american_contract per contract (planned with `cash_dividends` unless
    they name their own; an LsmContract that carries dividends was planned with
    "path" and is priced as it is); cfg is shared.  The Philox stream id of a
    contract is its index in `contracts`, or stream_ids[index].  `subrun_range` (a contiguous range
    within [0, cfg.n_subruns)) runs that part of every contract's sub-runs only
    -- a rank's shard -- and merge_lsm_stats combines the parts.  Results, in
    input order: price_american_mc's dict plus "sum_mean" and "sum_mean2"."""
    _check_cash_dividends(cash_dividends)
    plans = [c if isinstance(c, LsmContract)
             else plan_american_contract(**{"cash_dividends": cash_dividends, **c})
             for c in contracts]
    lo, hi = 0, int(cfg.n_subruns)
    if hi < 1:
        raise ValueError("cfg.n_subruns must be positive.")
    if subrun_range is not None:
        lo, hi = subrun_range.start, subrun_range.stop
        if subrun_range.step != 1 or not 0 <= lo < hi <= cfg.n_subruns:
            raise ValueError("subrun_range must be a non-empty contiguous range within the "
                             "contract's sub-runs")
    ids = list(range(len(plans))) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != len(plans):
        raise ValueError("one stream id per contract")
    out: List[Optional[dict]] = [None] * len(plans)
    by_steps: Dict[tuple, List[int]] = {}
    for k, c in enumerate(plans):
        if c.fixed_price is not None:
            out[k] = _result(c, cfg, hi - lo, None)
        else:
            by_steps.setdefault((c.n_steps, c.has_dividends), []).append(k)
    for members in by_steps.values():
        r = simulate_lsm([plans[k] for k in members], hi - lo, cfg.antithetic, engine=engine,
                         seed=cfg.seed, stream_ids=[ids[k] for k in members], subrun_first=lo)
        for row, k in enumerate(members):
            out[k] = _result(plans[k], cfg, hi - lo, r["stats"][row])
    return out  # type: ignore[return-value]


def price_american_mc(contract: Optional[LsmContract] = None, *, n_subruns: int = 32,
                      antithetic: bool = True, seed: int = 42, stream_id: int = 0,
                      engine: str = "hip", cash_dividends: str = "refuse",
                      **plan_kw) -> Dict[str, object]:
    """Least-squares Monte Carlo price of one contract -- an LsmContract
    (contract_from_pricer), or the keyword arguments of plan_american_contract
    (`dividends` needs cash_dividends="path") -- on the chosen engine.  Keys:
    price (the out-of-sample estimate), stderr,
    ci_95, fit_value and fit_stderr (the in-sample estimate, a diagnostic),
    n_paths, n_subruns, steps, invalid_fit_steps, min_margin, barrier_type."""
    _check_cash_dividends(cash_dividends)
    if contract is None:
        contract = plan_american_contract(cash_dividends=cash_dividends, **plan_kw)
    elif plan_kw:
        raise TypeError("give a contract or the keywords of plan_american_contract, not both")
    cfg = LsmConfig(n_subruns=int(n_subruns), antithetic=bool(antithetic), seed=int(seed))
    res = mc_american_batch([contract], cfg, engine=engine, stream_ids=[stream_id])[0]
    res.pop("sum_mean")
    res.pop("sum_mean2")
    return res


# ---------------------------------------------------------------------------
# the dual upper bound (include/fdcn.h, fdcn_mc_lsm_dual_batch)
# ---------------------------------------------------------------------------
_DUAL_BIT = 1 << 31              # bit 31 of counter word 3: the dual's streams
_OBS_BITS, _STEP_BITS, _OUTER_BITS = 14, 9, 10  # fields of the inner observation index
_INNER_CHUNK = 1 << 22           # path-steps of normals held at once by the host engine


@dataclass(frozen=True)
class DualConfig:
    n_outer: int = 8      # outer paths per sub-run
    n_inner: int = 2048   # inner paths per start


def _normals_at(obs: np.ndarray, n_steps: int, seed: int, word: int) -> np.ndarray:
    """z [..., n_steps] of the observations `obs` (uint64, any shape): the
    mapping of philox_normals for observation numbers that are not a range."""
    n_pairs = (n_steps + 1) // 2
    obs = np.asarray(obs, dtype=np.uint64)
    ctr = np.empty(obs.shape + (n_pairs, 4), dtype=np.uint64)
    ctr[..., 0] = (obs & np.uint64(0xFFFFFFFF))[..., None]
    ctr[..., 1] = (obs >> np.uint64(32))[..., None]
    ctr[..., 2] = np.arange(n_pairs, dtype=np.uint64)
    ctr[..., 3] = np.uint64(int(word))
    seed = int(seed) & (2 ** 64 - 1)
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))

    def u53(hi, lo):
        return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0
                + (lo >> np.uint32(6)).astype(np.float64) + 0.5) * 2.0 ** -53
    u1, u2 = u53(w[..., 0], w[..., 1]), u53(w[..., 2], w[..., 3])
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(obs.shape + (2 * n_pairs,))
    z[..., 0::2] = r * np.cos(2.0 * np.pi * u2)
    z[..., 1::2] = r * np.sin(2.0 * np.pi * u2)
    return z[..., :n_steps]


def _block_sum(v: np.ndarray) -> np.ndarray:
    """The kernel's sum of v [rows, n_inner] (path order): each thread its
    slots in slot order, then the fixed tree over the 256 threads."""
    rows = v.shape[0]
    v = v.reshape(rows, -1, _THREADS)
    s = np.zeros((rows, _THREADS))
    for k in range(v.shape[1]):
        s = s + v[:, k, :]
    off = _THREADS // 2
    while off > 0:
        s = s[:, :off] + s[:, off:2 * off]
        off //= 2
    return s[:, 0]


def _check_dual_sizes(n_outer, n_inner, antithetic: bool) -> None:
    if int(n_outer) != n_outer or not 1 <= n_outer <= capi.DUAL_MAX_OUTER:
        raise ValueError(f"n_outer must be in 1 .. {capi.DUAL_MAX_OUTER}")
    unit = 2 * _THREADS if antithetic else _THREADS
    if int(n_inner) != n_inner or not unit <= n_inner <= capi.DUAL_MAX_INNER or n_inner % unit:
        raise ValueError(f"n_inner must be a multiple of {_THREADS} ({2 * _THREADS} when "
                         f"antithetic) up to {capi.DUAL_MAX_INNER}")


def _check_dual_contract(c: LsmContract, cash_dividends: str = "refuse") -> None:
    if c.has_dividends and _check_cash_dividends(cash_dividends) == "refuse":
        raise ValueError("cash dividends are out of the dual bound's scope.")
    if int(c.flags[capi.LSM_F_KIND]) != 0 and np.any(c.step[:, capi.LSM_S_REBATE] < 0.0):
        raise ValueError("a negative rebate: the dual bound needs every cashflow >= 0.")


class _FittedRule:
    """Phase C's fitted rule for the dual walks: coef [g, n_steps, LSM_NCOEF],
    row crow[r] for outer path r."""

    def __init__(self, c: LsmContract, coef: np.ndarray, crow: np.ndarray):
        self.coef, self.crow = coef, crow
        self.centre, self.iscale = c.step[:, capi.LSM_S_CENTRE], c.step[:, capi.LSM_S_ISCALE]

    def any_at(self, rows, i) -> bool:
        return bool(np.any(self.coef[self.crow[rows], i, 4] != 0.0))

    def decide(self, rows, i, x, phi, live):
        """(stops, distance to the decision's edge; inf where none is taken)
        for the paths x of the outer paths `rows` (axis 0) at 0-based step i."""
        cc = self.coef[self.crow[rows], i]
        if x.ndim == 2:
            cc = cc[:, None, :]
        u = (x - self.centre[i]) * self.iscale[i]
        fit = cc[..., 0] + u * (cc[..., 1] + u * (cc[..., 2] + u * cc[..., 3]))
        cand = live & (cc[..., 4] != 0.0) & (phi > 0.0)
        return cand & (phi > fit), np.where(cand, np.abs(phi - fit), np.inf)


class _TableRule:
    """The table rule (include/fdcn.h, fdcn_mc_policy_batch): stop in the band
    [X_LO, X_HI] of the step where phi > 0; the decision is taken, and its
    margin counted, whatever phi is."""

    def __init__(self, policy: "ExercisePolicy"):
        self.lo, self.hi = policy.x_lo, policy.x_hi

    def any_at(self, rows, i) -> bool:
        return True

    def decide(self, rows, i, x, phi, live):
        lo, hi = self.lo[i], self.hi[i]
        gap = np.minimum(np.abs(x - lo), np.abs(x - hi))
        return live & (lo <= x) & (x <= hi) & (phi > 0.0), np.where(live, gap, np.inf)


def host_dual_subruns(c: LsmContract, coef: np.ndarray, subruns: Sequence[int], n_outer: int,
                      n_inner: int, antithetic: bool, seed: int, stream_id: int,
                      cash_dividends: str = "refuse") -> dict:
    """The dual estimator for the sub-runs `subruns` (absolute numbers) of
    contract c under the policies coef [g, n_steps, LSM_NCOEF], row for row of
    `subruns`: the kernel's operations per path on the same streams, the g *
    n_outer outer paths side by side.  -> gaps [g, n_outer] (D per outer
    path), cont [g, n_outer, n_steps] (the inner means, 0.0 where none was
    run), margin [g], inner_paths [g], inner_steps [g].  A contract that
    carries dividends needs cash_dividends="path": each step's dividend then
    follows its move on the outer and the inner walks (include/fdcn.h,
    fdcn_mc_lsm_dual_div_batch)."""
    coef = np.asarray(coef, dtype=float)
    if coef.shape != (len(subruns), c.n_steps, capi.LSM_NCOEF):
        raise ValueError("host_dual_subruns: coef [len(subruns), n_steps, LSM_NCOEF]")
    rule = _FittedRule(c, coef, np.repeat(np.arange(len(subruns)), int(n_outer)))
    return _host_dual(c, rule, subruns, n_outer, n_inner, antithetic, seed, stream_id,
                      cash_dividends)


def _host_dual(c: LsmContract, rule, subruns: Sequence[int], n_outer: int, n_inner: int,
               antithetic: bool, seed: int, stream_id: int,
               cash_dividends: str = "refuse") -> dict:
    """host_dual_subruns under `rule` (_FittedRule or _TableRule)."""
    _check_dual_sizes(n_outer, n_inner, bool(antithetic))
    _check_dual_contract(c, cash_dividends)
    P, F, S = c.params, c.flags, c.step
    M, ng = c.n_steps, len(subruns)
    if any(not 0 <= int(g) < 2 ** 31 for g in subruns):
        raise ValueError("host_dual_subruns: sub-run numbers must be in 0 .. 2^31 - 1")
    strike, lower, upper = float(P[capi.LSM_P_STRIKE]), float(P[capi.LSM_P_LOWER]), \
        float(P[capi.LSM_P_UPPER])
    put, kind = bool(F[capi.LSM_F_PUT]), int(F[capi.LSM_F_KIND])
    ko, ki = 1 <= kind <= 3, kind >= 4
    has_lo, has_hi = kind in (1, 3, 4, 6), kind in (2, 3, 5, 6)
    x0 = float(np.log(P[capi.LSM_P_SPOT]))
    w_outer = _DUAL_BIT + 2 * int(stream_id)
    w_inner = w_outer + 1
    n_obs = n_inner // 2 if antithetic else n_inner
    # inner path i of a start: its observation and the sign of its z
    i_path = np.arange(n_inner)
    k_slot, tid = i_path // _THREADS, i_path % _THREADS
    if antithetic:
        obs_of, sign = (k_slot // 2) * _THREADS + tid, np.where(k_slot % 2 == 1, -1.0, 1.0)
    else:
        obs_of, sign = i_path, np.ones(n_inner)

    def payoff(s):
        return np.maximum(strike - s, 0.0) if put else np.maximum(s - strike, 0.0)

    def breach(s):
        out = np.zeros(s.shape, dtype=bool)
        if has_lo:
            out |= s <= lower
        if has_hi:
            out |= s >= upper
        return out

    drift, diff = S[:, capi.LSM_S_DRIFT], S[:, capi.LSM_S_DIFF]
    mon = (S[:, capi.LSM_S_MONITOR] != 0.0) & (kind != 0)
    exr = S[:, capi.LSM_S_EXERCISE] != 0.0
    exr[M - 1] = False
    reb, dfe = S[:, capi.LSM_S_REBATE], S[:, capi.LSM_S_DF_END]
    Dv = c.div_row()  # after the move, before the step's events, on both walks

    R = ng * n_outer                                   # outer paths, row = g * n_outer + p
    sub = np.repeat(np.asarray([int(g) for g in subruns], dtype=np.uint64), n_outer)
    pth = np.tile(np.arange(n_outer, dtype=np.uint64), ng)
    Zo = _normals_at(sub * np.uint64(n_outer) + pth, M, seed, w_outer)
    margin = np.full(R, np.inf)
    walked = np.zeros(R)
    starts = np.zeros(R)
    cont = np.zeros((R, M))

    def inner(rows, i, x_start, in_start):
        """The mean over n_inner paths from step i + 1 (0-based i: the start
        step m = i + 1) for the outer paths `rows`."""
        n_rem = M - (i + 1)
        base = ((((sub[rows] << np.uint64(_OUTER_BITS)) + pth[rows]) << np.uint64(_STEP_BITS))
                + np.uint64(i)) << np.uint64(_OBS_BITS)
        z = _normals_at(base[:, None] + np.arange(n_obs, dtype=np.uint64)[None, :], n_rem, seed,
                        w_inner)
        n = len(rows)
        x = np.repeat(x_start[:, None], n_inner, axis=1)
        inn = np.repeat(in_start[:, None], n_inner, axis=1)
        val = np.zeros((n, n_inner))
        done = np.zeros((n, n_inner), dtype=bool)
        for t in range(n_rem):
            if done.all():
                break
            ii = i + 1 + t
            walked[rows] += np.sum(~done, axis=1)
            x = x + (drift[ii] + diff[ii] * (z[:, obs_of, t] * sign[None, :]))
            if Dv[ii] != 0.0:
                x = _div_forward(x, Dv[ii])
            ruled = bool(exr[ii]) and rule.any_at(rows, ii)
            if not (mon[ii] or ii == M - 1 or ruled):
                continue
            s = np.exp(x)
            phi = payoff(s)
            hit = breach(s) if mon[ii] else np.zeros((n, n_inner), dtype=bool)
            if ko:
                k = hit & ~done
                val = np.where(k, np.maximum(phi, reb[ii]) * dfe[ii], val)
                done |= k
            if ki:
                inn = inn | (hit & ~done)
            elig = inn if ki else np.ones((n, n_inner), dtype=bool)
            if ii == M - 1:
                val = np.where(~done, np.where(elig, phi, reb[ii]) * dfe[ii], val)
                done[:] = True
            elif ruled:
                go, gap = rule.decide(rows, ii, x, phi, ~done & elig)
                margin[rows] = np.minimum(margin[rows], gap.min(axis=1))
                val = np.where(go, phi * dfe[ii], val)
                done |= go
        return _block_sum(val) / float(n_inner)

    x = np.full(R, x0)
    r = np.zeros(R)
    D = np.full(R, -np.inf)
    inn = np.zeros(R, dtype=bool)
    alive = np.ones(R, dtype=bool)
    for i in range(M):
        x = x + (drift[i] + diff[i] * Zo[:, i])
        if Dv[i] != 0.0:
            x = _div_forward(x, Dv[i])
        last = i == M - 1
        if not (mon[i] or exr[i] or last):
            continue
        s = np.exp(x)
        phi = payoff(s)
        hit = breach(s) if mon[i] else np.zeros(R, dtype=bool)
        forced = alive & ((hit & ko) | last)
        if ki:
            inn = inn | (hit & alive)
        elig = inn if ki else np.ones(R, dtype=bool)
        live = alive & ~forced & bool(exr[i]) & elig
        go, gap = rule.decide(np.arange(R), i, x, phi, live)
        margin = np.minimum(margin, gap)
        rows_all = np.nonzero(live & (phi > 0.0))[0]
        per = max(1, _INNER_CHUNK // max(1, n_inner * (M - 1 - i)))
        for lo in range(0, len(rows_all), per):
            rows = rows_all[lo:lo + per]
            chat = inner(rows, i, x[rows], inn[rows])
            cont[rows, i] = chat
            starts[rows] += 1.0
            stops = go[rows]
            zc = phi[rows] * dfe[i] - chat
            D[rows] = np.where(stops, np.maximum(D[rows], 0.0 - r[rows]),
                               np.maximum(D[rows], zc - r[rows]))
            r[rows] = np.where(stops, r[rows] + zc, r[rows])
        D = np.where(forced, np.maximum(D, 0.0 - r), D)
        alive = alive & ~forced
    return dict(gaps=D.reshape(ng, n_outer), cont=cont.reshape(ng, n_outer, M),
                margin=margin.reshape(ng, n_outer).min(axis=1),
                inner_paths=starts.reshape(ng, n_outer).sum(axis=1) * float(n_inner),
                inner_steps=walked.reshape(ng, n_outer).sum(axis=1))


def _finalize_dual(gaps: np.ndarray, margin: float, paths: float, steps: float) -> np.ndarray:
    """One row of stats [DUAL_NSTAT] from the D of the outer paths, gaps
    [G, n_outer]: the kernels' sums in their order, _finalize's formulas."""
    G, n_outer = gaps.shape
    s, s2 = 0.0, 0.0
    for g in range(G):
        tot = 0.0
        for p in range(n_outer):
            tot += float(gaps[g, p])
        gap = tot / float(n_outer)
        s += gap
        s2 += gap * gap
    n = float(G)
    se = math.sqrt(max(0.0, s2 - s * s / n) / (n - 1.0) / n) if G > 1 else 0.0
    return np.array([s / n, se, s, s2, float(margin), float(paths), float(steps)])


def merge_dual_stats(parts) -> Dict[str, float]:
    """Gap and standard error of the union of disjoint sub-run ranges of one
    contract, from their (G, sum, sum of squares) of the sub-run gaps --
    tuples, or the result dicts of mc_american_bounds_batch (merge_lsm_stats
    does the lower bound's)."""
    G, s, s2 = 0, 0.0, 0.0
    for part in parts:
        if isinstance(part, dict):
            part = (part["n_subruns"], part["sum_gap"], part["sum_gap2"])
        G += int(part[0])
        s += float(part[1])
        s2 += float(part[2])
    if G <= 0:
        raise ValueError("merge_dual_stats: no sub-runs")
    n = float(G)
    stderr = math.sqrt(max(0.0, s2 - s * s / n) / (n - 1.0) / n) if G > 1 else 0.0
    return {"gap": s / n, "gap_stderr": stderr, "n_subruns": G, "sum_gap": s, "sum_gap2": s2}


def simulate_dual(group: Sequence[LsmContract], coef: np.ndarray, n_outer: int, n_inner: int,
                  antithetic: bool, *, engine: str = "hip", seed: int = 0,
                  stream_ids: Optional[Sequence[int]] = None, subrun_first: int = 0,
                  want_gap: bool = False, want_cont: bool = False, host_chunk: int = 16,
                  cash_dividends: str = "refuse") -> dict:
    """The dual estimator for contracts that share n_steps, under the policies
    coef [B, G, n_steps, LSM_NCOEF] -- simulate_lsm's "coef" of sub-runs
    subrun_first .. subrun_first + G - 1 with the same seed and stream ids.
    -> {"stats": [B, DUAL_NSTAT]} plus "gap" [B, G * n_outer] and "cont"
    [B, G * n_outer, n_steps] where asked for.  Contracts that carry dividends
    need cash_dividends="path"; one of them sends the launch through the div
    entry."""
    _check_cash_dividends(cash_dividends)
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    B = len(group)
    if B < 1:
        raise ValueError("simulate_dual: no contracts")
    n_steps = group[0].n_steps
    if any(c.n_steps != n_steps for c in group):
        raise ValueError("simulate_dual: the contracts of a launch share n_steps")
    if n_steps > capi.LSM_MAX_STEPS:
        raise ValueError(f"simulate_dual: at most {capi.LSM_MAX_STEPS} steps")
    if coef is None:
        raise ValueError("simulate_dual: coef is missing (simulate_lsm with want_coef=True)")
    coef = np.ascontiguousarray(coef, dtype=np.float64)
    if (coef.ndim != 4 or coef.shape[0] != B or coef.shape[1] < 1
            or coef.shape[2:] != (n_steps, capi.LSM_NCOEF)):
        raise ValueError("simulate_dual: coef [B, G, n_steps, LSM_NCOEF]")
    if not np.all(np.isfinite(coef)):
        raise ValueError("simulate_dual: a coefficient is not finite")
    G = coef.shape[1]
    antithetic = bool(antithetic)
    _check_dual_sizes(n_outer, n_inner, antithetic)
    n_outer, n_inner = int(n_outer), int(n_inner)
    first = int(subrun_first)
    if first != subrun_first or first < 0 or first + G > 2 ** 31:
        raise ValueError("simulate_dual: subrun_first must be a whole, non-negative number of "
                         "sub-runs with subrun_first + G <= 2^31")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError("simulate_dual: one stream id per contract")
    if any(not 0 <= s < 2 ** 30 for s in ids):
        raise ValueError("simulate_dual: stream ids must be in 0 .. 2^30 - 1")
    for c in group:
        _check_dual_contract(c, cash_dividends)
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)
        stats, gap, cont = capi.mc_dual_batch(P, F, S, coef, n_outer, n_inner, antithetic,
                                              seed=seed, subrun_first=first, want_gap=want_gap,
                                              want_cont=want_cont, div=_div_rows(group))
    else:
        stats = np.empty((B, capi.DUAL_NSTAT))
        gap = np.empty((B, G * n_outer))
        cont = np.empty((B, G * n_outer, n_steps)) if want_cont else None
        step = max(1, int(host_chunk))
        for b, c in enumerate(group):
            margin, paths, steps = math.inf, 0.0, 0.0
            for lo in range(0, G, step):
                hi = min(G, lo + step)
                r = host_dual_subruns(c, coef[b, lo:hi], range(first + lo, first + hi), n_outer,
                                      n_inner, antithetic, seed, ids[b], cash_dividends)
                gap[b, lo * n_outer:hi * n_outer] = r["gaps"].reshape(-1)
                if want_cont:
                    cont[b, lo * n_outer:hi * n_outer] = r["cont"].reshape(-1, n_steps)
                margin = min(margin, float(r["margin"].min()))
                paths += float(r["inner_paths"].sum())
                steps += float(r["inner_steps"].sum())
            stats[b] = _finalize_dual(gap[b].reshape(G, n_outer), margin, paths, steps)
        if not want_gap:
            gap = None
    out = {"stats": stats}
    if want_gap:
        out["gap"] = gap
    if want_cont:
        out["cont"] = cont
    return out


def _bounds_result(res: dict, dual: DualConfig, st: Optional[np.ndarray]) -> dict:
    if st is None:  # a fixed price: nothing simulated, both bounds are the price
        st = np.array([0.0, 0.0, 0.0, 0.0, math.inf, 0.0, 0.0])
    gap, gap_se = float(st[capi.DUAL_O_GAP]), float(st[capi.DUAL_O_STDERR])
    res = dict(res)
    res.update({
        "gap": gap,
        "gap_stderr": gap_se,
        "upper": res["price"] + gap,
        "upper_stderr": math.sqrt(res["stderr"] ** 2 + gap_se ** 2),
        "n_outer": int(dual.n_outer),
        "n_inner": int(dual.n_inner),
        "sum_gap": float(st[capi.DUAL_O_SUM]),
        "sum_gap2": float(st[capi.DUAL_O_SUM2]),
        "dual_min_margin": float(st[capi.DUAL_O_MIN_MARGIN]),
        "inner_paths": int(st[capi.DUAL_O_INNER_PATHS]),
    })
    return res


def mc_american_bounds_batch(contracts: Sequence, cfg: LsmConfig = LsmConfig(),
                             dual: DualConfig = DualConfig(), *, engine: str = "hip",
                             stream_ids: Optional[Sequence[int]] = None,
                             subrun_range: Optional[range] = None,
                             cash_dividends: str = "refuse") -> List[dict]:
    """Lower and upper bound of many contracts: per distinct (step count, has
    dividends) one least-squares Monte Carlo launch that keeps its
    coefficients, then one dual launch under them.  Arguments as
    mc_american_batch; contracts with cash dividends are refused unless
    cash_dividends="path", which also plans the keyword contracts that do not
    name a mode of their own.  Results, in input order: mc_american_batch's
    dict plus "gap" and "gap_stderr" (mean and standard error of the sub-run
    gaps), "upper" = price + gap, "upper_stderr" = sqrt(stderr^2 +
    gap_stderr^2), "n_outer", "n_inner", "sum_gap" and "sum_gap2"
    (merge_dual_stats), "dual_min_margin" and "inner_paths".

    upper_stderr ignores the covariance between a sub-run's lower mean and its
    gap.  That covariance is negative -- a sub-run with a poor policy has a low
    mean and a large gap --, so the figure errs wide.  The inner-sampling noise
    biases the gap upward by an amount that shrinks with n_inner: the safe
    side for an upper bound.  A contract with a `fixed_price` gets gap 0 and
    upper = price."""
    if _check_cash_dividends(cash_dividends) == "refuse":
        plans = [c if isinstance(c, LsmContract) else plan_american_contract(**c)
                 for c in contracts]
    else:
        plans = [c if isinstance(c, LsmContract)
                 else plan_american_contract(**{"cash_dividends": cash_dividends, **c})
                 for c in contracts]
    for c in plans:
        _check_dual_contract(c, cash_dividends)
    _check_dual_sizes(dual.n_outer, dual.n_inner, bool(cfg.antithetic))
    lo, hi = 0, int(cfg.n_subruns)
    if hi < 1:
        raise ValueError("cfg.n_subruns must be positive.")
    if subrun_range is not None:
        lo, hi = subrun_range.start, subrun_range.stop
        if subrun_range.step != 1 or not 0 <= lo < hi <= cfg.n_subruns:
            raise ValueError("subrun_range must be a non-empty contiguous range within the "
                             "contract's sub-runs")
    ids = list(range(len(plans))) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != len(plans):
        raise ValueError("one stream id per contract")
    out: List[Optional[dict]] = [None] * len(plans)
    by_steps: Dict[tuple, List[int]] = {}
    for k, c in enumerate(plans):
        if c.fixed_price is not None:
            out[k] = _bounds_result(_result(c, cfg, hi - lo, None), dual, None)
        else:
            by_steps.setdefault((c.n_steps, c.has_dividends), []).append(k)
    for members in by_steps.values():
        group = [plans[k] for k in members]
        kw = dict(engine=engine, seed=cfg.seed, stream_ids=[ids[k] for k in members],
                  subrun_first=lo)
        r = simulate_lsm(group, hi - lo, cfg.antithetic, want_coef=True, **kw)
        d = simulate_dual(group, r["coef"], dual.n_outer, dual.n_inner, cfg.antithetic,
                          cash_dividends=cash_dividends, **kw)
        for row, k in enumerate(members):
            out[k] = _bounds_result(_result(plans[k], cfg, hi - lo, r["stats"][row]), dual,
                                    d["stats"][row])
    return out  # type: ignore[return-value]


def price_american_mc_bounds(contract: Optional[LsmContract] = None, *, n_subruns: int = 32,
                             antithetic: bool = True, seed: int = 42, stream_id: int = 0,
                             n_outer: int = 8, n_inner: int = 2048, engine: str = "hip",
                             cash_dividends: str = "refuse", **plan_kw) -> Dict[str, object]:
    """Lower and upper bound of one contract -- an LsmContract, or the keyword
    arguments of plan_american_contract (`dividends` needs
    cash_dividends="path", which plans and permits with the one keyword):
    price_american_mc's keys plus those mc_american_bounds_batch adds."""
    _check_cash_dividends(cash_dividends)
    if contract is None:
        contract = plan_american_contract(cash_dividends=cash_dividends, **plan_kw)
    elif plan_kw:
        raise TypeError("give a contract or the keywords of plan_american_contract, not both")
    cfg = LsmConfig(n_subruns=int(n_subruns), antithetic=bool(antithetic), seed=int(seed))
    return mc_american_bounds_batch([contract], cfg, DualConfig(int(n_outer), int(n_inner)),
                                    engine=engine, stream_ids=[stream_id],
                                    cash_dividends=cash_dividends)[0]


def brackets(result: dict, fd_price: float, grid_error: float = 0.0, z: float = 5.0) -> bool:
    """Does the two-sided bracket of `result` (mc_american_bounds_batch) hold
    `fd_price`?  True when
        price - z * stderr - grid_error <= fd_price <= upper + z * upper_stderr + grid_error,
    grid_error the FD price's own uncertainty (its change over the last grid
    doubling, say).  No percentage allowance: the lower bound's policy bias is
    what the upper bound is there for."""
    lower = float(result["price"]) - z * float(result["stderr"]) - float(grid_error)
    upper = float(result["upper"]) + z * float(result["upper_stderr"]) + float(grid_error)
    return bool(lower <= float(fd_price) <= upper)


# ---------------------------------------------------------------------------
# bounds under a given exercise table (include/fdcn.h, fdcn_mc_policy_batch)
# ---------------------------------------------------------------------------
@dataclass
class ExercisePolicy:
    """A per-step exercise rule: at step m the holder stops where the path is
    eligible, X_LO_m <= ln(s) <= X_HI_m (both ends inclusive) and the payoff
    is positive.  +-inf are legal, x_lo > x_hi means never at that step, and
    a row on a step without an EXERCISE flag is ignored."""
    x_lo: np.ndarray   # [n_steps]
    x_hi: np.ndarray   # [n_steps]

    def __post_init__(self):
        self.x_lo = np.array(self.x_lo, dtype=float)
        self.x_hi = np.array(self.x_hi, dtype=float)
        if self.x_lo.ndim != 1 or self.x_lo.shape != self.x_hi.shape or self.x_lo.size < 1:
            raise ValueError("ExercisePolicy: x_lo and x_hi are shaped [n_steps]")
        if np.isnan(self.x_lo).any() or np.isnan(self.x_hi).any():
            raise ValueError("ExercisePolicy: a NaN entry (+-inf are legal)")

    @property
    def n_steps(self) -> int:
        return self.x_lo.shape[0]

    def table(self) -> np.ndarray:
        """[n_steps, POLICY_NCOL], the engines' layout."""
        return np.stack([self.x_lo, self.x_hi], axis=1)

    @classmethod
    def never(cls, n_steps: int) -> "ExercisePolicy":
        return cls(np.full(n_steps, np.inf), np.full(n_steps, -np.inf))

    @classmethod
    def always(cls, n_steps: int) -> "ExercisePolicy":
        return cls(np.full(n_steps, -np.inf), np.full(n_steps, np.inf))

    @classmethod
    def from_critical_spots(cls, contract: LsmContract, spots: Dict) -> "ExercisePolicy":
        """The threshold policy of `contract` from {t_m: (s_below, s_above)}:
        the two spots between which exercise stops being optimal at the
        exercise time t_m (matched to the contract's steps within 1e-12), or
        None for "never at t_m".  A put stops at and below the midpoint in
        log-spot of the pair (X_LO = -inf), a call at and above it (X_HI =
        +inf); s_below = 0 or s_above = inf puts the threshold at that end.
        Every EXERCISE step before maturity needs an entry, and every entry a
        step; the other steps get "never".

        A contract of the American kind planned with cash dividends has two
        steps at a dividend date t_d (plan_american_contract): the exercise on
        the cum-dividend spot, then the zero-length step that pays the dividend
        and exercises on the ex-dividend spot.  Such a time takes
        {"cum": pair_or_None, "ex": pair_or_None}, one entry per step; a plain
        pair there is an error, because it would not say which spot it is in."""
        M = contract.n_steps
        put = bool(contract.flags[capi.LSM_F_PUT])
        pol = cls.never(M)
        ex = contract.step[:, capi.LSM_S_EXERCISE] != 0.0
        ex[M - 1] = False
        seen = np.zeros(M, dtype=bool)
        entries: List[tuple] = []  # (step, pair or None)
        for t, pair in spots.items():
            i = int(np.argmin(np.abs(contract.times - float(t))))
            if abs(float(contract.times[i]) - float(t)) > _MERGE or seen[i]:
                raise ValueError(f"from_critical_spots: time {t!r} is not one step of the contract")
            two = i + 1 < M and abs(float(contract.times[i + 1] - contract.times[i])) <= _MERGE
            if two:
                if not (isinstance(pair, dict) and set(pair) == {"cum", "ex"}):
                    raise ValueError(
                        f"from_critical_spots: time {t!r} is a dividend date of two steps "
                        f"({i + 1}: cum-dividend, {i + 2}: ex-dividend): give "
                        "{'cum': pair_or_None, 'ex': pair_or_None}")
                seen[i] = seen[i + 1] = True
                entries += [(i, pair["cum"]), (i + 1, pair["ex"])]
            else:
                if isinstance(pair, dict):
                    raise ValueError(f"from_critical_spots: time {t!r} is one step, not a "
                                     "cum- / ex-dividend pair of steps")
                seen[i] = True
                entries.append((i, pair))
        for i, pair in entries:
            if pair is None:
                continue
            below, above = float(pair[0]), float(pair[1])
            if not 0.0 <= below <= above or math.isnan(above):
                raise ValueError("from_critical_spots: 0 <= s_below <= s_above")
            with np.errstate(divide="ignore"):
                mid = 0.5 * (float(np.log(below)) + float(np.log(above)))
            if math.isnan(mid):  # (0, inf): everywhere
                mid = math.inf if put else -math.inf
            if put:
                pol.x_lo[i], pol.x_hi[i] = -math.inf, mid
            else:
                pol.x_lo[i], pol.x_hi[i] = mid, math.inf
        if np.any(ex & ~seen):
            m = int(np.nonzero(ex & ~seen)[0][0]) + 1
            raise ValueError(f"from_critical_spots: exercise step {m} (t = "
                             f"{float(contract.times[m - 1])!r}) has no entry")
        return pol


def policy_from_pricer(p, contract: Optional[LsmContract] = None,
                       n_time: Optional[int] = None,
                       cash_dividends: str = "refuse") -> ExercisePolicy:
    """The exercise boundary of the BermudanFDMPricer `p` as the policy of
    `contract` (default: contract_from_pricer(p, cash_dividends=cash_dividends)).

    `p.exercise_boundary(n_time)` gives, per exercise date, the nodes at which
    the payoff exceeded the continuation value; its records are matched to
    the contract's steps by time (within 1e-12), and an exercise step without
    a record is an error.  A put stops at and below X_HI, the midpoint in
    log-spot of s_nodes[hi] and s_nodes[hi + 1] (X_LO = -inf); a call at and
    above X_LO, the midpoint of s_nodes[lo - 1] and s_nodes[lo] (X_HI = +inf);
    a record with count == 0 gives "never".  The exact sign change lies
    between those two nodes: the midpoint halves the worst case, and any
    threshold is a valid policy -- it can only lower the lower bound and
    widen the gap.

    Only a BermudanFDMPricer is taken: its exercise dates are calendar dates
    that coincide with the contract's steps, while the American classes are
    simulated on the grid k T / n_exercise, which no boundary record lies on.
    A knock-in contract takes the policy of a vanilla Bermudan twin: give the
    twin as `p` and the knock-in contract (same exercise times) as `contract`;
    the Monte Carlo applies the rule from the hit step on.

    Pricers and contracts with cash dividends in their life are refused unless
    cash_dividends="path".  The Bermudan class takes a date's dividend first
    and then the date's events on the ex-dividend spot (marching backward: the
    exercise event, then the dividend jump), and so does the contract's single
    step of that date.  The boundary record of an exercise date that is also a
    dividend date is therefore already in ex-dividend spots and maps to its
    step unchanged."""
    from .bermudan import BermudanFDMPricer
    if not isinstance(p, BermudanFDMPricer):
        raise ValueError(f"policy_from_pricer takes a BermudanFDMPricer, not {type(p).__name__}: "
                         "only Bermudan exercise dates coincide with the contract's steps (the "
                         "American classes are simulated on the grid k T / n_exercise).")
    refuse = _check_cash_dividends(cash_dividends) == "refuse"
    if refuse and p._div_times_tau():
        raise ValueError("cash dividends are out of the table policy's scope.")
    if contract is None:
        contract = contract_from_pricer(p, cash_dividends=cash_dividends)
    if refuse and contract.has_dividends:
        raise ValueError("cash dividends are out of the table policy's scope.")
    put = p.option_type == "put"
    if put != bool(contract.flags[capi.LSM_F_PUT]):
        raise ValueError("policy_from_pricer: the pricer and the contract differ in option type")
    recs = p.exercise_boundary(n_time)
    s = np.asarray(p.s_nodes, dtype=float)
    n = s.shape[0]
    spots: Dict[float, Optional[tuple]] = {}
    for _date, t, _s_star, lo, hi, count in recs:
        if count == 0:
            spots[t] = None
        elif put:
            spots[t] = (float(s[hi]), float(s[hi + 1]) if hi + 1 < n else math.inf)
        else:
            spots[t] = (float(s[lo - 1]) if lo >= 1 else 0.0, float(s[lo]))
    return ExercisePolicy.from_critical_spots(contract, spots)


def _check_policy(c: LsmContract, policy: ExercisePolicy,
                  cash_dividends: str = "refuse") -> None:
    if not isinstance(policy, ExercisePolicy):
        raise TypeError("an ExercisePolicy per contract")
    if policy.n_steps != c.n_steps:
        raise ValueError(f"the policy has {policy.n_steps} steps, the contract {c.n_steps}")
    if c.has_dividends and _check_cash_dividends(cash_dividends) == "refuse":
        raise ValueError("cash dividends are out of the table policy's scope.")


def _div_rows(group: Sequence[LsmContract]) -> Optional[np.ndarray]:
    """div [B, n_steps] of a launch: one contract with a dividend sends the
    launch through the div entry; None takes the plain one."""
    if not any(c.has_dividends for c in group):
        return None
    return np.stack([c.div_row() for c in group])


def host_policy_subruns(c: LsmContract, policy: ExercisePolicy, subruns: Sequence[int],
                        antithetic: bool, seed: int, stream_id: int,
                        cash_dividends: str = "refuse") -> dict:
    """The sub-runs `subruns` of contract c under `policy` on the host: the
    kernel's operations per path on the LSM's price-set streams.  -> values
    [g, LSM_SUBRUN], stop_step [g, LSM_SUBRUN] (the step m at which each path
    stopped), means [g] (the kernel's sum: slot order, then the fixed tree),
    margin [g], exercised [g] (paths the rule stopped).  A contract that
    carries dividends needs cash_dividends="path": each step's dividend then
    follows its move and precedes its events (fdcn_mc_policy_div_batch)."""
    _check_policy(c, policy, cash_dividends)
    P, F, S = c.params, c.flags, c.step
    M, ng, n = c.n_steps, len(subruns), capi.LSM_SUBRUN
    strike, lower, upper = float(P[capi.LSM_P_STRIKE]), float(P[capi.LSM_P_LOWER]), \
        float(P[capi.LSM_P_UPPER])
    put, kind = bool(F[capi.LSM_F_PUT]), int(F[capi.LSM_F_KIND])
    ko, ki = 1 <= kind <= 3, kind >= 4
    has_lo, has_hi = kind in (1, 3, 4, 6), kind in (2, 3, 5, 6)
    x0 = float(np.log(P[capi.LSM_P_SPOT]))
    per = obs_per_subrun(antithetic)

    def payoff(s):
        return np.maximum(strike - s, 0.0) if put else np.maximum(s - strike, 0.0)

    def breach(s):
        out = np.zeros(s.shape, dtype=bool)
        if has_lo:
            out |= s <= lower
        if has_hi:
            out |= s >= upper
        return out

    drift, diff = S[:, capi.LSM_S_DRIFT], S[:, capi.LSM_S_DIFF]
    mon = (S[:, capi.LSM_S_MONITOR] != 0.0) & (kind != 0)
    exr = S[:, capi.LSM_S_EXERCISE] != 0.0
    exr[M - 1] = False
    reb, dfe = S[:, capi.LSM_S_REBATE], S[:, capi.LSM_S_DF_END]
    Dv = c.div_row()
    rule = _TableRule(policy)
    Z = np.stack([_path_normals(M, seed, 2 * int(stream_id) + 1, int(g) * per, antithetic)
                  for g in subruns])
    x = np.full((ng, n), x0)
    val = np.zeros((ng, n))
    stop = np.zeros((ng, n), dtype=np.int64)
    done = np.zeros((ng, n), dtype=bool)
    inn = np.zeros((ng, n), dtype=bool)
    margin = np.full(ng, np.inf)
    exercised = np.zeros(ng)
    for m in range(1, M + 1):
        i = m - 1
        x = x + (drift[i] + diff[i] * Z[:, :, i])
        if Dv[i] != 0.0:
            x = _div_forward(x, Dv[i])
        if not (mon[i] or exr[i] or m == M):
            continue
        s = np.exp(x)
        phi = payoff(s)
        hit = breach(s) if mon[i] else np.zeros((ng, n), dtype=bool)
        if ko:
            k = hit & ~done
            val = np.where(k, np.maximum(phi, reb[i]) * dfe[i], val)
            stop[k] = m
            done |= k
        if ki:
            inn |= hit & ~done
        elig = inn if ki else np.ones((ng, n), dtype=bool)
        if m == M:
            val = np.where(~done, np.where(elig, phi, reb[i]) * dfe[i], val)
            stop[~done] = m
            done[:] = True
        elif exr[i]:
            go, gap = rule.decide(None, i, x, phi, ~done & elig)
            margin = np.minimum(margin, gap.min(axis=1))
            val = np.where(go, phi * dfe[i], val)
            stop[go] = m
            done |= go
            exercised += go.sum(axis=1)
    return dict(values=val, stop_step=stop, means=_block_sum(val) / float(n), margin=margin,
                exercised=exercised)


def host_policy_dual_subruns(c: LsmContract, policy: ExercisePolicy, subruns: Sequence[int],
                             n_outer: int, n_inner: int, antithetic: bool, seed: int,
                             stream_id: int, cash_dividends: str = "refuse") -> dict:
    """host_dual_subruns under the table `policy` (one for all sub-runs) in the
    place of the fitted coefficients: the same streams, sums and outputs."""
    _check_policy(c, policy, cash_dividends)
    return _host_dual(c, _TableRule(policy), subruns, n_outer, n_inner, antithetic, seed,
                      stream_id, cash_dividends)


def _finalize_policy(means: np.ndarray, margin: float, exercised: float) -> np.ndarray:
    """One row of stats [POLICY_NSTAT] from the sub-run means, the finalize
    kernel's sums in its order."""
    G = means.shape[0]
    s, s2 = 0.0, 0.0
    for g in range(G):
        s += float(means[g])
        s2 += float(means[g]) * float(means[g])
    n = float(G)
    se = math.sqrt(max(0.0, s2 - s * s / n) / (n - 1.0) / n) if G > 1 else 0.0
    return np.array([s / n, se, s, s2, float(margin), float(exercised)])


def merge_policy_stats(parts) -> Dict[str, float]:
    """merge_lsm_stats for the result dicts of mc_policy_batch (or (G, sum, sum
    of squares) tuples) of disjoint sub-run ranges of one contract; the dual
    part merges through merge_dual_stats.  "exercised" adds up."""
    parts = list(parts)
    out = merge_lsm_stats(parts)
    if all(isinstance(part, dict) for part in parts):
        out["exercised"] = int(sum(part["exercised"] for part in parts))
        out["min_margin"] = min(float(part["min_margin"]) for part in parts)
    return out


def _policy_group(who: str, group, policies, n_subruns, subrun_first, stream_ids, engine,
                  cash_dividends: str = "refuse"):
    _check_cash_dividends(cash_dividends)
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    B = len(group)
    if B < 1:
        raise ValueError(f"{who}: no contracts")
    if len(policies) != B:
        raise ValueError(f"{who}: one policy per contract")
    n_steps = group[0].n_steps
    if any(c.n_steps != n_steps for c in group):
        raise ValueError(f"{who}: the contracts of a launch share n_steps")
    if n_steps > capi.LSM_MAX_STEPS:
        raise ValueError(f"{who}: at most {capi.LSM_MAX_STEPS} steps")
    for c, pol in zip(group, policies):
        _check_policy(c, pol, cash_dividends)
    G = int(n_subruns)
    if G < 1:
        raise ValueError(f"{who}: n_subruns must be >= 1")
    first = int(subrun_first)
    if first != subrun_first or first < 0 or first + G > 2 ** 31:
        raise ValueError(f"{who}: subrun_first must be a whole, non-negative number of sub-runs "
                         "with subrun_first + n_subruns <= 2^31")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError(f"{who}: one stream id per contract")
    if any(not 0 <= s < 2 ** 30 for s in ids):
        raise ValueError(f"{who}: stream ids must be in 0 .. 2^30 - 1")
    return B, n_steps, G, first, ids


def simulate_policy(group: Sequence[LsmContract], policies: Sequence[ExercisePolicy],
                    n_subruns: int, antithetic: bool, *, engine: str = "hip", seed: int = 0,
                    stream_ids: Optional[Sequence[int]] = None, subrun_first: int = 0,
                    want_values: bool = False, host_chunk: int = 16,
                    cash_dividends: str = "refuse") -> dict:
    """simulate_lsm under given policies, one per contract: -> {"stats":
    [B, POLICY_NSTAT]} plus "values" [B, n_subruns * LSM_SUBRUN] where asked
    for, the paths those of simulate_lsm's "values".  Contracts that carry
    dividends need cash_dividends="path"; one of them sends the launch through
    the div entry."""
    B, n_steps, G, first, ids = _policy_group("simulate_policy", group, policies, n_subruns,
                                              subrun_first, stream_ids, engine, cash_dividends)
    antithetic = bool(antithetic)
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)
        T = np.stack([pol.table() for pol in policies])
        stats, val = capi.mc_policy_batch(P, F, S, T, G, antithetic, seed=seed,
                                          obs_first=first * obs_per_subrun(antithetic),
                                          want_values=want_values, div=_div_rows(group))
    else:
        stats = np.empty((B, capi.POLICY_NSTAT))
        val = np.empty((B, G * capi.LSM_SUBRUN)) if want_values else None
        step = max(1, int(host_chunk))
        for b, (c, pol) in enumerate(zip(group, policies)):
            means = np.empty(G)
            margin, exercised = math.inf, 0.0
            for lo in range(0, G, step):
                hi = min(G, lo + step)
                r = host_policy_subruns(c, pol, range(first + lo, first + hi), antithetic, seed,
                                        ids[b], cash_dividends)
                means[lo:hi] = r["means"]
                margin = min(margin, float(r["margin"].min()))
                exercised += float(r["exercised"].sum())
                if want_values:
                    val[b, lo * capi.LSM_SUBRUN:hi * capi.LSM_SUBRUN] = r["values"].reshape(-1)
            stats[b] = _finalize_policy(means, margin, exercised)
    out = {"stats": stats}
    if want_values:
        out["values"] = val
    return out


def simulate_policy_dual(group: Sequence[LsmContract], policies: Sequence[ExercisePolicy],
                         n_subruns: int, n_outer: int, n_inner: int, antithetic: bool, *,
                         engine: str = "hip", seed: int = 0,
                         stream_ids: Optional[Sequence[int]] = None, subrun_first: int = 0,
                         want_gap: bool = False, want_cont: bool = False,
                         host_chunk: int = 16, cash_dividends: str = "refuse") -> dict:
    """simulate_dual under given policies, one per contract: -> {"stats":
    [B, DUAL_NSTAT]} plus "gap" [B, G * n_outer] and "cont" [B, G * n_outer,
    n_steps] where asked for; cash_dividends as in simulate_policy."""
    B, n_steps, G, first, ids = _policy_group("simulate_policy_dual", group, policies,
                                              n_subruns, subrun_first, stream_ids, engine,
                                              cash_dividends)
    antithetic = bool(antithetic)
    _check_dual_sizes(n_outer, n_inner, antithetic)
    n_outer, n_inner = int(n_outer), int(n_inner)
    for c in group:
        _check_dual_contract(c, cash_dividends)
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)
        T = np.stack([pol.table() for pol in policies])
        stats, gap, cont = capi.mc_policy_dual_batch(
            P, F, S, T, G, n_outer, n_inner, antithetic, seed=seed, subrun_first=first,
            want_gap=want_gap, want_cont=want_cont, div=_div_rows(group))
    else:
        stats = np.empty((B, capi.DUAL_NSTAT))
        gap = np.empty((B, G * n_outer))
        cont = np.empty((B, G * n_outer, n_steps)) if want_cont else None
        step = max(1, int(host_chunk))
        for b, (c, pol) in enumerate(zip(group, policies)):
            margin, paths, steps = math.inf, 0.0, 0.0
            for lo in range(0, G, step):
                hi = min(G, lo + step)
                r = host_policy_dual_subruns(c, pol, range(first + lo, first + hi), n_outer,
                                             n_inner, antithetic, seed, ids[b], cash_dividends)
                gap[b, lo * n_outer:hi * n_outer] = r["gaps"].reshape(-1)
                if want_cont:
                    cont[b, lo * n_outer:hi * n_outer] = r["cont"].reshape(-1, n_steps)
                margin = min(margin, float(r["margin"].min()))
                paths += float(r["inner_paths"].sum())
                steps += float(r["inner_steps"].sum())
            stats[b] = _finalize_dual(gap[b].reshape(G, n_outer), margin, paths, steps)
        if not want_gap:
            gap = None
    out = {"stats": stats}
    if want_gap:
        out["gap"] = gap
    if want_cont:
        out["cont"] = cont
    return out


def _policy_result(c: LsmContract, G: int, st: Optional[np.ndarray]) -> dict:
    if st is None:  # answered by the pricer's own rule, nothing simulated
        price = float(c.fixed_price)
        st = np.array([price, 0.0, price * G, price * price * G, math.inf, 0.0])
        n_paths = 0
    else:
        n_paths = G * capi.LSM_SUBRUN
    price, stderr = float(st[capi.POLICY_O_PRICE]), float(st[capi.POLICY_O_STDERR])
    return {
        "price": price,
        "stderr": stderr,
        "ci_95": (price - 1.96 * stderr, price + 1.96 * stderr),
        "n_paths": int(n_paths),
        "n_subruns": int(G),
        "steps": int(c.n_steps),
        "min_margin": float(st[capi.POLICY_O_MIN_MARGIN]),
        "exercised": int(st[capi.POLICY_O_EXERCISED]),
        "barrier_type": c.barrier_type,
        "sum_mean": float(st[capi.POLICY_O_SUM]),
        "sum_mean2": float(st[capi.POLICY_O_SUM2]),
    }


def _policy_batches(contracts, policies, cfg: LsmConfig, subrun_range, stream_ids,
                    cash_dividends: str = "refuse"):
    _check_cash_dividends(cash_dividends)
    plans = list(contracts)
    if any(not isinstance(c, LsmContract) for c in plans):
        raise TypeError("the table policy takes LsmContract objects (a policy is made for one)")
    policies = list(policies)
    if len(policies) != len(plans):
        raise ValueError("one policy per contract")
    for c, pol in zip(plans, policies):
        if c.fixed_price is None:
            _check_policy(c, pol, cash_dividends)
    lo, hi = 0, int(cfg.n_subruns)
    if hi < 1:
        raise ValueError("cfg.n_subruns must be positive.")
    if subrun_range is not None:
        lo, hi = subrun_range.start, subrun_range.stop
        if subrun_range.step != 1 or not 0 <= lo < hi <= cfg.n_subruns:
            raise ValueError("subrun_range must be a non-empty contiguous range within the "
                             "contract's sub-runs")
    ids = list(range(len(plans))) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != len(plans):
        raise ValueError("one stream id per contract")
    by_steps: Dict[tuple, List[int]] = {}
    for k, c in enumerate(plans):
        if c.fixed_price is None:
            by_steps.setdefault((c.n_steps, c.has_dividends), []).append(k)
    return plans, policies, lo, hi, ids, by_steps


def mc_policy_batch(contracts: Sequence[LsmContract], policies: Sequence[ExercisePolicy],
                    cfg: LsmConfig = LsmConfig(), *, engine: str = "hip",
                    stream_ids: Optional[Sequence[int]] = None,
                    subrun_range: Optional[range] = None,
                    cash_dividends: str = "refuse") -> List[dict]:
    """The lower bound of many contracts under given policies, one launch per
    distinct (step count, has dividends); arguments as mc_american_batch
    (contracts that carry dividends need cash_dividends="path").  A `fixed_price`
    contract is answered without a launch (its policy is not read).  Results,
    in input order: price, stderr, ci_95, n_paths, n_subruns, steps,
    min_margin (the smallest distance of a decision's log-spot to a finite
    threshold), exercised (paths the rule stopped), barrier_type, sum_mean and
    sum_mean2 (merge_policy_stats)."""
    plans, policies, lo, hi, ids, by_steps = _policy_batches(contracts, policies, cfg,
                                                             subrun_range, stream_ids,
                                                             cash_dividends)
    out: List[Optional[dict]] = [None if c.fixed_price is None else _policy_result(c, hi - lo, None)
                                 for c in plans]
    for members in by_steps.values():
        r = simulate_policy([plans[k] for k in members], [policies[k] for k in members], hi - lo,
                            cfg.antithetic, engine=engine, seed=cfg.seed,
                            stream_ids=[ids[k] for k in members], subrun_first=lo,
                            cash_dividends=cash_dividends)
        for row, k in enumerate(members):
            out[k] = _policy_result(plans[k], hi - lo, r["stats"][row])
    return out  # type: ignore[return-value]


def price_policy_mc(contract: LsmContract, policy: ExercisePolicy, *, n_subruns: int = 32,
                    antithetic: bool = True, seed: int = 42, stream_id: int = 0,
                    engine: str = "hip", cash_dividends: str = "refuse") -> Dict[str, object]:
    """The lower bound of one contract under `policy`: mc_policy_batch's dict
    without the merging sums."""
    cfg = LsmConfig(n_subruns=int(n_subruns), antithetic=bool(antithetic), seed=int(seed))
    res = mc_policy_batch([contract], [policy], cfg, engine=engine, stream_ids=[stream_id],
                          cash_dividends=cash_dividends)[0]
    res.pop("sum_mean")
    res.pop("sum_mean2")
    return res


def mc_policy_bounds_batch(contracts: Sequence[LsmContract], policies: Sequence[ExercisePolicy],
                           cfg: LsmConfig = LsmConfig(), dual: DualConfig = DualConfig(), *,
                           engine: str = "hip", stream_ids: Optional[Sequence[int]] = None,
                           subrun_range: Optional[range] = None,
                           cash_dividends: str = "refuse") -> List[dict]:
    """Lower and upper bound of many contracts under given policies: per
    distinct (step count, has dividends) one lower-bound launch and one dual
    launch; contracts that carry dividends need cash_dividends="path".  Results:
    mc_policy_batch's dict plus what mc_american_bounds_batch adds (gap,
    gap_stderr, upper, upper_stderr, n_outer, n_inner, sum_gap, sum_gap2,
    dual_min_margin, inner_paths); `brackets` takes them as they are."""
    plans, policies, lo, hi, ids, by_steps = _policy_batches(contracts, policies, cfg,
                                                             subrun_range, stream_ids,
                                                             cash_dividends)
    for c in plans:
        _check_dual_contract(c, cash_dividends)
    _check_dual_sizes(dual.n_outer, dual.n_inner, bool(cfg.antithetic))
    out: List[Optional[dict]] = [
        None if c.fixed_price is None
        else _bounds_result(_policy_result(c, hi - lo, None), dual, None) for c in plans]
    for members in by_steps.values():
        group, pols = [plans[k] for k in members], [policies[k] for k in members]
        kw = dict(engine=engine, seed=cfg.seed, stream_ids=[ids[k] for k in members],
                  subrun_first=lo, cash_dividends=cash_dividends)
        r = simulate_policy(group, pols, hi - lo, cfg.antithetic, **kw)
        d = simulate_policy_dual(group, pols, hi - lo, dual.n_outer, dual.n_inner,
                                 cfg.antithetic, **kw)
        for row, k in enumerate(members):
            out[k] = _bounds_result(_policy_result(plans[k], hi - lo, r["stats"][row]), dual,
                                    d["stats"][row])
    return out  # type: ignore[return-value]


def price_policy_mc_bounds(contract: LsmContract, policy: ExercisePolicy, *, n_subruns: int = 32,
                           antithetic: bool = True, seed: int = 42, stream_id: int = 0,
                           n_outer: int = 8, n_inner: int = 2048, engine: str = "hip",
                           cash_dividends: str = "refuse") -> Dict[str, object]:
    """Lower and upper bound of one contract under `policy`."""
    cfg = LsmConfig(n_subruns=int(n_subruns), antithetic=bool(antithetic), seed=int(seed))
    return mc_policy_bounds_batch([contract], [policy], cfg,
                                  DualConfig(int(n_outer), int(n_inner)), engine=engine,
                                  stream_ids=[stream_id], cash_dividends=cash_dividends)[0]
