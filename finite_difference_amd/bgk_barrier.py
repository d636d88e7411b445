"""Discrete barrier pricer: BGK / Hörfelt closed forms and Monte Carlo paths.

The reference's third barrier pricer family (discrete_barrier_bgk.py), with its
constructor keywords, methods and numbers:

* single and double barriers, in and out, in a Black-76 forward layout with
  the Broadie-Glasserman-Kou shift of the barrier for discrete monitoring;
* Monte Carlo paths for sparse monitoring, with the smoothed barrier test and
  the smoothed payoff, double barriers included;
* ``pricing_method="auto"``: closed form for dense schedules, paths otherwise;
* Greeks from five re-priced scenarios on common random numbers;
* a per-date hazard table and the PV of a rebate paid at the hit.

Everything that is not a path stays on the host, in the reference's operation
order (dates, curves, flat dividend yield, time grid, closed forms).  The
paths run

* ``engine="hip"``: in libfdcn's kernel (csrc/fdcn_mc_bgk.hip).  One launch
  prices B trades x G scenarios; the five scenarios of ``greeks()`` are one
  G = 5 launch that draws every normal once;
* ``engine="host"``: in NumPy, in the reference's order -- the CPU fallback and
  the timed CPU baseline.

A missing GPU under ``engine="hip"`` is an error, never a silent fallback.

Normals (``mc_rng``): ``None`` draws them on the host exactly as the reference
does (torch or NumPy, by ``mc_use_torch_rng``) and hands them to the engine, so
``price()`` reproduces the reference; ``"torch"`` / ``"numpy"`` force one of the
two; ``"philox"`` generates them on the device (include/fdcn.h), stream id
``mc_stream_id`` (0), seed ``mc_seed`` or a random one.

Deviations from the reference: a smoothed barrier with a
rebate at expiry pays ``R * (1 - alive)`` where the reference raises
UnboundLocalError; torch normals come from a local generator, the global
torch RNG state is left alone.
"""
from __future__ import annotations

import datetime as _dt
import math
import secrets
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import capi, market

BETA_BGK = 0.5826  # Broadie-Glasserman-Kou continuity-correction constant
EPS = 1e-12

_OUT_SINGLE = ("up-and-out", "down-and-out")
_IN_SINGLE = ("up-and-in", "down-and-in")
_OUT = _OUT_SINGLE + ("double-out",)
_NO_HAZARD = {"P_hit": 0.0, "survival_to_T": 1.0, "hazard": [], "expected_hit_date": None,
              "mode_hit_date": None, "rebate_pv_at_hit": 0.0}


def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def smooth_relu(x, eps=0.005):
    """Smoothed max(x, 0): 0 below -eps, x above eps, a quadratic between."""
    mid = (0.5 * x**2 + eps * x + 0.5 * eps**2) / (2 * eps)
    if _is_torch(x):
        import torch
        return torch.where(x < -eps, torch.zeros_like(x), torch.where(x > eps, x, mid))
    return np.where(x < -eps, 0.0, np.where(x > eps, x, mid))


def smooth_heaviside_up(x, k, eps=0.01):
    """Smoothed 1{x >= k}: 0 below k - eps, 1 above k + eps, linear between."""
    mid = 0.5 + (x - k) / (2.0 * eps)
    if _is_torch(x):
        import torch
        return torch.where(x < k - eps, torch.zeros_like(x),
                           torch.where(x > k + eps, torch.ones_like(x), mid))
    return np.where(x < k - eps, 0.0, np.where(x > k + eps, 1.0, mid))


def smooth_heaviside_down(x, k, eps=0.01):
    """Smoothed 1{x <= k}: 1 below k - eps, 0 above k + eps, linear between."""
    mid = 0.5 + (k - x) / (2.0 * eps)
    if _is_torch(x):
        import torch
        return torch.where(x < k - eps, torch.ones_like(x),
                           torch.where(x > k + eps, torch.zeros_like(x), mid))
    return np.where(x < k - eps, 1.0, np.where(x > k + eps, 0.0, mid))


def _norm_cdf(x: float) -> float:
    return 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


# ---------------------------------------------------------------------------
# paths
# ---------------------------------------------------------------------------
@dataclass
class PathPlan:
    """One scenario as the path engines take it (include/fdcn.h, fdcn_mc_bgk_*)."""
    params: np.ndarray   # [BGK_NPARAM]
    flags: np.ndarray    # [BGK_NFLAG] int32 (stream id 0; set per launch)
    step: np.ndarray     # [n_steps, BGK_NSTEP]
    df_T: float
    n_half: int          # observations
    antithetic: bool

    @property
    def n_steps(self) -> int:
        return self.step.shape[0]

    @property
    def n_sim(self) -> int:
        return self.n_half * (2 if self.antithetic else 1)

    @property
    def rebate_mode(self) -> int:
        return int(self.flags[capi.BGK_F_REBATE_MODE])


def host_paths(plan: PathPlan, Z: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """x, rebate_pv and alive of each row of Z [n, n_steps] (one path per row)
    in NumPy, with the reference's operations in the reference's order."""
    P, S = plan.params, plan.step
    K, Hu, Hd = (float(P[k]) for k in (capi.BGK_P_STRIKE, capi.BGK_P_UPPER, capi.BGK_P_LOWER))
    eps_b, eps_p = float(P[capi.BGK_P_EPS_BARRIER]), float(P[capi.BGK_P_EPS_PAYOFF])
    R = float(P[capi.BGK_P_REBATE])
    sides, mode = int(plan.flags[capi.BGK_F_SIDES]), plan.rebate_mode
    n = Z.shape[0]
    incs = S[:, capi.BGK_S_DRIFT][None, :] + S[:, capi.BGK_S_DIFF][None, :] * Z
    spots = np.exp(P[capi.BGK_P_LOG_SPOT] + np.cumsum(incs, axis=1))   # spot at each step's end
    breached = np.zeros(n)
    rebate_pv = np.zeros(n)
    for k in range(plan.n_steps):
        if S[k, capi.BGK_S_MONITOR] == 0.0 or sides == 0:
            continue
        s_k = spots[:, k]
        df_k = float(S[k, capi.BGK_S_DF_END])
        if eps_b > 0.0:
            event = np.zeros(n)
            if sides & 1:
                event = np.maximum(event, smooth_heaviside_up(s_k, Hu, eps=eps_b))
            if sides & 2:
                event = np.maximum(event, smooth_heaviside_down(s_k, Hd, eps=eps_b))
            if mode == 2:
                newly = np.maximum(0.0, event - (rebate_pv > 0).astype(float))
                rebate_pv += newly * R * df_k
        else:
            hit = np.zeros(n, dtype=bool)
            if sides & 1:
                hit |= s_k >= Hu
            if sides & 2:
                hit |= s_k <= Hd
            if mode == 2:
                rebate_pv[hit & (breached == 0.0)] = R * df_k
            event = hit.astype(float)
        breached = breached + event
    alive = np.clip(1.0 - breached, 0.0, 1.0)
    s_T = spots[:, -1]
    d = K - s_T if plan.flags[capi.BGK_F_PUT] else s_T - K
    intrinsic = smooth_relu(d, eps=eps_p) if eps_p > 0.0 else np.maximum(d, 0.0)
    x = alive * intrinsic
    if mode == 1:
        x = x + R * (1.0 - alive)
    return x, rebate_pv, alive


def compose(plan: PathPlan, n: int, sum_x: float, sum_x2: float, sum_rebate: float
            ) -> Tuple[float, float]:
    """Price and standard error of n paths from their raw sums: the reference's
    estimator (ddof = 1; the rebate-at-hit mean is added outside the
    discounting)."""
    nf = float(n)
    price = plan.df_T * (sum_x / nf)
    if plan.rebate_mode == 2:
        price = price + sum_rebate / nf
    if n < 2:
        return price, float("nan")
    var = max(0.0, (sum_x2 - sum_x * sum_x / nf) / (nf - 1.0))
    return price, math.sqrt(var) * plan.df_T / math.sqrt(nf)


def _compose_arrays(plan: PathPlan, x: np.ndarray, rebate_pv: np.ndarray) -> Tuple[float, float]:
    """compose() on the per-path arrays, with the reference's np.mean / np.std."""
    price = plan.df_T * float(np.mean(x))
    if plan.rebate_mode == 2:
        price = price + float(np.mean(rebate_pv))
    with np.errstate(all="ignore"):
        se = np.std(x, ddof=1) * plan.df_T / math.sqrt(x.shape[0]) if x.shape[0] > 1 else np.nan
    return price, float(se)


def draw_normals(kind: str, seed: Optional[int], n_half: int, n_steps: int) -> np.ndarray:
    """z [n_half, n_steps] as the reference draws them: "torch" =
    torch.randn(..., dtype=float64) after manual_seed(seed), on a local
    generator; "numpy" = default_rng(seed).standard_normal."""
    if kind == "torch":
        import torch
        g = torch.Generator()
        if seed is not None:
            g.manual_seed(int(seed))
        else:
            g.seed()
        return torch.randn(n_half, n_steps, dtype=torch.float64, generator=g).numpy()
    if kind == "numpy":
        return np.random.default_rng(seed).standard_normal((n_half, n_steps))
    raise ValueError("mc_rng must be None, 'philox', 'numpy' or 'torch'")


def run_paths(groups: Sequence[Sequence[PathPlan]], *, engine: str = "hip", z=None, seed: int = 0,
              stream_ids: Optional[Sequence[int]] = None, obs_first: int = 0,
              n_obs: Optional[int] = None, want_payoffs: bool = False):
    """One launch: B trades x G scenarios (groups[b][g]) that share n_steps,
    the observation count, the antithetic switch and G.  Returns stats
    [B, G, 4] = sum x, sum x^2, sum rebate_pv, sum (1 - alive) over the paths
    (and payoffs [B, G, 2, n_sim] with want_payoffs).  Normals: `z`
    [n_obs, n_steps] shared by the launch, else the Philox stream
    (seed, stream id) from observation obs_first."""
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    B, G = len(groups), len(groups[0])
    first = groups[0][0]
    n_steps, anti = first.n_steps, first.antithetic
    n_obs = first.n_half if n_obs is None else int(n_obs)
    if not 1 <= G <= capi.BGK_MAX_G:
        raise ValueError(f"run_paths: G must be in 1 .. {capi.BGK_MAX_G}")
    for grp in groups:
        if len(grp) != G or any(p.n_steps != n_steps or p.antithetic != anti for p in grp):
            raise ValueError("run_paths: the trades of a launch share n_steps, antithetic and G")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError("run_paths: one stream id per trade")
    Z = None
    if z is not None:
        Z = np.ascontiguousarray(z, dtype=np.float64)
        if Z.shape != (n_obs, n_steps):
            raise ValueError(f"run_paths: z must be [n_obs, n_steps] = {(n_obs, n_steps)}")
    if engine == "hip":
        capi.require_device()
        P = np.stack([np.stack([p.params for p in grp]) for grp in groups])
        S = np.stack([np.stack([p.step for p in grp]) for grp in groups])
        F = np.stack([grp[0].flags for grp in groups]).astype(np.int32)
        F[:, capi.BGK_F_STREAM] = np.asarray(ids, dtype=np.int32)
        return capi.mc_bgk_batch(P, F, S, n_obs, anti, z=Z, seed=seed, obs_first=obs_first,
                                 want_payoffs=want_payoffs)
    from .mc_barrier import philox_normals
    n_sim = n_obs * (2 if anti else 1)
    stats = np.zeros((B, G, capi.BGK_NSTAT))
    pay = np.empty((B, G, 2, n_sim)) if want_payoffs else None
    for b, grp in enumerate(groups):
        Zb = Z if Z is not None else philox_normals(n_obs, n_steps, seed, ids[b], obs_first)
        if anti:
            Zb = np.concatenate([Zb, -Zb], axis=0)
        for g, plan in enumerate(grp):
            x, rp, alive = host_paths(plan, Zb)
            stats[b, g] = (np.sum(x), np.sum(x * x), np.sum(rp), np.sum(1.0 - alive))
            if want_payoffs:
                pay[b, g, 0], pay[b, g, 1] = x, rp
    return (stats, pay) if want_payoffs else stats


@dataclass
class _Job:
    """A scenario's raw (unscaled) price: known on the host (`value`), or
    `base + sign * (path price of plan)`."""
    value: Optional[float] = None
    plan: Optional[PathPlan] = None
    base: float = 0.0
    sign: float = 1.0
    sums: Optional[Tuple[float, ...]] = None   # the launch's raw sums of this scenario
    n_sim: int = 0


class DiscreteBarrierBGKPricer:
    """Discrete barrier option pricer (BGK / Hörfelt closed forms, Monte Carlo
    paths) in a Black-76 forward layout: the reference's class, see the module
    docstring for `engine` and `mc_rng`."""

    def __init__(
        self,
        *,
        spot: float,
        strike: float,
        valuation_date: _dt.date,
        maturity_date: _dt.date,
        option_type: str,
        barrier_type: str = "none",
        lower_barrier: Optional[float] = None,
        upper_barrier: Optional[float] = None,
        monitor_dates: Optional[List[_dt.date]] = None,
        rebate_amount: float = 0.0,
        rebate_at_hit: bool = False,
        already_hit: bool = False,
        barrier_hit_date: Optional[_dt.date] = None,
        discount_curve=None,
        forward_curve=None,
        dividend_schedule: Optional[List[Tuple[_dt.date, float]]] = None,
        volatility: float = 0.2,
        day_count: str = "ACT/365",
        include_expiry_monitor: bool = True,
        use_mean_sqrt_dt: bool = False,
        theta_from_forward: bool = False,
        pricing_method: str = "auto",
        bgk_min_freq: float = 20.0,
        mc_n_paths: int = 4096,
        mc_seed: Optional[int] = 42,
        mc_use_antithetic: bool = True,
        mc_use_torch_rng: bool = True,
        mc_smooth_barrier_eps: float = 0.01,
        mc_smooth_payoff_eps: float = 0.005,
        underlying_spot_days: int = 0,
        option_days: int = 0,
        option_settlement_days: int = 0,
        trade_id: str = "T-0001",
        direction: str = "long",
        quantity: int = 1,
        contract_multiplier: float = 1.0,
        engine: str = "hip",
        mc_rng: Optional[str] = None,
    ) -> None:
        if spot <= 0 or strike <= 0 or volatility <= 0:
            raise ValueError("spot, strike, volatility must be positive.")
        if maturity_date <= valuation_date:
            raise ValueError("maturity_date must be after valuation_date.")
        if engine not in ("hip", "host"):
            raise ValueError("engine must be 'hip' or 'host'")
        if mc_rng not in (None, "philox", "numpy", "torch"):
            raise ValueError("mc_rng must be None, 'philox', 'numpy' or 'torch'")
        self.engine = engine
        self.mc_rng = mc_rng
        self.mc_stream_id = 0

        self.spot_price = float(spot)
        self.strike_price = float(strike)
        self.valuation_date = valuation_date
        self.maturity_date = maturity_date
        self.option_type = option_type
        self.barrier_type = barrier_type
        self.lower_barrier = lower_barrier
        self.upper_barrier = upper_barrier
        self.monitor_dates = sorted(monitor_dates or [])
        self.rebate_amount = float(rebate_amount)
        self.rebate_at_hit = bool(rebate_at_hit)
        self.already_hit = bool(already_hit)
        self.barrier_hit_date = barrier_hit_date
        self.discount_curve_df = discount_curve.copy() if discount_curve is not None else None
        self.forward_curve_df = forward_curve.copy() if forward_curve is not None else None
        self.dividend_schedule = sorted(dividend_schedule or [], key=lambda x: x[0])
        self.sigma = float(volatility)
        self.day_count = day_count.upper()
        self._year_denominator = self._infer_denominator(self.day_count)
        self.underlying_spot_days = int(underlying_spot_days)
        self.option_days = int(option_days)
        self.option_settlement_days = int(option_settlement_days)
        self.include_expiry_monitor = include_expiry_monitor
        self.use_mean_sqrt_dt = use_mean_sqrt_dt
        self.theta_from_forward = theta_from_forward
        self.pricing_method = pricing_method
        self.bgk_min_freq = float(bgk_min_freq)
        self.mc_n_paths = int(mc_n_paths)
        self.mc_seed = mc_seed
        self.mc_use_antithetic = bool(mc_use_antithetic)
        self.mc_use_torch_rng = bool(mc_use_torch_rng)
        self.mc_smooth_barrier_eps = float(mc_smooth_barrier_eps)
        self.mc_smooth_payoff_eps = float(mc_smooth_payoff_eps)
        self._last_mc_std_error: float = 0.0
        self._last_mc_sums: Optional[Tuple[float, float, float, float]] = None
        self.trade_id = trade_id
        self.direction = direction
        self.quantity = int(quantity)
        self.contract_multiplier = float(contract_multiplier)

        # settlement windows: carry (spot lag) and discounting (option lags)
        self.carry_start_date = self.discount_start_date = valuation_date
        self.carry_end_date = self.discount_end_date = maturity_date
        if self.underlying_spot_days > 0 or self.option_days > 0 or self.option_settlement_days > 0:
            cal = market.SouthAfrica()
            self.carry_start_date = cal.add_working_days(valuation_date, self.underlying_spot_days)
            self.carry_end_date = cal.add_working_days(maturity_date, self.underlying_spot_days)
            self.discount_start_date = cal.add_working_days(valuation_date, self.option_days)
            self.discount_end_date = cal.add_working_days(maturity_date,
                                                          self.option_settlement_days)
        self.time_to_expiry = self._year_fraction(valuation_date, maturity_date)
        self.time_to_carry = self._year_fraction(self.carry_start_date, self.carry_end_date)
        self.time_to_discount = self._year_fraction(self.discount_start_date,
                                                    self.discount_end_date)
        self.tenor_years = self.time_to_expiry
        self.discount_years = self.time_to_discount

        self.discount_rate_nacc = (
            self.get_forward_nacc_rate(self.discount_start_date, self.discount_end_date)
            if self.discount_curve_df is not None else 0.0)
        self.discount_rate = self.discount_rate_nacc
        carry_curve = (self.forward_curve_df if self.forward_curve_df is not None
                       else self.discount_curve_df)
        self.carry_rate_nacc = (
            self.get_forward_nacc_rate(self.carry_start_date, self.carry_end_date,
                                       curve_df=carry_curve)
            if carry_curve is not None else self.discount_rate_nacc)
        self.div_yield_nacc = self._dividend_yield_nacc()
        self._refresh_for_spot_change()
        self._dt_years = self._compute_dt_years_from_schedule()
        self.m = len(self._dt_years) if self._dt_years is not None else self._heuristic_m()

    # ------------------------------------------------------------------ API
    def price(self) -> float:
        """Total price including the rebate leg (if any)."""
        return self._signed_scale(self._settle([self._job()])[0])

    def greeks(self, ds_rel: float = 1e-4, dvol_abs: float = 1e-4) -> Dict[str, float]:
        """Finite-difference Greeks under the spot convention: five re-priced
        scenarios (S + dS, S - dS, base, sigma + dsigma, sigma - dsigma).  In
        Monte Carlo mode they are one launch on common random numbers."""
        ds = max(1e-8, ds_rel * self.spot_price)
        jobs = self._bumped_jobs(ds, dvol_abs)
        # every scenario is priced as a long position; quantity and multiplier
        # enter there and once more in the final scale, as in the reference
        unit = self.quantity * self.contract_multiplier
        up, dn, base, upv, dnv = (1.0 * unit * float(px) for px in self._settle(jobs))
        delta = (up - dn) / (2 * ds)
        gamma = (up - 2 * base + dn) / (ds * ds)
        vega = (upv - dnv) / (2 * dvol_abs)
        scale = (1.0 if self.direction == "long" else -1.0) * self.quantity \
            * self.contract_multiplier
        return {"delta": scale * delta, "gamma": scale * gamma, "vega": scale * vega}

    def _bumped_jobs(self, ds: float, dvol: float) -> List[_Job]:
        """The jobs of the five Greeks scenarios, in the reference's pricing
        order: S + dS, S - dS, base, sigma + dsigma, sigma - dsigma."""
        s0, sig0 = self.spot_price, self.sigma
        jobs = []
        try:
            for spot, sig in ((s0 + ds, sig0), (s0 - ds, sig0), (s0, sig0), (s0, sig0 + dvol),
                              (s0, sig0 - dvol)):
                self.spot_price, self.sigma = spot, sig
                self._refresh_for_spot_change()
                jobs.append(self._job())
        finally:
            self.spot_price, self.sigma = s0, sig0
            self._refresh_for_spot_change()
        return jobs

    def report(self) -> str:
        """Model summary and a concise barrier-hit summary."""
        sel = self._select_method()
        dash = "-"
        L = [
            "==== Discrete Barrier (BGK/Hörfelt) — Black-76 layout ====",
            f"Trade ID           : {self.trade_id}",
            f"Direction          : {self.direction}",
            f"Quantity           : {self.quantity}",
            f"Contract Multiplier: {self.contract_multiplier:.6g}",
            f"Option Type        : {self.option_type}",
            f"Barrier Type       : {self.barrier_type}",
            f"Lower Barrier (Hd) : {self.lower_barrier if self.lower_barrier is not None else dash}",
            f"Upper Barrier (Hu) : {self.upper_barrier if self.upper_barrier is not None else dash}",
            f"Spot (S0)          : {self.spot_price:.8f}",
            f"Strike (K)         : {self.strike_price:.8f}",
            f"Valuation Date     : {self.valuation_date.isoformat()}",
            f"Maturity Date      : {self.maturity_date.isoformat()}",
            f"Day Count          : {self.day_count}",
            f"Spot lag (carry)   : {self.underlying_spot_days}bd  "
            f"({self.carry_start_date.isoformat()} -> {self.carry_end_date.isoformat()})",
            f"Settlement (disc)  : {self.option_days}bd start / "
            f"{self.option_settlement_days}bd end  "
            f"({self.discount_start_date.isoformat()} -> {self.discount_end_date.isoformat()})",
            f"T expiry (years)   : {self.time_to_expiry:.8f}",
            f"T carry (years)    : {self.time_to_carry:.8f}",
            f"T discount (years) : {self.time_to_discount:.8f}",
            f"Volatility (sigma) : {self.sigma:.8f}",
            f"Discount r (NACC)  : {self.discount_rate_nacc:.8f}  (fwd over discount window)",
            f"Carry r (NACC)     : {self.carry_rate_nacc:.8f}  (fwd over carry window)",
            f"Dividend y (q)     : {self.div_yield_nacc:.8f}",
            f"F0 (forward)       : {self.forward_price:.8f}",
            f"m (monitors)       : {self.m}",
            f"include_expiry_mon : {self.include_expiry_monitor}",
            f"use_mean_sqrt_dt   : {self.use_mean_sqrt_dt}",
            f"theta_from_forward : {self.theta_from_forward}",
            f"pricing_method     : {self.pricing_method}  →  selected: {sel.upper()}",
            f"bgk_min_freq       : {self.bgk_min_freq:.1f} dates/yr  "
            f"(mon freq = {self.m / max(self.tenor_years, EPS):.1f}/yr)",
        ]
        if sel == "mc":
            style = lambda e: "RISKFLOW-style" if e > 0 else "exact"  # noqa: E731
            L += [
                f"mc_n_paths         : {self.mc_n_paths:,}",
                f"mc_seed            : {self.mc_seed}",
                f"mc_use_antithetic  : {self.mc_use_antithetic}",
                f"mc_use_torch_rng   : {self.mc_use_torch_rng}",
                f"mc_smooth_barrier  : ε={self.mc_smooth_barrier_eps:.4f} "
                f"({style(self.mc_smooth_barrier_eps)})",
                f"mc_smooth_payoff   : ε={self.mc_smooth_payoff_eps:.4f} "
                f"({style(self.mc_smooth_payoff_eps)})",
            ]
        L.append("----------------------------------------")
        px = self.price()
        gk = self.greeks()
        L.append(f"Price              : {px:.10f}")
        if sel == "mc":
            L.append(f"MC std error       : {self._last_mc_std_error:.2e}")
        L += [f"Delta              : {gk['delta']:.10f}",
              f"Gamma              : {gk['gamma']:.10f}",
              f"Vega               : {gk['vega']:.10f}"]
        try:
            mets = self.barrier_hit_metrics()
            L.append("---- Barrier hit summary ----")
            if mets.get("hazard"):
                L += self._hazard_head(mets)[:3]
                for d, p, DF, contrib in sorted(mets["hazard"], key=lambda h: h[1],
                                                reverse=True)[:3]:
                    L.append(f"  {d.isoformat()}: p={p:.4%}, DF={DF:.6f}, "
                             f"rebate PV contrib={contrib:.6f}")
                L.append(self._hazard_head(mets)[3])
            else:
                L.append("No schedule/single barrier not set: hazard summary not available.")
        except Exception as e:  # the report survives a failing summary, as the reference's
            L.append(f"(hazard summary unavailable: {e})")
        return "\n".join(L)

    @staticmethod
    def _hazard_head(mets) -> List[str]:
        return [f"P(hit by last monitor): {mets['P_hit']:.6%}",
                f"Expected hit date     : {mets['expected_hit_date'] or '-'}",
                f"Mode hit date         : {mets['mode_hit_date'] or '-'}",
                f"Rebate PV at hit (expected): {mets['rebate_pv_at_hit']:.6f}"]

    def report_hazard_table(self, max_rows: int = 20) -> str:
        """The per-date hazard table."""
        mets = self.barrier_hit_metrics()
        L = ["=== Barrier hit hazard table ==="]
        if not mets.get("hazard"):
            L.append("No hazard entries (no schedule or not a single barrier).")
            return "\n".join(L)
        L += self._hazard_head(mets)
        L += ["", f"{'Date':<12} {'p_i':>10} {'DF_i':>12} {'PV contrib':>14}", "-" * 52]
        for i, (d, p, DF, contrib) in enumerate(mets["hazard"]):
            if i >= max_rows:
                L.append(f"... ({len(mets['hazard'])-max_rows} more rows)")
                break
            L.append(f"{d.isoformat():<12} {p:>9.4%} {DF:>12.6f} {contrib:>14.6f}")
        return "\n".join(L)

    # ------------------------------------------------- curves, dividends, time
    def _df_from_curve(self, curve, date: _dt.date) -> float:
        """Discount factor to `date` from a ('date','df') table (last row at or
        before the date) or a ('Date','NACA') table (the date's row, else the
        nearest prior one); column names in any case.  No curve: 1.0."""
        import pandas as pd
        if curve is None or curve.empty:
            return 1.0
        col = {c.lower(): c for c in curve.columns}
        if "date" in col and "df" in col:
            days = pd.to_datetime(curve[col["date"]]).dt.date
            keep = days <= date
            row = curve[keep].tail(1) if keep.any() else curve.head(1)
            return float(row[col["df"]].values[0])
        if "date" in col and "naca" in col:
            days = pd.to_datetime(curve[col["date"]]).dt.date
            keep = days == date
            if not keep.any():
                keep = days < date
            row = curve[keep].tail(1) if keep.any() else curve.head(1)
            naca = float(row[col["naca"]].values[0])
            return (1.0 + naca) ** (-self._year_fraction(self.valuation_date, date))
        raise ValueError("Curve must have ('date','df') or ('Date','NACA').")

    def get_discount_factor(self, lookup_date: _dt.date, curve_df=None) -> float:
        """Discount factor from valuation_date to lookup_date."""
        return self._df_from_curve(curve_df if curve_df is not None else self.discount_curve_df,
                                   lookup_date)

    def get_forward_nacc_rate(self, start_date: _dt.date, end_date: _dt.date,
                              curve_df=None) -> float:
        """-ln(DF(end) / DF(start)) / tau(start, end)."""
        df_far = self.get_discount_factor(end_date, curve_df)
        df_near = self.get_discount_factor(start_date, curve_df)
        tau = self._year_fraction(start_date, end_date)
        if tau <= EPS:
            return 0.0
        return -math.log(max(df_far / max(df_near, 1e-16), 1e-16)) / tau

    def _pv_dividends(self) -> float:
        pv = 0.0
        for pay_date, amt in self.dividend_schedule:
            if self.valuation_date < pay_date <= self.maturity_date:
                pv += float(amt) * self.get_discount_factor(pay_date)
        return pv

    def _dividend_yield_nacc(self) -> float:
        """Flat q with S0 * exp(-q T) = S0 - PV(dividends)."""
        pv = self._pv_dividends()
        if pv <= 0.0:
            return 0.0
        if pv >= self.spot_price:
            return 50.0
        return -math.log((self.spot_price - pv) / self.spot_price) / max(self.tenor_years, EPS)

    @staticmethod
    def _infer_denominator(day_count: str) -> int:
        return {"ACT/360": 360, "ACT/364": 364, "30/360": 360, "30E/360": 360, "BOND": 360,
                "US30/360": 360}.get(day_count, 365)

    def _year_fraction(self, d0: _dt.date, d1: _dt.date) -> float:
        if d1 <= d0:
            return 0.0
        if self.day_count in ("ACT/365", "ACT/365F", "ACT/360", "ACT/364"):
            return (d1 - d0).days / float(self._year_denominator)
        if self.day_count in ("30/360", "30E/360", "BOND", "US30/360"):
            dd0 = min(d0.day, 30)
            dd1 = min(d1.day, 30) if dd0 == 30 else d1.day
            return ((d1.year - d0.year) * 360 + (d1.month - d0.month) * 30 + (dd1 - dd0)) / 360.0
        return (d1 - d0).days / 365.0

    def _monitors_in_life(self) -> List[_dt.date]:
        if self.include_expiry_monitor:
            return [d for d in self.monitor_dates if self.valuation_date < d <= self.maturity_date]
        return [d for d in self.monitor_dates if self.valuation_date < d < self.maturity_date]

    def _compute_dt_years_from_schedule(self) -> Optional[List[float]]:
        prev, dts = self.valuation_date, []
        for d in sorted(self._monitors_in_life()):
            dt = self._year_fraction(prev, d)
            if dt > 0:
                dts.append(dt)
                prev = d
        return dts or None

    def _heuristic_m(self) -> int:
        """Without a schedule: daily for puts, about weekly for calls."""
        if self.option_type == "put":
            return max(1, int(round(252 * self.tenor_years)))
        return max(1, int(round(252 * self.tenor_years) / 5))

    def _refresh_for_spot_change(self) -> None:
        self.spot_price_eff = self.spot_price * math.exp(-self.div_yield_nacc * self.time_to_carry)
        self.forward_price = self.spot_price_eff * math.exp(self.carry_rate_nacc
                                                            * self.time_to_carry)

    def _signed_scale(self, px: float) -> float:
        sgn = 1.0 if self.direction == "long" else -1.0
        return sgn * self.quantity * self.contract_multiplier * float(px)

    def _df_T(self) -> float:
        return math.exp(-self.discount_rate * self.discount_years)

    # ------------------------------------------------------------ closed forms
    def _vanilla_b76(self) -> float:
        T, sig, K = self.tenor_years, self.sigma, self.strike_price
        if T <= 0.0 or sig <= 0.0:
            return max(self.spot_price - K, 0.0) if self.option_type == "call" \
                else max(K - self.spot_price, 0.0)
        DF = self._df_T()
        F0 = self.forward_price
        st = sig * math.sqrt(T)
        d1 = (math.log(F0 / K) + 0.5 * sig * sig * T) / st
        d2 = d1 - st
        if self.option_type == "call":
            return DF * (F0 * _norm_cdf(d1) - K * _norm_cdf(d2))
        return DF * (K * _norm_cdf(-d2) - F0 * _norm_cdf(-d1))

    def _phi_at(self, x: float, T: float) -> float:
        return math.log(max(x, EPS) / self.spot_price_eff) / (self.sigma * math.sqrt(max(T, EPS)))

    def _phi(self, x: float) -> float:
        return self._phi_at(x, self.tenor_years)

    def _thetas_at(self, T: float) -> Tuple[float, float]:
        sqrtT = math.sqrt(max(T, EPS))
        if self.theta_from_forward:
            mu = math.log(self.forward_price / self.spot_price_eff) / max(self.time_to_carry, EPS)
        else:
            mu = (self.carry_rate_nacc - self.div_yield_nacc)
        theta0 = (mu - 0.5 * self.sigma * self.sigma) * sqrtT / self.sigma
        return theta0, theta0 + self.sigma * sqrtT

    def _theta0_theta1(self) -> Tuple[float, float]:
        return self._thetas_at(self.tenor_years)

    def _F_plus(self, a: float, b: float, theta: float) -> float:
        """Up-barrier block, a clamped to a <= b."""
        if b <= 0.0:
            return 0.0
        a = a if a <= b else b
        return _norm_cdf(a - theta) - math.exp(2.0 * b * theta) * _norm_cdf(a - 2.0 * b - theta)

    def _F_minus(self, a: float, b: float, theta: float) -> float:
        """Down-barrier block, a clamped to a >= b: the mirror of _F_plus."""
        if b >= 0.0:
            return 0.0
        a = a if a >= b else b
        return self._F_plus(-a, -b, -theta)

    def _shift_magnitude(self, dts: Optional[List[float]], T: float, m: int) -> float:
        if self.use_mean_sqrt_dt and dts:
            mean_sqrt_dt = sum(math.sqrt(dt) for dt in dts) / len(dts)
            return (BETA_BGK * mean_sqrt_dt) / math.sqrt(max(T, EPS))
        return BETA_BGK / math.sqrt(m)

    def _bgk_phi_shift(self, side: str, d_phi: float) -> float:
        if self.m <= 0:
            return d_phi
        sign = +1.0 if side == "up" else -1.0
        return d_phi + sign * self._shift_magnitude(self._dt_years, self.tenor_years, self.m)

    def _bgk_phi_shift_at(self, side: str, d_phi: float, T: float, m_t: int) -> float:
        if m_t <= 0:
            return d_phi
        sign = +1.0 if side == "up" else -1.0
        dts = self._dt_years[:m_t] if self._dt_years else None
        return d_phi + sign * self._shift_magnitude(dts, T, m_t)

    def _select_method(self) -> str:
        """"bgk" or "mc": under "auto", the closed form when the schedule has
        at least bgk_min_freq dates a year, paths otherwise."""
        if self.pricing_method in ("bgk", "mc"):
            return self.pricing_method
        if self.m <= 0:
            return "bgk"
        return "bgk" if self.m / max(self.tenor_years, EPS) >= self.bgk_min_freq else "mc"

    def _single_barrier_out_price(self, side: str) -> float:
        if self.m <= 0:
            return self._vanilla_b76()
        H = self.upper_barrier if side == "up" else self.lower_barrier
        if H is None or (self.spot_price >= H if side == "up" else self.spot_price <= H):
            return 0.0
        th0, th1 = self._theta0_theta1()
        K = self.strike_price
        c = self._phi(K)
        DF = self._df_T()
        F0 = self.forward_price
        d = self._phi(H)
        b = self._bgk_phi_shift(side, d)
        if side == "up":
            Fp = self._F_plus
            if self.option_type == "call":
                if K >= H:
                    return 0.0
                return DF * (F0 * (Fp(d, b, th1) - Fp(c, b, th1))
                             - K * (Fp(d, b, th0) - Fp(c, b, th0)))
            return DF * (K * Fp(c, b, th0) - F0 * Fp(c, b, th1))
        Fm = self._F_minus
        if self.option_type == "put":
            if K <= H:
                return 0.0
            return DF * (K * (Fm(d, b, th0) - Fm(c, b, th0))
                         - F0 * (Fm(d, b, th1) - Fm(c, b, th1)))
        return DF * (F0 * Fm(c, b, th1) - K * Fm(c, b, th0))

    def _G_continuous(self, a1: float, a2: float, b1: float, b2: float, theta: float,
                      series_terms: int = 50) -> float:
        """Image series of the double-barrier survival block."""
        N = _norm_cdf
        total = N(a2 - theta) - N(a1 - theta)
        width = (b2 - b1)
        for k in range(1, series_terms + 1):
            shift = 2.0 * k * width
            total += (N(a2 - theta - shift) - N(a1 - theta - shift))
            total -= (N(a2 - theta + shift) - N(a1 - theta + shift))
        return total

    def _double_barrier_out_price(self, series_terms: int = 50) -> float:
        if self.m <= 0 or (self.lower_barrier is None and self.upper_barrier is None):
            return self._vanilla_b76()
        if self.lower_barrier is None or self.upper_barrier is None:
            raise ValueError("Double barrier requires both lower_barrier and upper_barrier.")
        d1 = self._phi(self.lower_barrier)
        d2 = self._phi(self.upper_barrier)
        c = self._phi(self.strike_price)
        th0, th1 = self._theta0_theta1()
        shift = self._shift_magnitude(self._dt_years, self.tenor_years, self.m)
        b1, b2 = d1 - shift, d2 + shift

        def G(a1, a2, th):
            return self._G_continuous(a1, a2, b1, b2, th, series_terms=series_terms)
        DF = self._df_T()
        F0, K = self.forward_price, self.strike_price
        if self.option_type == "call":
            if K >= self.upper_barrier:
                return 0.0
            a1, a2 = max(c, d1), d2
            return DF * (F0 * G(a1, a2, th1) - K * G(a1, a2, th0))
        if K <= self.lower_barrier:
            return 0.0
        a1, a2 = d1, min(c, d2)
        return DF * (K * G(a1, a2, th0) - F0 * G(a1, a2, th1))

    def _survival_prob_to(self, side: str, T: float, m_t: int) -> float:
        """Survival to the sub-horizon T with its first m_t monitors."""
        th0, _ = self._thetas_at(T)
        if side == "up":
            b = self._bgk_phi_shift_at("up", self._phi_at(self.upper_barrier, T), T, m_t)
            return self._F_plus(b, b, th0)
        b = self._bgk_phi_shift_at("down", self._phi_at(self.lower_barrier, T), T, m_t)
        return self._F_minus(b, b, th0)

    def barrier_hit_metrics(self) -> Dict[str, Any]:
        """Per-date hazard (date, p_i, DF_i, PV contribution), P_hit, survival
        to the last monitor, expected and mode hit dates, PV of a rebate at
        hit.  Single barriers with a schedule only."""
        mons = self._monitors_in_life()
        if (self.barrier_type not in _OUT_SINGLE + _IN_SINGLE or not self._dt_years or not mons):
            return dict(_NO_HAZARD, hazard=[])
        side = "up" if "up" in self.barrier_type else "down"
        horizons, acc = [], 0.0
        for dt in self._dt_years:
            acc += dt
            horizons.append(acc)
        hazards, surv, p_hit, pv = [], 1.0, 0.0, 0.0
        for k, (T_k, d_k) in enumerate(zip(horizons, mons), start=1):
            s_k = self._survival_prob_to(side, T_k, k)
            p_k = max(0.0, surv - s_k)
            DF_k = self.get_discount_factor(d_k)
            contrib = self.rebate_amount * DF_k * p_k
            hazards.append((d_k, p_k, DF_k, contrib))
            pv += contrib
            p_hit += p_k
            surv = s_k
        expected = mode = None
        if p_hit > 0.0:
            weights = [h[1] / p_hit for h in hazards]
            mean_ord = sum(w * h[0].toordinal() for w, h in zip(weights, hazards))
            expected = _dt.date.fromordinal(int(round(mean_ord)))
            mode = max(hazards, key=lambda h: h[1])[0]
        return {"P_hit": float(p_hit), "survival_to_T": float(surv), "hazard": hazards,
                "expected_hit_date": expected, "mode_hit_date": mode,
                "rebate_pv_at_hit": float(pv)}

    def _hit_date_df(self) -> float:
        return self._df_from_curve(self.discount_curve_df,
                                   self.barrier_hit_date or self.valuation_date)

    def _rebate_leg(self) -> float:
        """PV of the rebate leg of the closed-form out styles."""
        if self.rebate_amount <= 0.0 or self.barrier_type not in _OUT:
            return 0.0
        if not self.rebate_at_hit:
            return self.rebate_amount * self._df_T()
        if self.already_hit:
            return self.rebate_amount * self._hit_date_df()
        return self.barrier_hit_metrics()["rebate_pv_at_hit"]

    def _bgk_raw(self) -> float:
        bt = self.barrier_type
        if bt in _OUT_SINGLE:
            return self._single_barrier_out_price("up" if "up" in bt else "down") \
                + self._rebate_leg()
        if bt in _IN_SINGLE:
            px_out = self._single_barrier_out_price("up" if "up" in bt else "down")
            return self._vanilla_b76() - px_out
        if bt == "double-out":
            return self._double_barrier_out_price() + self._rebate_leg()
        if bt == "double-in":
            px_out = self._double_barrier_out_price()
            return self._vanilla_b76() - px_out
        raise ValueError(f"Unsupported barrier_type: {bt}")

    # ------------------------------------------------------------------ paths
    def _mc_monitoring_times(self) -> List[float]:
        """Cumulative monitoring times in years from the valuation date."""
        if self._dt_years:
            acc, times = 0.0, []
            for dt in self._dt_years:
                acc += dt
                times.append(round(acc, 12))
            return times
        T, m = self.tenor_years, max(1, self.m)
        return [round(T * k / m, 12) for k in range(1, m + 1)]

    def _path_plan(self, btype: str) -> PathPlan:
        """The per-step table and parameters of the out-style `btype` under the
        current spot and sigma (the reference's grid, :696-772)."""
        T = self.tenor_years
        mon_times = self._mc_monitoring_times()
        raw = [0.0] + mon_times
        if not mon_times or abs(mon_times[-1] - T) > 1e-10:
            raw.append(T)
        points = sorted(set(round(t, 10) for t in raw))
        monitored = {round(t, 10) for t in mon_times}
        dts = np.diff(points)
        n_steps = len(dts)
        mu = self.carry_rate_nacc - self.div_yield_nacc
        sig = self.sigma
        df_T = self._df_T()
        mode = 0
        if self.rebate_amount > 0.0:
            mode = 2 if self.rebate_at_hit else 1
        step = np.empty((n_steps, capi.BGK_NSTEP))
        step[:, capi.BGK_S_DRIFT] = (mu - 0.5 * sig * sig) * dts
        step[:, capi.BGK_S_DIFF] = sig * np.sqrt(np.maximum(dts, 0.0))
        for k in range(n_steps):
            tp = points[k + 1]
            is_mon = round(tp, 10) in monitored
            step[k, capi.BGK_S_MONITOR] = 1.0 if is_mon else 0.0
            step[k, capi.BGK_S_DF_END] = (math.exp(-self.discount_rate * tp)
                                          if is_mon and mode == 2 else df_T)
        Hu, Hd = self.upper_barrier, self.lower_barrier
        sides = ((1 if btype in ("up-and-out", "double-out") and Hu is not None else 0)
                 | (2 if btype in ("down-and-out", "double-out") and Hd is not None else 0))
        params = np.array([float(np.log(self.spot_price)), self.strike_price,
                           float(Hu) if sides & 1 else 0.0, float(Hd) if sides & 2 else 0.0,
                           self.mc_smooth_barrier_eps if self.mc_smooth_barrier_eps > 0.0 else 0.0,
                           self.mc_smooth_payoff_eps if self.mc_smooth_payoff_eps > 0.0 else 0.0,
                           self.rebate_amount], dtype=float)
        flags = np.array([self.option_type != "call", sides, mode, 0], dtype=np.int32)
        n_half = max(1, self.mc_n_paths // 2) if self.mc_use_antithetic else self.mc_n_paths
        return PathPlan(params=params, flags=flags, step=step, df_T=df_T, n_half=int(n_half),
                        antithetic=self.mc_use_antithetic)

    def _mc_job(self) -> _Job:
        """Route the barrier type to paths, with the reference's short-circuits."""
        bt = self.barrier_type
        if bt in ("up-and-out", "double-out"):
            if self.upper_barrier is not None and self.spot_price >= self.upper_barrier:
                return _Job(value=0.0)
        if bt in ("down-and-out", "double-out"):
            if self.lower_barrier is not None and self.spot_price <= self.lower_barrier:
                return _Job(value=0.0)
        if self.already_hit:
            return _Job(value=self.rebate_amount * self._hit_date_df()
                        if self.rebate_amount > 0.0 else 0.0)
        if bt in _OUT:
            return _Job(plan=self._path_plan(bt))
        if bt in _IN_SINGLE:   # in = vanilla - out of the same direction
            out_type = "up-and-out" if "up" in bt else "down-and-out"
            return _Job(plan=self._path_plan(out_type), base=self._vanilla_b76(), sign=-1.0)
        if bt == "double-in":
            return _Job(plan=self._path_plan("double-out"), base=self._vanilla_b76(), sign=-1.0)
        raise ValueError(f"Unsupported barrier_type for MC: {bt}")

    def _job(self) -> _Job:
        """The raw price under the current spot and sigma, or its path job."""
        if self.barrier_type == "none":
            return _Job(value=self._vanilla_b76())
        if self._select_method() == "mc":
            return self._mc_job()
        return _Job(value=self._bgk_raw())

    def _rng_kind(self) -> str:
        if self.mc_rng is not None:
            return self.mc_rng
        return "torch" if self.mc_use_torch_rng else "numpy"

    def _settle(self, jobs: List[_Job], obs_range: Optional[range] = None) -> List[float]:
        """Raw prices of the jobs; those with paths run as one launch."""
        todo = [j for j in jobs if j.plan is not None]
        if todo:
            _run_groups([(self, todo)], self.engine, self._rng_kind(), [self.mc_stream_id],
                        obs_range)
        return [j.value for j in jobs]


def _run_groups(work, engine: str, rng: str, stream_ids: Sequence[int],
                obs_range: Optional[range]) -> None:
    """work: (pricer, its path jobs) per trade; all share n_steps, n_half,
    antithetic and G.  Fills each job's value and sums and the pricer's
    _last_mc_std_error (that of its last job, as in the reference)."""
    first = work[0][1][0].plan
    n_total = first.n_half
    lo, hi = 0, n_total
    if obs_range is not None:
        lo, hi = obs_range.start, obs_range.stop
        if obs_range.step != 1 or not 0 <= lo < hi <= n_total:
            raise ValueError("obs_range must be a non-empty contiguous range within the "
                             "trade's observations")
        if rng != "philox" and (lo, hi) != (0, n_total):
            raise ValueError("obs_range needs mc_rng='philox' (a counter-based stream)")
    groups = [[j.plan for j in jobs] for _, jobs in work]
    n_obs = hi - lo
    n_sim = n_obs * (2 if first.antithetic else 1)
    pricer0 = work[0][0]
    if rng == "philox":
        seed = pricer0.mc_seed if pricer0.mc_seed is not None else secrets.randbits(63)
        stats = run_paths(groups, engine=engine, seed=seed, stream_ids=stream_ids, obs_first=lo,
                          n_obs=n_obs)
        pay = None
    else:
        z = draw_normals(rng, pricer0.mc_seed, n_total, first.n_steps)
        # the host engine keeps the per-path values: np.mean / np.std as the reference
        stats, pay = run_paths(groups, engine=engine, z=z, stream_ids=stream_ids,
                               want_payoffs=True) if engine == "host" else \
            (run_paths(groups, engine=engine, z=z, stream_ids=stream_ids), None)
    for b, (pricer, jobs) in enumerate(work):
        for g, job in enumerate(jobs):
            sums = tuple(float(v) for v in stats[b, g])
            if pay is not None:
                px, se = _compose_arrays(job.plan, pay[b, g, 0], pay[b, g, 1])
            else:
                px, se = compose(job.plan, n_sim, sums[0], sums[1], sums[2])
            job.value = job.base + job.sign * px
            job.sums = sums
            job.n_sim = n_sim
            pricer._last_mc_std_error = float(se)
            pricer._last_mc_sums = sums


def bgk_price_batch(trades: Sequence[dict], *, greeks: bool = False, engine: str = "hip",
                    mc_rng: Optional[str] = None, obs_range: Optional[range] = None) -> List[dict]:
    """Price many trades.  `trades`: constructor keyword dicts of
    DiscreteBarrierBGKPricer (without engine / mc_rng).  Trades that need paths
    run one launch per distinct (n_steps, observations, antithetic, G) -- G = 5
    with `greeks`, else 1 -- and, with host-drawn normals, per generator and
    seed, since a launch shares one z.  The Philox stream id of a trade is its
    index in `trades`.  `obs_range` (contiguous, within the observations; needs
    mc_rng="philox") runs that part of every trade's observations only; the raw
    sums of disjoint ranges add.  Results, in input order: price, method
    ("vanilla", "bgk" or "mc"), mc_std_error, n_paths and sums (sum x, sum x^2,
    sum rebate_pv, sum (1 - alive); None without paths), and delta / gamma /
    vega with `greeks`."""
    pricers = [DiscreteBarrierBGKPricer(engine=engine, mc_rng=mc_rng, **kw) for kw in trades]
    all_jobs: List[List[_Job]] = []
    bumps: List[Tuple[float, float]] = []
    for p in pricers:
        ds, dv = max(1e-8, 1e-4 * p.spot_price), 1e-4
        bumps.append((ds, dv))
        jobs = p._bumped_jobs(ds, dv) if greeks else [p._job()]
        all_jobs.append(jobs)
    launches: Dict[tuple, List[int]] = {}
    for k, (p, jobs) in enumerate(zip(pricers, all_jobs)):
        todo = [j for j in jobs if j.plan is not None]
        if not todo:
            continue
        rng = p._rng_kind()
        key = (todo[0].plan.n_steps, todo[0].plan.n_half, todo[0].plan.antithetic, len(todo), rng,
               p.mc_seed if rng != "philox" or p.mc_seed is not None else ("random", k))
        launches.setdefault(key, []).append(k)
    for key, members in launches.items():
        work = [(pricers[k], [j for j in all_jobs[k] if j.plan is not None]) for k in members]
        _run_groups(work, engine, key[4], members, obs_range)
    out = []
    for p, jobs, (ds, dv) in zip(pricers, all_jobs, bumps):
        main = jobs[2] if greeks else jobs[0]
        has_paths = main.plan is not None
        res = {"price": p._signed_scale(main.value),
               "method": ("vanilla" if p.barrier_type == "none" else p._select_method()),
               "mc_std_error": 0.0,
               "n_paths": main.n_sim, "sums": main.sums}
        if has_paths:   # the std error of the priced scenario, not of the last bump
            res["mc_std_error"] = compose(main.plan, main.n_sim, *main.sums[:3])[1]
        if greeks:
            unit = p.quantity * p.contract_multiplier
            up, dn, base, upv, dnv = (1.0 * unit * float(j.value) for j in jobs)
            scale = (1.0 if p.direction == "long" else -1.0) * unit
            res["delta"] = scale * ((up - dn) / (2 * ds))
            res["gamma"] = scale * ((up - 2 * base + dn) / (ds * ds))
            res["vega"] = scale * ((upv - dnv) / (2 * dv))
        out.append(res)
    return out
