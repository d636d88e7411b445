"""American option with a discretely monitored knock-out: the Ikonen-Toivanen
march of american.py cut at the monitoring dates.

The American solve already marches tau-segment by tau-segment between
ex-dividend dates, maps the value vector at each date and restarts lambda = 0
in the next segment (fd_american_equity.py:778-843).  A monitoring date is one
more event of that list.  At a monitoring time t_mon inside (0, T)

    V_j <- max(payoff_j, R)   on knocked nodes,   unchanged elsewhere,

with the knocked nodes compared on the job's own ``s_nodes`` as barrier.py's
integer thresholds do (up-and-out: s_j >= upper_barrier, down-and-out:
s_j <= lower_barrier, double-out: either) and R the rebate of barrier.py
(``rebate_amount`` when paid at the hit, else discounted at the carry rate
over the time left).  The exercise floor is the mathematics -- the holder may
exercise an instant before the monitoring time, V(t_mon-) = max(phi,
KO(V(t_mon+))) -- and the numerics: a knocked node left at 0 where the payoff
is 20 makes the next IT step build a multiplier of payoff/dt that leaks value
into the live region ("American knock-out").

A monitoring date at maturity applies the same rule to the terminal payoff;
dates at or before valuation are skipped.  A dividend on a monitoring date:
marching backward the knock-out comes first (monitoring sees the ex-dividend
spot), then the dividend jump, with no steps in between.

There is no in/out parity under early exercise, so the ``*-in`` types are not
priced here: AmericanKnockInFDMPricer (american_knockin.py) marches them as
two coupled chains.  Without a barrier, or without a monitoring date in (valuation,
maturity], every number equals AmericanFDMPricer's bit for bit.
"""
from __future__ import annotations

import datetime as _dt
from typing import Dict, List, Optional, Tuple

import numpy as np

from .american import AmericanFDMPricer
from .barrier import KO_TYPES, rebate_value

__all__ = ["AmericanBarrierFDMPricer"]


class AmericanBarrierFDMPricer(AmericanFDMPricer):
    """AmericanFDMPricer with the knock-out keywords of DiscreteBarrierFDMPricer.

    ``restart_on_monitoring`` (default True) restarts the Rannacher steps in
    the segment that follows (in tau) a monitoring date, for puts and calls;
    with False only the reference's rule applies (the first segment, and
    every segment of a call).

    ``already_hit=True`` returns ``rebate_amount`` itself as the price, with
    zero Greeks, whatever ``rebate_at_hit`` says.  This differs from
    DiscreteBarrierFDMPricer, whose price_log2 discounts the amount to
    ``discount_end_date`` (barrier.py): a caller who wants the present value
    of a rebate still to be paid at maturity multiplies by
    ``get_discount_factor(discount_end_date)``."""

    def __init__(self, *args,
                 barrier_type: str = "none",
                 lower_barrier: Optional[float] = None,
                 upper_barrier: Optional[float] = None,
                 monitor_dates: Optional[List[_dt.date]] = None,
                 rebate_amount: float = 0.0,
                 rebate_at_hit: bool = False,
                 already_hit: bool = False,
                 restart_on_monitoring: bool = True,
                 **kwargs) -> None:
        super().__init__(*args, **kwargs)
        bt = str(barrier_type).lower()
        if bt.endswith("-in"):
            raise ValueError(f"barrier_type {barrier_type!r}: knock-in types have no in/out "
                             "parity under early exercise and are not supported here; "
                             "use AmericanKnockInFDMPricer.")
        if bt != "none" and bt not in KO_TYPES:
            raise ValueError(f"Unsupported barrier_type: {barrier_type}")
        if bt in ("down-and-out", "double-out") and lower_barrier is None:
            raise ValueError(f"{bt} needs lower_barrier.")
        if bt in ("up-and-out", "double-out") and upper_barrier is None:
            raise ValueError(f"{bt} needs upper_barrier.")
        self.barrier_type = bt
        self.lower_barrier = None if lower_barrier is None else float(lower_barrier)
        self.upper_barrier = None if upper_barrier is None else float(upper_barrier)
        self.monitor_dates = sorted(set(monitor_dates or []))
        self.rebate_amount = float(rebate_amount)
        self.rebate_at_hit = bool(rebate_at_hit)
        self.already_hit = bool(already_hit)
        self.restart_on_monitoring = bool(restart_on_monitoring)

    # ---------------------------------------------------------------- events
    def _monitor_taus(self) -> Tuple[List[float], bool]:
        """(tau of the monitoring dates inside (0, T), ascending; whether a
        date falls on maturity).  Dates at or before valuation are skipped."""
        taus, at_maturity = [], False
        if self.barrier_type == "none":
            return taus, at_maturity
        T = self.time_to_expiry
        for d in self.monitor_dates:
            if not (self.valuation_date < d <= self.maturity_date):
                continue
            t = self._year_fraction(self.valuation_date, d)
            if t <= 0.0:
                continue
            if t >= T - 1e-14:
                at_maturity = True
            else:
                taus.append(T - t)
        return sorted(set(taus)), at_maturity

    def _ko_thresholds(self) -> Tuple[int, int]:
        """(ko_lo, ko_hi) on the current grid, the convention of FDCN_I_KO_LO /
        FDCN_I_KO_HI: nodes j <= ko_lo or j >= ko_hi are knocked (-1 / n_nodes:
        none); the per-node compares of barrier.py's _ko_thresholds."""
        s = self._s_array()
        ko_lo, ko_hi = -1, int(s.shape[0])
        if self.barrier_type in ("down-and-out", "double-out"):
            ko_lo = int(np.searchsorted(s, self.lower_barrier, side="right")) - 1
        if self.barrier_type in ("up-and-out", "double-out"):
            ko_hi = int(np.searchsorted(s, self.upper_barrier, side="left"))
        return ko_lo, ko_hi

    def _rebate(self, tau: float) -> float:
        return rebate_value(self.rebate_amount, self.rebate_at_hit, self.carry_rate_nacc, tau)

    def _ko_event(self, tau: float) -> tuple:
        ko_lo, ko_hi = self._ko_thresholds()
        return ("ko", ko_lo, ko_hi, self._rebate(tau))

    def _job_events(self, n_time: int):
        """AmericanFDMPricer._job_events over the merged dividend and
        monitoring times: _segments' step rule (_segments_over), the
        knock-out before the dividend jump where both fall on one date."""
        mon, _ = self._monitor_taus()
        if not mon:
            return super()._job_events(n_time)
        # A dividend and a monitoring date on one day share one tau exactly:
        # both are T - _year_fraction(valuation_date, date), the same
        # expression on the same date (_div_times_tau, _monitor_taus), so the
        # float key merges them; any change to either must keep that.
        at: Dict[float, list] = {tau: [self._ko_event(tau)] for tau in mon}
        for tau, cash in self._div_times_tau():
            at.setdefault(tau, []).append(("div", cash))
        taus = sorted(at)
        pts, steps = self._segments_over(taus, n_time)
        events = [at[tau] for tau in taus]
        restart = [seg == 0 or self.option_type == "call"
                   or (self.restart_on_monitoring and events[seg - 1][0][0] == "ko")
                   for seg in range(len(steps))]
        return events, pts, steps, restart

    def _initial_vector(self) -> np.ndarray:
        v = self._payoff_array()
        if self._monitor_taus()[1]:  # monitored at maturity: the same rule on the payoff
            _, ko_lo, ko_hi, reb = self._ko_event(0.0)
            v = self._apply_knockout(v, ko_lo, ko_hi, reb)
        return v

    def _state_key(self, sigma: float, n_time: int) -> tuple:
        return super()._state_key(sigma, n_time) + (
            self.barrier_type, self.lower_barrier, self.upper_barrier, tuple(self.monitor_dates),
            self.rebate_amount, self.rebate_at_hit, self.already_hit, self.restart_on_monitoring)

    # ------------------------------------------------- already knocked out
    def _skip_solve(self) -> bool:
        return self.already_hit and self.barrier_type != "none"

    def price_log(self, n_time: Optional[int] = None, *, N_time: Optional[int] = None) -> float:
        if self._skip_solve():
            return self.rebate_amount
        return super().price_log(n_time, N_time=N_time)

    def price_log2(self, apply_ko: bool = True, use_richardson: bool = True, *,
                   apply_KO: Optional[bool] = None) -> float:
        if self._skip_solve():
            return self.rebate_amount
        return super().price_log2(apply_ko, use_richardson, apply_KO=apply_KO)

    def greeks_log2(self, dv_sigma: float = 0.01, use_richardson: bool = True) -> Dict[str, float]:
        if self._skip_solve():
            return {"price": self.rebate_amount, "delta": 0.0, "gamma": 0.0, "vega": 0.0,
                    "theta": 0.0}
        return super().greeks_log2(dv_sigma, use_richardson)
