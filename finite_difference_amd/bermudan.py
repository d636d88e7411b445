"""Bermudan option, optionally with a discretely monitored knock-out: plain
Crank-Nicolson segments cut at the exercise dates, with the exercise event
V <- max(V, payoff) between them.

The American march is already cut into tau-segments at its event dates
(american.py); the U chain of american_knockin.py already runs such segments
as plain Crank-Nicolson (``Solve(it=False)``).  A Bermudan option is that
chain with one more event.  One chain ``job["v"]``, every segment
``_segment_solve`` with ``it=False, payoff=None`` and the vanilla boundaries,
the segments those of ``_segments_over`` over the merged exercise, monitoring
and dividend times.  At an event time tau inside (0, T), with payoff phi, the
knocked nodes those of ``_ko_thresholds`` and R = ``_rebate(tau)``:

    kind of date               knocked nodes     other nodes
    exercise only              (none knocked)    max(V, phi)
    exercise and monitoring    max(phi, R)       max(V, phi)
    monitoring only            R                 unchanged

On a date that is both, the holder exercises an instant before monitoring (the
rule of american_barrier.py); on a monitoring date that is no exercise date
nobody may exercise, so the knocked nodes take the plain projection.  A
dividend on an event date comes after the event, marching backward, and its
jump has no exercise floor (a call is exercised on its exercise dates only).
Maturity always exercises: an exercise date there adds nothing, and a
monitoring date there applies max(phi, R) to the payoff as the parent class
does.  Dates at or before valuation are skipped.

Rannacher steps restart in the first segment, after an exercise event
(``restart_on_exercise``, default True), after a monitoring event
(``restart_on_monitoring``) and, for calls, after a dividend.

Without an exercise date inside the life and without a usable barrier the
march is one uncut Crank-Nicolson solve: the European option on the American
grid.  The value satisfies the PDE between events, so ``price_log``,
``price_log2``, ``greeks_log2`` (with its theta identity), Richardson and the
device epilogue are the parent's.  Knock-in types are not priced here.

``exercise_boundary`` reports where exercise was optimal at each date.
"""
from __future__ import annotations

import datetime as _dt
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import capi
from .american import AmericanFDMPricer, _one_of
from .american_barrier import AmericanBarrierFDMPricer
from .session import Session

__all__ = ["BermudanFDMPricer"]


def exercise_region(v: np.ndarray, floor: np.ndarray, knocked: np.ndarray) -> Tuple[int, int, int]:
    """(lo, hi, count) of the nodes that are not knocked and where floor_j >
    V_j (a NaN compares false); (n, -1, 0) when there are none."""
    idx = np.nonzero(~knocked & (floor > v))[0]
    if idx.size == 0:
        return int(v.shape[0]), -1, 0
    return int(idx[0]), int(idx[-1]), int(idx.size)


class BermudanFDMPricer(AmericanBarrierFDMPricer):
    """AmericanBarrierFDMPricer's keywords (knock-out types, rebate, cash
    dividends) plus ``exercise_dates``, the dates on which the holder may
    exercise besides maturity, and ``restart_on_exercise`` (default True),
    which restarts the Rannacher steps in the segment that follows (in tau) an
    exercise date."""

    def __init__(self, *args,
                 exercise_dates: Optional[List[_dt.date]] = None,
                 restart_on_exercise: bool = True,
                 **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.exercise_dates = sorted(set(exercise_dates or []))
        self.restart_on_exercise = bool(restart_on_exercise)

    # ---------------------------------------------------------------- events
    def _exercise_taus(self) -> List[Tuple[float, _dt.date]]:
        """(tau, date) of the exercise dates inside (0, T), ascending in tau.
        Dates at or before valuation are skipped; a date at maturity adds no
        event (maturity always exercises)."""
        T = self.time_to_expiry
        out: Dict[float, _dt.date] = {}
        for d in self.exercise_dates:
            if not (self.valuation_date < d <= self.maturity_date):
                continue
            t = self._year_fraction(self.valuation_date, d)
            if t <= 0.0 or t >= T - 1e-14:
                continue
            out.setdefault(T - t, d)
        return sorted(out.items())

    def _job_events(self, n_time: int):
        """The merged exercise, monitoring and dividend times: ("ex", ko_lo,
        ko_hi, rebate) at an exercise date (no node knocked unless it is a
        monitoring date too), ("kop", ko_lo, ko_hi, rebate), the plain
        projection, at a monitoring date that is none, then ("div", cash)."""
        mon, _ = self._monitor_taus()
        n = len(self.s_nodes)
        # one tau for events on one day: all three are T - _year_fraction(
        # valuation_date, date), as in AmericanBarrierFDMPricer._job_events
        at: Dict[float, list] = {}
        for tau, _d in self._exercise_taus():
            at[tau] = [("ex", -1, n, 0.0)]
        if mon:
            ko_lo, ko_hi = self._ko_thresholds()
            for tau in mon:
                kind = "ex" if tau in at else "kop"
                at[tau] = [(kind, ko_lo, ko_hi, self._rebate(tau))]
        mon_set = set(mon)
        for tau, cash in self._div_times_tau():
            at.setdefault(tau, []).append(("div", cash))
        taus = sorted(at)
        pts, steps = self._segments_over(taus, n_time)
        events = [at[tau] for tau in taus]
        call = self.option_type == "call"

        def restarts(seg: int) -> bool:
            if seg == 0:
                return True
            evs, tau = events[seg - 1], taus[seg - 1]
            return ((self.restart_on_exercise and evs[0][0] == "ex")
                    or (self.restart_on_monitoring and tau in mon_set)
                    or (call and any(e[0] == "div" for e in evs)))
        return events, pts, steps, [restarts(seg) for seg in range(len(steps))]

    def _make_job(self, key: tuple, sigma: float, n_time: int) -> dict:
        job = super()._make_job(key, sigma, n_time)
        # per exercise event, in the order of the march (tau ascending): the
        # host's (lo, hi, count), or the device session's region ids
        job["regions"], job["region_ids"] = [], []
        return job

    def _job_solves(self, job: dict, seg: int) -> list:
        s = self._segment_solve(job["v"], job["pts"][seg], job["pts"][seg + 1],
                                job["steps"][seg], job["restart"][seg])
        s.it, s.payoff = False, None
        return [("v", s)]

    def _apply_job_event(self, job: dict, seg: int, event: tuple) -> None:
        if event[0] == "div":  # no exercise floor between exercise dates
            job["v"] = capi.dividend_jump(self.s_nodes, job["v"], event[1], -1.0)
            return
        v = np.asarray(job["v"], dtype=np.float64)
        j = np.arange(v.shape[0])
        knocked = (j <= event[1]) | (j >= event[2])
        if event[0] == "kop":
            job["v"] = np.where(knocked, event[3], v)
            return
        pay = self._payoff_array()
        job["regions"].append(exercise_region(v, pay, knocked))
        job["v"] = np.where(knocked, np.maximum(pay, event[3]), np.maximum(v, pay))

    def _jump_chains(self, job: dict, seg: int) -> list:
        return [("v", -1.0)]

    def _state_key(self, sigma: float, n_time: int) -> tuple:
        return super()._state_key(sigma, n_time) + (
            "bermudan", tuple(self.exercise_dates), self.restart_on_exercise)

    # ------------------------------------------------------ exercise boundary
    def exercise_boundary(self, n_time: Optional[int] = None, *,
                          N_time: Optional[int] = None) -> List[tuple]:
        """One record ``(date, t, s_star, lo, hi, count)`` per exercise date
        inside the life, in calendar order, from the march of ``n_time`` steps
        (default ``num_time_steps``) at the pricer's sigma.

        ``lo``, ``hi`` and ``count`` describe the nodes that are not knocked
        and where payoff_j > V_j held before the event: the smallest and the
        largest such node and how many there are, raw; without any, ``lo =
        n_nodes``, ``hi = -1``, ``count = 0``.  ``s_star`` is the meaningful
        edge, the critical spot: ``s_nodes[hi]`` for a put, ``s_nodes[lo]``
        for a call, ``None`` when ``count == 0``.  The other edge is the
        grid's: with the put's lower Dirichlet value K exp(-r tau), below the
        payoff's K - S only from some node on, the lowest nodes are not in the
        region (at 400 nodes ``lo`` is 21 to 53, not 0), and ``count`` is not
        ``hi - lo + 1`` where knocked nodes interrupt the region.

        With a device engine the regions come from the session's exercise
        events (``Session.exercise_regions``)."""
        n_time = _one_of("n_time", n_time, "N_time", N_time)
        nt = self.num_time_steps if n_time is None else int(n_time)
        if self._skip_solve():
            return []
        engine = self._engine()
        jobs, _ = self._device_jobs([(self.sigma, nt)])
        job = jobs[0]
        if engine.on_device:
            with Session() as S:
                AmericanFDMPricer._march_jobs_device(jobs, engine, S)
                ids = job["region_ids"]
                regs = [tuple(int(x) for x in r) for r in S.exercise_regions(ids)] if ids else []
        else:
            self._march_jobs(jobs, engine)
            regs = job["regions"]
        s = job["grid"]["s_nodes"]
        T, put = self.time_to_expiry, self.option_type == "put"
        dates = self._exercise_taus()
        assert len(dates) == len(regs)
        out = []
        for (tau, d), (lo, hi, count) in zip(reversed(dates), reversed(regs)):
            s_star = None if count == 0 else float(s[hi] if put else s[lo])
            out.append((d, T - tau, s_star, lo, hi, count))
        return out
