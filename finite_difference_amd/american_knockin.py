"""American option with a discretely monitored knock-in: two coupled chains
over the segments of american_barrier.py's knock-out march.

There is no in/out parity under early exercise, but the product is well
defined.  Once the barrier is seen breached at a monitoring date the holder
owns a vanilla American option, value W; before that nothing can be exercised
and the value U follows the plain Black-Scholes PDE.  Marching backward in
tau, both chains run over the same segments (the merged dividend and
monitoring times, cut by ``_segments_over`` exactly as the knock-out cuts
them, the same ``pts`` and ``steps``):

W   the vanilla American Ikonen-Toivanen march: vanilla boundaries, the
    payoff, the reference's Rannacher rule (the first segment, and every
    segment of a call), the dividend jump with the call's exercise floor.  It
    has no monitoring event of its own.
U   plain Crank-Nicolson segments (``Solve(it=False)``) with the same
    coefficients, dt, tau0 and tau accumulation.  At maturity U = R, the
    rebate, on every node (a knock-in rebate is paid at maturity if the
    option never knocked in); where a monitoring date falls on maturity the
    knocked nodes hold the payoff instead.  On a side of the grid that lies
    inside the knock-in region (its edge node is knocked: the lower side of a
    down-and-in whose barrier is on the grid) the Dirichlet value is the
    vanilla boundary of that side; on a side outside it (the other side, and
    both sides of a barrier the grid does not reach) it is the rebate alone,
    R exp(-r tau) with r the discount rate (the exact solution for a
    constant).  Rannacher restarts in the first segment, after a dividend for
    calls (the reference's rule) and, with ``restart_on_monitoring`` (default
    True), after every monitoring date: the event puts a jump into U at the
    barrier.

At a monitoring time inside (0, T)

    U_j <- W_j   on knocked nodes,   unchanged elsewhere,

with the knocked nodes those of the matching ``*-out`` type
(``_ko_thresholds`` on the job's own ``s_nodes``) and both vectors those
after the segment that ends there, before a dividend jump at the same time:
monitoring sees the ex-dividend spot, as in the knock-out.  A dividend jump
then maps both chains, W with the call's exercise floor and U without it (the
holder of U cannot exercise).  W marches only as far as the last monitoring
time that reads it.

Price, Greeks and the cached value vector all read U; the theta identity
holds for U, which satisfies the PDE wherever it is not overwritten.

With ``already_in=True`` or ``barrier_type="none"`` every number is
AmericanFDMPricer's bit for bit (the uncut chain).  Without a monitoring date
in (valuation, maturity] the option can never knock in: the price is
R exp(-r T) with zero delta, gamma and vega and theta from the identity, and
nothing is solved.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

from . import capi
from .american import AmericanFDMPricer
from .american_barrier import AmericanBarrierFDMPricer
from .engine import FORM_SUM, Boundary

__all__ = ["AmericanKnockInFDMPricer"]

_OUT_OF = {"up-and-in": "up-and-out", "down-and-in": "down-and-out", "double-in": "double-out"}


class AmericanKnockInFDMPricer(AmericanBarrierFDMPricer):
    """AmericanBarrierFDMPricer's keywords for the knock-in types
    (``up-and-in``, ``down-and-in``, ``double-in``, ``none``), with
    ``already_in`` in place of ``already_hit``.  The rebate is paid at
    maturity if the option never knocked in, so ``rebate_at_hit=True`` is
    refused.  ``restart_on_monitoring`` acts on the U chain only."""

    def __init__(self, *args,
                 barrier_type: str = "none",
                 rebate_at_hit: bool = False,
                 already_in: bool = False,
                 **kwargs) -> None:
        bt = str(barrier_type).lower()
        if bt.endswith("-out"):
            raise ValueError(f"barrier_type {barrier_type!r}: knock-out types are priced by "
                             "AmericanBarrierFDMPricer.")
        if bt != "none" and bt not in _OUT_OF:
            raise ValueError(f"Unsupported barrier_type: {barrier_type}")
        if rebate_at_hit:
            raise ValueError("rebate_at_hit=True: a knock-in rebate is paid at maturity, if the "
                             "option never knocked in.")
        if "already_hit" in kwargs:
            raise TypeError("already_hit belongs to AmericanBarrierFDMPricer; a knock-in takes "
                            "already_in.")
        try:  # the barrier levels required are those of the matching *-out type
            super().__init__(*args, barrier_type=_OUT_OF.get(bt, "none"), rebate_at_hit=False,
                             **kwargs)
        except ValueError as e:
            out = _OUT_OF.get(bt)
            raise ValueError(str(e).replace(out, bt) if out else str(e)) from None
        self.barrier_type = bt
        self.already_in = bool(already_in)

    # ---------------------------------------------------------------- events
    def _plain(self) -> bool:
        """The uncut vanilla chain: no barrier, or already knocked in."""
        return self.already_in or self.barrier_type == "none"

    def _ko_thresholds(self) -> Tuple[int, int]:
        """The knocked nodes of the matching *-out type."""
        bt = self.barrier_type
        self.barrier_type = _OUT_OF.get(bt, bt)
        try:
            return super()._ko_thresholds()
        finally:
            self.barrier_type = bt

    def _u_boundaries(self) -> Tuple[Boundary, Boundary]:
        """Dirichlet values of U on the current grid: the vanilla boundary on a
        side inside the knock-in region (its edge node is knocked), the
        discounted rebate on a side outside it."""
        lower, upper = self._boundaries()
        R = self.rebate_amount
        reb = Boundary(FORM_SUM, R, -self.discount_rate_nacc, 0.0, 0.0) if R != 0.0 else Boundary()
        ko_lo, ko_hi = self._ko_thresholds()
        n = len(self.s_nodes)
        if not (ko_lo >= 0 or ko_hi <= 0):
            lower = reb
        if not (ko_hi <= n - 1 or ko_lo >= n - 1):
            upper = reb
        return lower, upper

    def _job_events(self, n_time: int):
        """The knock-out class's segments with ("ki", ko_lo, ko_hi) at every
        monitoring time, before the dividend jump of the same time; restart
        is the U chain's rule."""
        mon, _ = ([], False) if self._plain() else self._monitor_taus()
        if not mon:
            return AmericanFDMPricer._job_events(self, n_time)
        ko_lo, ko_hi = self._ko_thresholds()
        # one tau for a dividend and a monitoring date on one day, as in
        # AmericanBarrierFDMPricer._job_events
        at: Dict[float, list] = {tau: [("ki", ko_lo, ko_hi)] for tau in mon}
        for tau, cash in self._div_times_tau():
            at.setdefault(tau, []).append(("div", cash))
        taus = sorted(at)
        pts, steps = self._segments_over(taus, n_time)
        events = [at[tau] for tau in taus]
        call = self.option_type == "call"
        restart = [seg == 0
                   or (call and any(e[0] == "div" for e in events[seg - 1]))
                   or (self.restart_on_monitoring and events[seg - 1][0][0] == "ki")
                   for seg in range(len(steps))]
        return events, pts, steps, restart

    def _initial_vector(self) -> np.ndarray:
        """U at maturity: the rebate, and the payoff on the nodes knocked by a
        monitoring date at maturity."""
        pay = self._payoff_array()
        if self._plain():
            return pay
        v = np.full(pay.shape[0], self.rebate_amount, dtype=np.float64)
        if self._monitor_taus()[1]:
            ko_lo, ko_hi = self._ko_thresholds()
            j = np.arange(pay.shape[0])
            v = np.where((j <= ko_lo) | (j >= ko_hi), pay, v)
        return v

    def _make_job(self, key: tuple, sigma: float, n_time: int) -> dict:
        job = super()._make_job(key, sigma, n_time)
        if self._plain():
            return job
        # the coupled chain W: marched up to the last knock-in that reads it
        # (-1: never), with the reference's Rannacher rule
        job["w"] = self._payoff_array()
        job["w_last"] = max((i for i, evs in enumerate(job["events"])
                             if any(e[0] == "ki" for e in evs)), default=-1)
        job["w_restart"] = [seg == 0 or self.option_type == "call"
                            for seg in range(len(job["steps"]))]
        return job

    def _job_solves(self, job: dict, seg: int) -> list:
        if "w" not in job:
            return super()._job_solves(job, seg)
        a, b, ns = job["pts"][seg], job["pts"][seg + 1], job["steps"][seg]
        out = []
        if seg <= job["w_last"]:
            out.append(("w", self._segment_solve(job["w"], a, b, ns, job["w_restart"][seg])))
        u = self._segment_solve(job["v"], a, b, ns, job["restart"][seg])
        u.it, u.payoff = False, None
        u.lower, u.upper = self._u_boundaries()
        out.append(("v", u))
        return out

    def _apply_job_event(self, job: dict, seg: int, event: tuple) -> None:
        if "w" not in job:
            return super()._apply_job_event(job, seg, event)
        if event[0] == "ki":
            u = np.asarray(job["v"], dtype=np.float64)
            j = np.arange(u.shape[0])
            job["v"] = np.where((j <= event[1]) | (j >= event[2]),
                                np.asarray(job["w"], dtype=np.float64), u)
            return
        # the dividend jump: U without the call's exercise floor, W as vanilla
        job["v"] = capi.dividend_jump(self.s_nodes, job["v"], event[1], -1.0)
        if seg < job["w_last"]:
            job["w"] = np.asarray(self._apply_dividend_jump(job["w"], event[1]))

    def _jump_chains(self, job: dict, seg: int) -> list:
        if "w" not in job:
            return super()._jump_chains(job, seg)
        out = [("v", -1.0)]
        if seg < job["w_last"]:
            out += [("w", kc) for _, kc in super()._jump_chains(job, seg)]
        return out

    def _state_key(self, sigma: float, n_time: int) -> tuple:
        return super()._state_key(sigma, n_time) + ("knock-in", self.already_in)

    # ------------------------------------------------- can never knock in
    def _skip_solve(self) -> bool:
        if self._plain():
            return False
        mon, at_maturity = self._monitor_taus()
        return not mon and not at_maturity

    def _never_in(self) -> Dict[str, float]:
        r = self.discount_rate_nacc
        price = self.rebate_amount * math.exp(-r * self.time_to_expiry)
        return {"price": price, "delta": 0.0, "gamma": 0.0, "vega": 0.0, "theta": r * price}

    def price_log(self, n_time: Optional[int] = None, *, N_time: Optional[int] = None) -> float:
        if self._skip_solve():
            return self._never_in()["price"]
        return AmericanFDMPricer.price_log(self, n_time, N_time=N_time)

    def price_log2(self, apply_ko: bool = True, use_richardson: bool = True, *,
                   apply_KO: Optional[bool] = None) -> float:
        if self._skip_solve():
            return self._never_in()["price"]
        return AmericanFDMPricer.price_log2(self, apply_ko, use_richardson, apply_KO=apply_KO)

    def greeks_log2(self, dv_sigma: float = 0.01, use_richardson: bool = True) -> Dict[str, float]:
        if self._skip_solve():
            return self._never_in()
        return AmericanFDMPricer.greeks_log2(self, dv_sigma, use_richardson)
