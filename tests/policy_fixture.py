#!/usr/bin/env python3
"""Shared cases of the table-policy Monte Carlo tests (test_mc_policy_host.py,
test_gpu_mc_policy.py) and the generator of golden/policy_cases.json.

BATCHES  the parity batches of lsm_fixture.batches() -- 1, 2, 3 and 8 steps,
         every kind, puts and calls, G = 1 to 3, antithetic on and off -- each
         contract with a table of its own (tables()): put and call thresholds,
         finite bands, "always" (-inf, +inf), "never" as LO > HI with finite
         and with infinite entries, and, in m8_bermudan, finite rows on steps
         without an EXERCISE flag.
PARITY   dual_fixture.PARITY: the (n_outer, n_inner) of each batch's dual launch.
TRADES   the three Bermudan trades of the end-to-end test: the vanilla put of
         test_bermudan_host.py exercised on weekdays and weekly, and the
         strike-250 up-and-out put (barrier 240) exercised and monitored weekly;
         END_G, END_OUTER, END_INNER are the sizes of that test.

The log-spot of device and host agree within TAU_X at every decision
(measured: DESIGN section 13.4).  The generator picks, per contract, the first
of the 16 stream ids 16 b .. 16 b + 15 at which the host engines' smallest
decision margin -- lower bound and dual, outer and inner decisions alike -- is
at least MIN_MARGIN_X = 100 TAU_X, so that no decision can flip inside the
tolerance; generation fails if none of the 16 qualifies (then change the
contract's table, not the rule).

Run as a script (CPU only, a few seconds) it writes the golden file from the
project's own host engines.
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import dual_fixture as df  # noqa: E402
import lsm_fixture as lf  # noqa: E402
from finite_difference_amd import mc_american  # noqa: E402

OUT = os.path.join(HERE, "golden", "policy_cases.json")
TAU_X = 1e-12
MIN_MARGIN_X = 100.0 * TAU_X
N_CANDIDATES = 16
PARITY = df.PARITY
END_G, END_OUTER, END_INNER, END_SEED = 256, 2, 512, 42
INF = math.inf
# the rows a table cycles through; spots around the batches' spot of 100
ROWS = (
    (-INF, math.log(95.0)),              # a put's threshold
    (math.log(104.0), INF),              # a call's threshold
    (math.log(92.0), math.log(108.0)),   # a finite band
    (math.log(105.0), math.log(95.0)),   # never: LO > HI, finite
    (-INF, INF),                         # always
    (INF, -INF),                         # never: LO > HI, infinite
)


def tables(plans):
    """One ExercisePolicy per contract: row (b + i) % 6 of ROWS at step i of
    contract b, EXERCISE flag or not (a row without the flag is ignored)."""
    out = []
    for b, c in enumerate(plans):
        rows = [ROWS[(b + i) % len(ROWS)] for i in range(c.n_steps)]
        out.append(mc_american.ExercisePolicy([r[0] for r in rows], [r[1] for r in rows]))
    return out


def batch(name):
    """(G, antithetic, seed, plans, policies) of a parity batch."""
    G, anti, seed, kws = lf.batches()[name]
    plans = lf.plan_batch(kws)
    return G, anti, seed, plans, tables(plans)


def host_lower(name, ids):
    G, anti, seed, plans, pols = batch(name)
    return [mc_american.host_policy_subruns(c, pol, range(G), anti, seed, sid)
            for c, pol, sid in zip(plans, pols, ids)]


def host_dual(name, ids, subruns=None):
    G, anti, seed, plans, pols = batch(name)
    n_outer, n_inner = PARITY[name]
    sub = range(G) if subruns is None else subruns
    return [mc_american.host_policy_dual_subruns(c, pol, sub, n_outer, n_inner, anti, seed, sid)
            for c, pol, sid in zip(plans, pols, ids)]


def trade_kw():
    from test_bermudan_host import WEEKDAYS, WEEKLY
    return {
        "put_weekdays": dict(exercise_dates=WEEKDAYS),
        "put_weekly": dict(exercise_dates=WEEKLY),
        "up_out_250_weekly": dict(exercise_dates=WEEKLY, strike=250.0, barrier_type="up-and-out",
                                  upper_barrier=240.0, rebate_amount=0.0, rebate_at_hit=True,
                                  monitor_dates=WEEKLY),
    }


def trade_case(name, engine=None):
    """(pricer at 400 x 400, its FD price, |fd(N) - fd(N / 2)|, contract, policy)."""
    from backends import oracle_engine
    from test_bermudan_host import trade
    engine = oracle_engine() if engine is None else engine
    kw = trade_kw()[name]
    p = trade(engine, **kw)
    fd = p.price_log()
    coarse = trade(engine, n=200, m=200, **kw).price_log()
    c = mc_american.contract_from_pricer(p)
    return p, fd, abs(fd - coarse), c, mc_american.policy_from_pricer(p, c)


# ---- the generator ----------------------------------------------------------
def main():
    doc = dict(batches={}, tau_x=TAU_X, min_margin_required=MIN_MARGIN_X)
    for name in PARITY:
        G, anti, seed, plans, pols = batch(name)
        n_outer, n_inner = PARITY[name]
        ids, lower, dual = [], [], []
        for b, (c, pol) in enumerate(zip(plans, pols)):
            for sid in range(N_CANDIDATES * b, N_CANDIDATES * (b + 1)):
                ml = float(mc_american.host_policy_subruns(c, pol, range(G), anti, seed,
                                                           sid)["margin"].min())
                md = float(mc_american.host_policy_dual_subruns(
                    c, pol, range(G), n_outer, n_inner, anti, seed, sid)["margin"].min())
                if min(ml, md) >= MIN_MARGIN_X:
                    break
            else:
                raise SystemExit(f"{name}[{b}]: no stream id of {N_CANDIDATES} has a margin of "
                                 f"{MIN_MARGIN_X}")
            ids.append(sid)
            lower.append(lf.finite(ml))
            dual.append(lf.finite(md))
        doc["batches"][name] = dict(stream_ids=ids, min_margin=lower, dual_min_margin=dual,
                                    n_outer=n_outer, n_inner=n_inner)
        print(name, doc["batches"][name], flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
