#!/usr/bin/env python3
"""Shared cases of the cash-dividend tests of the dual and the table-policy
Monte Carlo bounds (test_mc_bounds_div_host.py, test_gpu_mc_bounds_div.py) and
the generator of golden/bounds_div_cases.json.

BATCHES  lsm_div_cases.div_batches() -- 1, 2, 3 and 8 steps, all seven kinds,
         puts and calls, a dividend on the first step, on an odd and on an
         even step of a Philox pair, on two consecutive steps, on the last
         step and on a zero-length step, and the D = 45 on spot 100 contract
         whose lower branch carries a fifth of the paths -- plus, in m8_div,
         one down-and-out put whose dividend of 12 on a monitored step takes
         about half of the paths to the barrier there (an outer path knocked
         out on a dividend step).  G = 1 to 3 and both pairings are the
         batches' own; PARITY adds n_outer 1 and 3 and n_inner 512 and 1024.
         Each contract has a table of its own (policy_fixture.tables: put
         threshold, call threshold, finite band, the two "never", "always")
         and the fitted policies of its own least-squares sub-runs
         (host_subruns on the stream ids of lsm_div_cases.STREAM_IDS).
TRADES   the two Bermudan calls of the end-to-end tests.

Device and host agree within TAU_C = 1e-9 strike in a continuation value and
within TAU_X in a log-spot (measured under dividends: DESIGN section 13.5).
Per contract the generator stores the first of the 16 stream ids 16 b .. 16 b +
15 at which the host engines' smallest decision margin is at least 100 TAU_C
under the fitted rules (outer and inner decisions of the fitted dual) and the
first at which it is at least 100 TAU_X under the table (lower bound, outer and
inner decisions of the table dual).  No contract is dropped: generation fails
if none of the 16 qualifies (then change that contract's table entry).

Run as a script (CPU only, under a minute) it writes the golden file from the
project's own host engines.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import lsm_div_cases as ldc  # noqa: E402
import lsm_fixture as lf  # noqa: E402
import policy_fixture as pf  # noqa: E402
import test_bermudan_host as tb  # noqa: E402
from finite_difference_amd import mc_american  # noqa: E402
from finite_difference_amd.bermudan import BermudanFDMPricer  # noqa: E402

OUT = os.path.join(HERE, "golden", "bounds_div_cases.json")
PATH = "path"
TAU_X = 1e-12
MIN_MARGIN_X = 100.0 * TAU_X
N_CANDIDATES = 16
PARITY = {"m8_div": (3, 512), "m3_div": (1, 1024), "m2_div": (3, 1024), "m1_div": (1, 512)}
KO_DIV = 12.0  # of spot 100 on a monitored step, barrier 88
END_G, END_OUTER, END_INNER, END_SEED = pf.END_G, pf.END_OUTER, pf.END_INNER, pf.END_SEED


def batch(name):
    """(G, antithetic, seed, plans, table policies, the stream ids of the
    least-squares fits)."""
    G, anti, seed, plans = ldc.div_batches()[name]
    lsm_ids = list(ldc.STREAM_IDS[name])
    if name == "m8_div":
        plans = plans + [ldc.contract("down-and-out", "put", ldc.T8, (1, 4, 5, 7), range(8),
                                      {1: KO_DIV}, rebate=1.0, at_hit=True)]
        lsm_ids.append(0)
    return G, anti, seed, plans, pf.tables(plans), lsm_ids


def fitted(name):
    """coef [B, G, n_steps, LSM_NCOEF]: the host engine's fits, with dividends."""
    G, anti, seed, plans, _, lsm_ids = batch(name)
    return np.stack([mc_american.host_subruns(c, range(G), anti, seed, sid)["coef"]
                     for c, sid in zip(plans, lsm_ids)])


def host_lower(name, ids):
    G, anti, seed, plans, pols, _ = batch(name)
    return [mc_american.host_policy_subruns(c, pol, range(G), anti, seed, sid, PATH)
            for c, pol, sid in zip(plans, pols, ids)]


def host_table_dual(name, ids, subruns=None):
    G, anti, seed, plans, pols, _ = batch(name)
    n_outer, n_inner = PARITY[name]
    sub = range(G) if subruns is None else subruns
    return [mc_american.host_policy_dual_subruns(c, pol, sub, n_outer, n_inner, anti, seed, sid,
                                                 PATH)
            for c, pol, sid in zip(plans, pols, ids)]


def host_fitted_dual(name, coef, ids, subruns=None):
    G, anti, seed, plans, _, _ = batch(name)
    n_outer, n_inner = PARITY[name]
    sub = range(G) if subruns is None else subruns
    return [mc_american.host_dual_subruns(c, coef[b, sub.start:sub.stop], sub, n_outer, n_inner,
                                          anti, seed, ids[b], PATH)
            for b, c in enumerate(plans)]


def min_margin_c(c):
    """100 TAU_C of a contract."""
    return ldc.min_margin(c)


# ---- the end-to-end trades (spot 229.74, sigma 0.26, one month) --------------
def trade(name, engine, n):
    """(a) "weekly_230": the Bermudan call K 230 exercised weekly, D = 2.5 on an
    exercise date.  (b) "cum_200": the Bermudan call K 200 with D = 8 at
    DIV_MID, exercised weekly and on the business day before DIV_MID -- the
    cum-dividend exercise the American call of section 13.2 earns 6.786 from.
    "cum_200_european": (b) with maturity as its only exercise date."""
    if name == "weekly_230":
        return ldc.bermudan_call(engine, n)
    dates = dict(cum_200=sorted(tb.WEEKLY + [lf.WEEKDAYS[10]]), cum_200_european=[])[name]
    assert lf.WEEKDAYS[10] < ldc.DIV_MID == lf.WEEKDAYS[11]
    return ldc.american_call(engine, n, cls=BermudanFDMPricer, exercise_dates=dates)


def trade_case(name, engine):
    """(FD price at 400 x 400, |fd(400) - fd(200)|, contract, policy)."""
    p = trade(name, engine, 400)
    fd = p.price_log()
    coarse = trade(name, engine, 200).price_log()
    c = mc_american.contract_from_pricer(p, cash_dividends=PATH)
    return fd, abs(fd - coarse), c, mc_american.policy_from_pricer(p, c, cash_dividends=PATH)


# ---- the generator ----------------------------------------------------------
def main():
    doc = dict(batches={}, tau_x=TAU_X, min_margin_x_required=MIN_MARGIN_X,
               tau_c_rel=lf.TAU_C_REL)
    for name, (n_outer, n_inner) in PARITY.items():
        G, anti, seed, plans, pols, lsm_ids = batch(name)
        coef = fitted(name)
        sub = range(G)
        out = dict(table_ids=[], fit_ids=[], lower_margin=[], table_dual_margin=[],
                   fit_dual_margin=[], n_outer=n_outer, n_inner=n_inner, lsm_ids=lsm_ids)
        for b, (c, pol) in enumerate(zip(plans, pols)):
            cand = range(N_CANDIDATES * b, N_CANDIDATES * (b + 1))
            for sid in cand:
                ml = float(mc_american.host_policy_subruns(c, pol, sub, anti, seed, sid, PATH)
                           ["margin"].min())
                md = float(mc_american.host_policy_dual_subruns(
                    c, pol, sub, n_outer, n_inner, anti, seed, sid, PATH)["margin"].min())
                if min(ml, md) >= MIN_MARGIN_X:
                    break
            else:
                raise SystemExit(f"{name}[{b}]: no stream id of {N_CANDIDATES} has a table "
                                 f"margin of {MIN_MARGIN_X}")
            out["table_ids"].append(sid)
            out["lower_margin"].append(lf.finite(ml))
            out["table_dual_margin"].append(lf.finite(md))
            for sid in cand:
                mf = float(mc_american.host_dual_subruns(c, coef[b], sub, n_outer, n_inner, anti,
                                                         seed, sid, PATH)["margin"].min())
                if mf >= min_margin_c(c):
                    break
            else:
                raise SystemExit(f"{name}[{b}]: no stream id of {N_CANDIDATES} has a fitted "
                                 f"margin of {min_margin_c(c)}")
            out["fit_ids"].append(sid)
            out["fit_dual_margin"].append(lf.finite(mf))
        doc["batches"][name] = out
        print(name, out, flush=True)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
