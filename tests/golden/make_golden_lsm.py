#!/usr/bin/env python3
"""Writes tests/golden/lsm_cases.json from this project's own engines (CPU
only, a few minutes):

trades   for the three trades of tests/lsm_fixture.py: the FD price on the CPU
         oracle engine at N = M = 1600 and 3200, and the host engine's
         out-of-sample least-squares Monte Carlo price at G = FIXTURE_G
         sub-runs with its standard error, through contract_from_pricer.
batches  for every contract of the parity batches the Philox stream id, the
         first of b, b + 100, b + 200, ... at which the host engine's smallest
         decision margin is at least MIN_MARGIN = 100 tau_c (asserted), and
         that margin.

Usage: python tests/golden/make_golden_lsm.py [--trades-only | --batches-only]
(the other part is kept from the existing file).
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import lsm_fixture as lf  # noqa: E402
from backends import oracle_engine  # noqa: E402
from finite_difference_amd import mc_american  # noqa: E402

OUT = os.path.join(HERE, "lsm_cases.json")


def trades():
    out = {}
    for k, name in enumerate(lf.TRADES):
        fd = {}
        for n in (1600, 3200):
            fd[n] = float(lf.trade_pricer(name, oracle_engine(), n).price_log())
        p = lf.trade_pricer(name, oracle_engine(), 400)
        c = mc_american.contract_from_pricer(p)
        r = mc_american.price_american_mc(c, n_subruns=lf.FIXTURE_G, antithetic=True,
                                          seed=lf.FIXTURE_SEED, stream_id=k, engine="host")
        out[name] = dict(fd_1600=fd[1600], fd_3200=fd[3200], spot=float(c.params[0]),
                         strike=float(c.params[1]), n_steps=c.n_steps, n_subruns=lf.FIXTURE_G,
                         seed=lf.FIXTURE_SEED, stream_id=k, price=r["price"], stderr=r["stderr"],
                         fit_value=r["fit_value"], fit_stderr=r["fit_stderr"],
                         invalid_fit_steps=r["invalid_fit_steps"])
        print(name, out[name], flush=True)
    return out


def batches():
    out = {}
    for name, (G, anti, seed, kws) in lf.batches().items():
        ids, margins = [], []
        for b, c in enumerate(lf.plan_batch(kws)):
            for sid in range(b, b + 100 * 50, 100):
                m = float(mc_american.host_subruns(c, range(G), anti, seed, sid)["margin"].min())
                if m >= lf.MIN_MARGIN:
                    break
            assert m >= lf.MIN_MARGIN, (name, b, m)
            ids.append(sid)
            margins.append(lf.finite(m))
        out[name] = dict(stream_ids=ids, min_margin=margins)
        print(name, out[name], flush=True)
    return out


def main():
    old = json.load(open(OUT)) if os.path.exists(OUT) else {}
    doc = dict(old)
    if "--batches-only" not in sys.argv:
        doc["trades"] = trades()
    if "--trades-only" not in sys.argv:
        doc["batches"] = batches()
    doc["min_margin_required"] = lf.MIN_MARGIN
    assert all(math.isfinite(v["price"]) for v in doc.get("trades", {}).values())
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
