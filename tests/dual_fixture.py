#!/usr/bin/env python3
"""Shared cases of the dual-bound tests (test_mc_dual_host.py,
test_gpu_mc_dual.py) and the generator of golden/lsm_dual_cases.json.

PARITY   per parity batch of lsm_fixture.batches() the (n_outer, n_inner) of
         its dual launch: n_outer 1 and 3, n_inner 512 and 1024, with the
         batches' own G (1, 2, 3) and antithetic on and off.
The policies of a batch are the host engine's least-squares fits on the
streams of golden/lsm_cases.json, so a device test that takes them from here
cannot see a policy difference.  The dual's own stream id of each contract is
chosen by the generator: the first of 16 b .. 16 b + 15 at which the host
engine's smallest decision margin, outer and inner decisions alike, is at
least lsm_fixture.MIN_MARGIN, so that no stopping decision can flip inside the
continuation-value tolerance (generation fails if none of the 16 qualifies).

Run as a script (CPU only, about a minute) it writes the golden file from the
project's own host engine:
batches  the stream ids above and their margins;
trades   for the three trades of lsm_fixture.TRADES, with the seed and stream
         ids of lsm_cases.json: gap, gap_stderr and the inner-path count of
         the host engine at G = 32, n_outer = 4, n_inner = 1024, and the
         two-sided bracket of the FD price it gives with the fixture's
         G = 1024 lower bound (asserted here and in test_mc_dual_host.py).
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

import lsm_fixture as lf  # noqa: E402
from finite_difference_amd import mc_american  # noqa: E402

OUT = os.path.join(HERE, "golden", "lsm_dual_cases.json")
PARITY = {"m8_all_kinds": (3, 512), "m8_bermudan": (3, 1024), "m3_kinds": (1, 512),
          "m2_kinds": (3, 1024), "m1_kinds": (1, 512)}
TRADE_G, TRADE_OUTER, TRADE_INNER = 32, 4, 1024
N_CANDIDATES = 16


def _golden(name):
    with open(os.path.join(HERE, "golden", name)) as f:
        return json.load(f)


def policies(name):
    """(plans, coef [B, G, n_steps, LSM_NCOEF]) of a parity batch: the host
    engine's fits on the streams of lsm_cases.json."""
    import numpy as np
    G, anti, seed, kws = lf.batches()[name]
    plans = lf.plan_batch(kws)
    ids = _golden("lsm_cases.json")["batches"][name]["stream_ids"]
    coef = np.stack([mc_american.host_subruns(c, range(G), anti, seed, sid)["coef"]
                     for c, sid in zip(plans, ids)])
    return plans, coef


def host_dual(name, plans, coef, ids, subruns=None):
    """Per contract of the batch: host_dual_subruns over its sub-runs."""
    G, anti, seed, _ = lf.batches()[name]
    n_outer, n_inner = PARITY[name]
    sub = range(G) if subruns is None else subruns
    return [mc_american.host_dual_subruns(c, coef[b, sub.start:sub.stop], sub, n_outer, n_inner,
                                          anti, seed, ids[b])
            for b, c in enumerate(plans)]


def trade_contract(name):
    from backends import oracle_engine
    return mc_american.contract_from_pricer(lf.trade_pricer(name, oracle_engine(), 400))


def trade_bracket(fix, gap, gap_stderr):
    """The result dict brackets() takes, from the fixture's G = 1024 lower
    bound and a gap; and the grid error |fd_3200 - fd_1600|."""
    res = dict(price=fix["price"], stderr=fix["stderr"], upper=fix["price"] + gap,
               upper_stderr=math.hypot(fix["stderr"], gap_stderr))
    return res, abs(fix["fd_3200"] - fix["fd_1600"])


# ---- the generator ----------------------------------------------------------
def _batches():
    out = {}
    for name in PARITY:
        plans, coef = policies(name)
        ids, margins = [], []
        for b in range(len(plans)):
            for sid in range(N_CANDIDATES * b, N_CANDIDATES * (b + 1)):
                one = host_dual(name, plans[b:b + 1], coef[b:b + 1], [sid])[0]
                m = float(one["margin"].min())
                if m >= lf.MIN_MARGIN:
                    break
            else:
                raise SystemExit(f"{name}[{b}]: no stream id of {N_CANDIDATES} has a margin of "
                                 f"{lf.MIN_MARGIN}")
            ids.append(sid)
            margins.append(lf.finite(m))
        out[name] = dict(stream_ids=ids, min_margin=margins, n_outer=PARITY[name][0],
                         n_inner=PARITY[name][1])
        print(name, out[name], flush=True)
    return out


def _trades():
    import time
    lsm = _golden("lsm_cases.json")["trades"]
    out = {}
    for name in lf.TRADES:
        fix = lsm[name]
        cfg = mc_american.LsmConfig(n_subruns=TRADE_G, antithetic=True, seed=fix["seed"])
        t0 = time.time()
        r = mc_american.mc_american_bounds_batch(
            [trade_contract(name)], cfg, mc_american.DualConfig(TRADE_OUTER, TRADE_INNER),
            engine="host", stream_ids=[fix["stream_id"]])[0]
        res, grid = trade_bracket(fix, r["gap"], r["gap_stderr"])
        out[name] = dict(gap=r["gap"], gap_stderr=r["gap_stderr"], inner_paths=r["inner_paths"],
                         n_subruns=TRADE_G, n_outer=TRADE_OUTER, n_inner=TRADE_INNER,
                         seed=fix["seed"], stream_id=fix["stream_id"], price_g32=r["price"],
                         stderr_g32=r["stderr"], upper=res["upper"],
                         upper_stderr=res["upper_stderr"])
        print(name, out[name], f"fd_3200 {fix['fd_3200']:.5f} lower {fix['price']:.5f} "
              f"{time.time() - t0:.1f} s", flush=True)
        assert mc_american.brackets(res, fix["fd_3200"], grid_error=grid, z=5.0), name
    return out


def main():
    doc = dict(batches=_batches(), trades=_trades(), min_margin_required=lf.MIN_MARGIN)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
