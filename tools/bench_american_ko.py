#!/usr/bin/env python3
"""Time of one American knock-out chain on the device session
(csrc/fdcn_session.hip: fdcn_session_march_ps + fdcn_session_knockout).

Workload: the American throughput configuration's trade and grid (the
notebook put over a strike x vol sweep, 2048 x 4096, 4096 scenarios) as a
down-and-out put monitored on every weekday: 23 segments, 22 knock-out events.
Every scenario shares the dates, so each segment is one launch for the batch.

Three times, same process, same grid and batch:

  chain       upload the payoff once, then per segment fdcn_session_march_ps
              and fdcn_session_knockout; ends with the price readout (which
              waits for the chain).  Wall clock around the calls.
  chain_host  the same chain through fdcn_session_march, which sends the
              payoff from the host with every segment.
  plain       one fdcn_it_batch_dev launch of all the steps (the vanilla
              American march: the code every segment runs), device events.

The chains are timed on the host clock and the plain launch with device
events, so chain_over_plain compares two clocks (a chain's kernel time needs
a kernel trace of this tool).  The launch plans are built before the clock
starts (the facade's own
_job_events / _segment_solve per scenario); the first scenarios are checked
against the facade's session path.  Prints one JSON line.  --dump-outputs DIR
writes the chain's prices as DIR/american_ko_prices.npy.  Without a GPU it
fails; there is no fallback.

--knock-in times the American knock-in chain instead (american_knockin.py:
the same trades as a down-and-in put, fdcn_session_knockin): per segment the
Ikonen-Toivanen march of W (fdcn_session_march_ps, up to the last monitoring
time), the Crank-Nicolson march of U and the knock-in event U <- W, 22 of
them.  Same clock as `chain`; the line then holds ki_chain, the knock-out
`chain` of the same process and the plain launch (chain_host is left out),
and --dump-outputs writes american_ki_prices.npy.

--bermudan times the Bermudan chain instead (bermudan.py: the same trades as
a put exercisable weekly, no barrier): five Crank-Nicolson segments with
fdcn_session_exercise between them, beside the knock-out `chain` of the same
process (same grid and batch, 23 Ikonen-Toivanen segments).  Same clock as
`chain`; the line holds bermudan_chain, chain and the range of the exercised
node counts per date.  A kernel trace of this mode shows exercise_kernel and
knockout_kernel on the same shape; --dump-outputs writes bermudan_prices.npy
and bermudan_regions.npy.
"""
from __future__ import annotations

import argparse
import datetime as dt
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
SPOT = 176.39


def weekdays():
    days = [VAL + dt.timedelta(days=k) for k in range((MAT - VAL).days + 1)]
    return [d for d in days if d.weekday() < 5]


def weekly():
    return [VAL + dt.timedelta(days=k) for k in (7, 14, 21, 28)]


def build_jobs(B: int, n_space: int, n_time: int, barrier: float, seed: int = 0,
               knock_in: bool = False, bermudan: bool = False):
    """One grid job per scenario: a single pricer re-pointed at each trade of
    the sweep (same dates and curve), as bench.py builds the vanilla batch."""
    from finite_difference_amd import (AmericanBarrierFDMPricer, AmericanKnockInFDMPricer,
                                       BermudanFDMPricer, market)
    cls = AmericanKnockInFDMPricer if knock_in else AmericanBarrierFDMPricer
    kw = dict(barrier_type="down-and-in" if knock_in else "down-and-out",
              lower_barrier=barrier, monitor_dates=weekdays())
    if bermudan:  # no barrier: the exercise event alone
        cls, kw = BermudanFDMPricer, dict(exercise_dates=weekly())
    curve = market.iso_curve(market.create_rate_df(math.exp(0.07053828272) - 1.0))
    p, jobs = None, []
    for i in range(B):
        j = (i * 2654435761 + seed * 97) % B
        strike = 140.0 + 70.0 * (j % 64) / 63.0
        sigma = 0.18 + 0.30 * ((j // 64) % 64) / 63.0
        if p is None:
            p = cls(
                spot=SPOT, strike=strike, valuation_date=VAL, maturity_date=MAT, sigma=sigma,
                option_type="put", discount_curve=curve, forward_curve=curve,
                num_space_nodes=n_space, num_time_steps=n_time, rannacher_steps=2, **kw)
        p._reset_trade(SPOT, strike, sigma)
        p._build_log_grid()
        jobs.append(p._make_job(p._state_key(sigma, n_time), sigma, n_time))
    return p, jobs


def segment_groups(p, jobs, n_time: int):
    """The launch group of every segment (all scenarios share pts / steps),
    and the group of the unsegmented march."""
    from finite_difference_amd import capi
    from finite_difference_amd.engine import Group, pack
    j0 = jobs[0]
    assert all(j["pts"] == j0["pts"] and j["steps"] == j0["steps"] for j in jobs)
    solves = []
    for j in jobs:
        p.sigma = j["sigma"]
        p._restore(j["grid"])
        solves.append(p._segment_solve(j["v"], j0["pts"][0], j0["pts"][1], j0["steps"][0],
                                       j0["restart"][0]))
    g0 = pack(solves, list(range(len(solves))))
    del solves

    def variant(tau0, tau1, steps, restart):
        P = g0.params.copy()
        P[:, capi.P_DT] = (tau1 - tau0) / float(steps)
        P[:, capi.P_TAU0] = tau0
        return Group(True, g0.n_nodes, int(steps), p.rannacher_steps if restart else 0, P,
                     g0.iparams, g0.v_init, g0.payoff, g0.mon_step, g0.mon_rebate, g0.index)
    groups = [variant(j0["pts"][s], j0["pts"][s + 1], j0["steps"][s], j0["restart"][s])
              for s in range(len(j0["steps"]))]
    assert np.array_equal(groups[0].params, g0.params)
    plain = variant(0.0, p.time_to_expiry, n_time, True)
    plain.v_init = g0.payoff  # the vanilla march starts from the payoff
    return groups, plain


def run_chain(p, jobs, groups, payoff_slots: bool):
    """One chain in a fresh session: (seconds from the first call to the end
    of the readout's wait, (seconds of the host calls that queue the chain,
    seconds of the payoff upload call among them), prices)."""
    from finite_difference_amd.session import GK_READOUT, Session
    n = groups[0].n_nodes
    ev = [[j["events"][s][0] for j in jobs] for s in range(len(groups) - 1)]
    lo = [np.array([e[1] for e in es], np.int32) for es in ev]
    hi = [np.array([e[2] for e in es], np.int32) for es in ev]
    reb = [np.array([e[3] for e in es]) for es in ev]
    # with rebate 0 the knock-out of the payoff at maturity leaves it as it is:
    # the chain then starts from the payoff slot (the facade does the same)
    from_slot = payoff_slots and all(j["v_is_payoff"] for j in jobs)
    with Session() as S:
        t0 = time.perf_counter()
        pay = S.upload(groups[0].payoff)
        t_upload = time.perf_counter() - t0
        slots = pay if from_slot else None
        for s, g in enumerate(groups):
            slots = S.march(g, slots, pay) if payoff_slots else S.march(g, slots)
            if s < len(ev):
                S.knockout(slots, n, lo[s], hi[s], reb[s], pay)
        t_queued = time.perf_counter() - t0
        trades = [(GK_READOUT, [p._job_readout(j, int(sl), False)], ())
                  for j, sl in zip(jobs, slots)]
        t1 = time.perf_counter()
        out = S.greeks(trades)  # waits for the chain
        t_wait = time.perf_counter() - t1
    # the readout plan is host work of this tool, not of the chain: the chain's
    # time is its calls plus the wait for the device
    return t_queued + t_wait, (t_queued, t_upload), out[:, 0].copy()


def knockin_groups(p, jobs):
    """The launch groups of the knock-in chain's two marches per segment: W
    (Ikonen-Toivanen, segments 0 .. w_last) and U (Crank-Nicolson, all)."""
    from finite_difference_amd import capi
    from finite_difference_amd.engine import Group, pack
    j0 = jobs[0]
    same = ("pts", "steps", "restart", "w_restart", "w_last")
    assert all(all(j[k] == j0[k] for k in same) for j in jobs)
    W, U = [], []
    for j in jobs:
        p.sigma = j["sigma"]
        p._restore(j["grid"])
        for chain, s in p._job_solves(j, 0):
            (W if chain == "w" else U).append(s)
    first = [pack(W, list(range(len(W)))), pack(U, list(range(len(U))))]
    del W, U

    def variant(g0, seg, restart):
        tau0, tau1, steps = j0["pts"][seg], j0["pts"][seg + 1], j0["steps"][seg]
        P = g0.params.copy()
        P[:, capi.P_DT] = (tau1 - tau0) / float(steps)
        P[:, capi.P_TAU0] = tau0
        return Group(g0.it, g0.n_nodes, int(steps), p.rannacher_steps if restart else 0, P,
                     g0.iparams, g0.v_init, g0.payoff, g0.mon_step, g0.mon_rebate, g0.index)
    gw = [variant(first[0], s, j0["w_restart"][s]) for s in range(j0["w_last"] + 1)]
    gu = [variant(first[1], s, j0["restart"][s]) for s in range(len(j0["steps"]))]
    assert np.array_equal(gw[0].params, first[0].params)
    assert np.array_equal(gu[0].params, first[1].params)
    return gw, gu


def run_knockin_chain(p, jobs, gw, gu):
    """run_chain for the knock-in: payoff uploaded once and named by W's
    marches, U's first march sends its initial vectors, then everything stays
    in slots; the prices are read from U."""
    from finite_difference_amd.session import GK_READOUT, Session
    n = gu[0].n_nodes
    ev = [[j["events"][s][0] for j in jobs] for s in range(len(gu) - 1)]
    assert all(e[0] == "ki" for es in ev for e in es)
    lo = [np.array([e[1] for e in es], np.int32) for es in ev]
    hi = [np.array([e[2] for e in es], np.int32) for es in ev]
    with Session() as S:
        t0 = time.perf_counter()
        pay = S.upload(gw[0].payoff)
        t_upload = time.perf_counter() - t0
        w, u = pay, None
        for s, g in enumerate(gu):
            if s < len(gw):
                w = S.march(gw[s], w, pay)
            u = S.march(g, u)
            if s < len(ev):
                S.knockin(u, n, lo[s], hi[s], w)
        t_queued = time.perf_counter() - t0
        trades = [(GK_READOUT, [p._job_readout(j, int(sl), False)], ())
                  for j, sl in zip(jobs, u)]
        t1 = time.perf_counter()
        out = S.greeks(trades)  # waits for the chain
        t_wait = time.perf_counter() - t1
    return t_queued + t_wait, (t_queued, t_upload), out[:, 0].copy()


def bermudan_groups(p, jobs):
    """The launch group of every segment of the Bermudan chain (plain
    Crank-Nicolson; all scenarios share pts / steps / restart)."""
    from finite_difference_amd import capi
    from finite_difference_amd.engine import Group, pack
    j0 = jobs[0]
    assert all(all(j[k] == j0[k] for k in ("pts", "steps", "restart")) for j in jobs)
    solves = []
    for j in jobs:
        p.sigma = j["sigma"]
        p._restore(j["grid"])
        solves.extend(s for _, s in p._job_solves(j, 0))
    g0 = pack(solves, list(range(len(solves))))
    del solves
    assert not g0.it

    def variant(seg):
        tau0, tau1, steps = j0["pts"][seg], j0["pts"][seg + 1], j0["steps"][seg]
        P = g0.params.copy()
        P[:, capi.P_DT] = (tau1 - tau0) / float(steps)
        P[:, capi.P_TAU0] = tau0
        return Group(False, g0.n_nodes, int(steps),
                     p.rannacher_steps if j0["restart"][seg] else 0, P, g0.iparams, g0.v_init,
                     g0.payoff, g0.mon_step, g0.mon_rebate, g0.index)
    groups = [variant(s) for s in range(len(j0["steps"]))]
    assert np.array_equal(groups[0].params, g0.params)
    return groups


def run_bermudan_chain(p, jobs, groups):
    """run_chain for the Bermudan put: payoff uploaded once, the first march
    starts from its slots, fdcn_session_exercise (no barrier) after every
    segment but the last; the region records are read back at the end."""
    from finite_difference_amd.session import GK_READOUT, Session
    n = groups[0].n_nodes
    assert all(j["v_is_payoff"] for j in jobs)
    assert all(len(evs) == 1 and evs[0][0] == "ex" for j in jobs for evs in j["events"])
    pay_host = groups[0].v_init  # the chain starts from the payoff
    with Session() as S:
        t0 = time.perf_counter()
        pay = S.upload(pay_host)
        t_upload = time.perf_counter() - t0
        slots, ids = pay, []
        for s, g in enumerate(groups):
            slots = S.march(g, slots)
            if s < len(groups) - 1:
                ids.append(S.exercise(slots, n, pay))
        t_queued = time.perf_counter() - t0
        trades = [(GK_READOUT, [p._job_readout(j, int(sl), False)], ())
                  for j, sl in zip(jobs, slots)]
        t1 = time.perf_counter()
        out = S.greeks(trades)  # waits for the chain
        t_wait = time.perf_counter() - t1
        regions = S.exercise_regions(np.concatenate(ids)).reshape(len(ids), len(jobs), 3)
    return t_queued + t_wait, (t_queued, t_upload), out[:, 0].copy(), regions


def run_plain(g, launches: int, warmup: int):
    import torch
    from finite_difference_amd import capi
    dev = torch.device("cuda:0")
    k_cap = capi.sm_extent(g.n_nodes, g.n_time, g.n_ranna, g.params)
    plan = capi.plan(g.n_nodes, True, k_cap, n_time=g.n_time, B=g.B)
    P, I = torch.from_numpy(g.params).to(dev), torch.from_numpy(g.iparams).to(dev)
    V0, F = torch.from_numpy(g.v_init).to(dev), torch.from_numpy(g.payoff).to(dev)
    out = torch.empty_like(V0)
    ws_bytes = max(8, plan["ws_bytes_per_scen"] * g.B)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream()

    def launch():
        capi.it_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, P.data_ptr(), I.data_ptr(),
                          V0.data_ptr(), F.data_ptr(), out.data_ptr(), k_cap, ws.data_ptr(),
                          ws_bytes, stream.cuda_stream)
    for _ in range(warmup):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    return times, torch.cuda.get_device_name(0)


def facade_parity(p, jobs, prices, count: int = 3):
    """The first scenarios through the facade's own session path."""
    from finite_difference_amd.american import AmericanFDMPricer
    from finite_difference_amd.session import GK_READOUT, Session
    sub = [dict(j) for j in jobs[:count]]
    with Session() as S:
        AmericanFDMPricer._march_jobs_device(sub, p._engine(), S)
        out = S.greeks([(GK_READOUT, [p._job_readout(j, j["slot"], False)], ()) for j in sub])
    worst = max(abs(float(a) - float(b)) / max(1.0, abs(float(b)))
                for a, b in zip(prices[:count], out[:, 0]))
    return {"scenarios": count, "worst_rel_price_diff": worst, "bound": 1e-9,
            "ok": bool(worst <= 1e-9)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n-space", type=int, default=2048)
    ap.add_argument("--n-time", type=int, default=4096)
    ap.add_argument("--barrier", type=float, default=150.0, help="down-and-out level")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    ap.add_argument("--knock-in", action="store_true",
                    help="time the knock-in chain (down-and-in at --barrier) beside the "
                         "knock-out chain and the plain launch")
    ap.add_argument("--bermudan", action="store_true",
                    help="time the Bermudan chain (a put exercisable weekly) beside the "
                         "knock-out chain")
    args = ap.parse_args()

    from finite_difference_amd import capi
    capi.require_device()
    t0 = time.perf_counter()
    p, jobs = build_jobs(args.batch, args.n_space, args.n_time, args.barrier)
    groups, plain = segment_groups(p, jobs, args.n_time)
    t_plan = time.perf_counter() - t0

    if args.knock_in:
        return main_knock_in(args, p, jobs, groups, plain, t_plan)
    if args.bermudan:
        return main_bermudan(args, p, jobs, groups, t_plan)
    res = {}
    for name, ps in (("chain", True), ("chain_host", False)):
        runs = [run_chain(p, jobs, groups, ps) for _ in range(args.warmup + args.reps)]
        runs = runs[args.warmup:]
        res[name] = {"seconds": [r[0] for r in runs], "queued": [r[1][0] for r in runs],
                     "upload": [r[1][1] for r in runs], "prices": runs[-1][2]}
    plain_t, device = run_plain(plain, args.reps, args.warmup)
    chain = statistics.median(res["chain"]["seconds"])
    chain_host = statistics.median(res["chain_host"]["seconds"])
    plain_med = statistics.median(plain_t)
    prices = res["chain"]["prices"]
    line = {
        "metric": "american_ko_chain_ms",
        "value": chain * 1e3,
        "device": device,
        "batch": args.batch, "n_space": args.n_space, "n_time": args.n_time,
        "segments": len(groups), "segment_steps": [int(g.n_time) for g in groups],
        "barrier": args.barrier, "reps": args.reps, "warmup": args.warmup,
        "chain_ms": {"median": chain * 1e3, "min": min(res["chain"]["seconds"]) * 1e3,
                     "max": max(res["chain"]["seconds"]) * 1e3,
                     "host_calls_ms": statistics.median(res["chain"]["queued"]) * 1e3,
                     "payoff_upload_call_ms": statistics.median(res["chain"]["upload"]) * 1e3},
        "chain_host_payoff_ms": {"median": chain_host * 1e3,
                                 "min": min(res["chain_host"]["seconds"]) * 1e3,
                                 "max": max(res["chain_host"]["seconds"]) * 1e3,
                                 "host_calls_ms":
                                     statistics.median(res["chain_host"]["queued"]) * 1e3},
        "plain_it_batch_dev_ms": {"median": plain_med * 1e3, "min": min(plain_t) * 1e3,
                                  "max": max(plain_t) * 1e3},
        "chain_over_plain": chain / plain_med,
        "chain_host_over_chain": chain_host / chain,
        "payoff_paths_bitwise_equal": bool(np.array_equal(prices, res["chain_host"]["prices"])),
        "plan_seconds": t_plan,
        "parity": facade_parity(p, jobs, prices),
        "all_finite": bool(np.all(np.isfinite(prices))),
        "price_range": [float(prices.min()), float(prices.max())],
    }
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "american_ko_prices.npy"), prices)
        line["dumped"] = {"american_ko_prices": list(prices.shape)}
    print(json.dumps(line))
    return 0 if line["parity"]["ok"] and line["all_finite"] else 3


def main_knock_in(args, p, jobs, groups, plain, t_plan: float) -> int:
    t0 = time.perf_counter()
    q, ki_jobs = build_jobs(args.batch, args.n_space, args.n_time, args.barrier, knock_in=True)
    gw, gu = knockin_groups(q, ki_jobs)
    t_plan += time.perf_counter() - t0

    def spread(runs):
        sec = [r[0] for r in runs]
        return {"median": statistics.median(sec) * 1e3, "min": min(sec) * 1e3,
                "max": max(sec) * 1e3,
                "host_calls_ms": statistics.median([r[1][0] for r in runs]) * 1e3}
    ki = [run_knockin_chain(q, ki_jobs, gw, gu) for _ in range(args.warmup + args.reps)]
    ki = ki[args.warmup:]
    ko = [run_chain(p, jobs, groups, True) for _ in range(args.warmup + args.reps)]
    ko = ko[args.warmup:]
    plain_t, device = run_plain(plain, args.reps, args.warmup)
    plain_med = statistics.median(plain_t)
    prices = ki[-1][2]
    line = {
        "metric": "american_ki_chain_ms",
        "value": spread(ki)["median"],
        "device": device,
        "batch": args.batch, "n_space": args.n_space, "n_time": args.n_time,
        "segments": len(gu), "w_segments": len(gw),
        "segment_steps": [int(g.n_time) for g in gu],
        "barrier": args.barrier, "reps": args.reps, "warmup": args.warmup,
        "ki_chain_ms": spread(ki),
        "chain_ms": spread(ko),
        "plain_it_batch_dev_ms": {"median": plain_med * 1e3, "min": min(plain_t) * 1e3,
                                  "max": max(plain_t) * 1e3},
        "ki_over_chain": spread(ki)["median"] / spread(ko)["median"],
        "ki_over_plain": spread(ki)["median"] * 1e-3 / plain_med,
        "plan_seconds": t_plan,
        "parity": facade_parity(q, ki_jobs, prices),
        "all_finite": bool(np.all(np.isfinite(prices))),
        "price_range": [float(prices.min()), float(prices.max())],
    }
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "american_ki_prices.npy"), prices)
        line["dumped"] = {"american_ki_prices": list(prices.shape)}
    print(json.dumps(line))
    return 0 if line["parity"]["ok"] and line["all_finite"] else 3


def main_bermudan(args, p, jobs, groups, t_plan: float) -> int:
    t0 = time.perf_counter()
    q, b_jobs = build_jobs(args.batch, args.n_space, args.n_time, args.barrier, bermudan=True)
    gb = bermudan_groups(q, b_jobs)
    t_plan += time.perf_counter() - t0

    def spread(runs):
        sec = [r[0] for r in runs]
        return {"median": statistics.median(sec) * 1e3, "min": min(sec) * 1e3,
                "max": max(sec) * 1e3,
                "host_calls_ms": statistics.median([r[1][0] for r in runs]) * 1e3}
    bm = [run_bermudan_chain(q, b_jobs, gb) for _ in range(args.warmup + args.reps)]
    bm = bm[args.warmup:]
    ko = [run_chain(p, jobs, groups, True) for _ in range(args.warmup + args.reps)]
    ko = ko[args.warmup:]
    prices, regions = bm[-1][2], bm[-1][3]
    line = {
        "metric": "bermudan_chain_ms",
        "value": spread(bm)["median"],
        "batch": args.batch, "n_space": args.n_space, "n_time": args.n_time,
        "segments": len(gb), "segment_steps": [int(g.n_time) for g in gb],
        "ko_segments": len(groups), "reps": args.reps, "warmup": args.warmup,
        "bermudan_chain_ms": spread(bm),
        "chain_ms": spread(ko),
        "bermudan_over_chain": spread(bm)["median"] / spread(ko)["median"],
        "plan_seconds": t_plan,
        "parity": facade_parity(q, b_jobs, prices),
        "all_finite": bool(np.all(np.isfinite(prices))),
        "price_range": [float(prices.min()), float(prices.max())],
        # per exercise date (tau ascending): the exercised node counts over the batch
        "region_count_range": [[int(r[:, 2].min()), int(r[:, 2].max())] for r in regions],
    }
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "bermudan_prices.npy"), prices)
        np.save(os.path.join(args.dump_outputs, "bermudan_regions.npy"), regions)
        line["dumped"] = {"bermudan_prices": list(prices.shape),
                          "bermudan_regions": list(regions.shape)}
    print(json.dumps(line))
    return 0 if line["parity"]["ok"] and line["all_finite"] else 3


if __name__ == "__main__":
    sys.exit(main())
