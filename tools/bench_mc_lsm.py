#!/usr/bin/env python3
"""Throughput of the least-squares Monte Carlo kernel (csrc/fdcn_mc_lsm.hip).

Device: `--contracts` contracts (the seven barrier kinds in turn, spot and
strike spread by a seeded draw) x `--subruns` sub-runs of 4 096 paths x
`--steps` steps, antithetic, every array resident on the device, through
fdcn_mc_lsm_batch_dev with a planned workspace.  Warm-up, then `--launches`
launches timed one by one with device events; the median is the result.  A
path-step is one `x += drift + diff z` of one path in one pass, and the
kernel makes three passes (fit set forward, fit set backward with the
regressions, price set forward): 3 x paths x steps per launch.

Yardstick, same process: the NumPy host engine (mc_american.host_subruns, the
same algorithm on the same streams) on `--host-contracts` contracts x
`--host-subruns` sub-runs, on threads sized from OMP_NUM_THREADS (1 if unset).

--dividends N puts a cash dividend on N steps of every contract (spread over
the life, none on the last step) and times the dividend instance of the kernel
(fdcn_mc_lsm_div_batch_dev) beside the plain launch of the same batch without
them, in the same process: both medians and their ratio join the JSON line.

Prints one JSON line.  --dump-outputs DIR writes the stats of the last timed
plain launch as DIR/mc_lsm_stats.npy.  Without a GPU it fails; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KINDS = ("none", "down-and-out", "up-and-out", "double-out", "down-and-in", "up-and-in",
         "double-in")


def build_batch(B: int, n_steps: int, seed: int = 1):
    """B contracts on n_steps equal steps over half a year, every second step
    monitored (maturity included), exercise at every step."""
    from finite_difference_amd import mc_american
    rng = np.random.default_rng(seed)
    T = 0.5
    t = [T * k / n_steps for k in range(1, n_steps + 1)]
    plans = []
    for k in range(B):
        kind = KINDS[k % len(KINDS)]
        scale = float(rng.uniform(0.9, 1.1))
        plans.append(mc_american.plan_american_contract(
            spot=100.0 * scale, strike=100.0 * scale * float(rng.uniform(0.95, 1.05)), vol=0.3,
            option_type="put" if (k // len(KINDS)) % 2 == 0 else "call", discount_rate=0.05,
            carry_rate=0.03, time_to_expiry=T, barrier_type=kind,
            lower_barrier=85.0 * scale if "down" in kind or "double" in kind else None,
            upper_barrier=115.0 * scale if "up" in kind or "double" in kind else None,
            monitor_times=t[1::2], rebate_amount=1.0 if kind != "none" else 0.0,
            exercise_times=t))
    return plans


def dividend_rows(plans, n_div: int) -> np.ndarray:
    """[B, n_steps]: 0.4 % of the spot on n_div steps spread over the life."""
    B, n_steps = len(plans), plans[0].n_steps
    if not 0 <= n_div < n_steps:
        raise SystemExit("--dividends must be in 0 .. steps - 1")
    rows = np.zeros((B, n_steps))
    at = [((k + 1) * n_steps) // (n_div + 1) - 1 for k in range(n_div)]
    for b, c in enumerate(plans):
        rows[b, at] = 0.004 * float(c.params[0])
    return rows


def device_run(plans, G: int, launches: int, warmup: int, seed: int, div=None):
    import torch
    from finite_difference_amd import capi, mc_american
    capi.require_device()
    dev = torch.device("cuda:0")
    B, n_steps = len(plans), plans[0].n_steps
    P, F, S = mc_american._stack(plans, list(range(B)))
    dP, dF, dS = (torch.from_numpy(a).to(dev) for a in (P, F, S))
    dD = torch.from_numpy(np.ascontiguousarray(div)).to(dev) if div is not None else None
    stats = torch.zeros((B, capi.LSM_NSTAT), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_lsm_plan(n_steps, G, True)["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def launch():
        if dD is not None:
            capi.mc_lsm_div_batch_dev(B, n_steps, G, True, dP.data_ptr(), dF.data_ptr(),
                                      dS.data_ptr(), dD.data_ptr(), seed, 0, stats.data_ptr(),
                                      None, None, ws.data_ptr(), ws_bytes, stream.cuda_stream)
            return
        capi.mc_lsm_batch_dev(B, n_steps, G, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
                              seed, 0, stats.data_ptr(), None, None, ws.data_ptr(), ws_bytes,
                              stream.cuda_stream)
    times = []
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            launch()
        stream.synchronize()
        for _ in range(launches):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            launch()
            t1.record(stream)
            t1.synchronize()
            times.append(t0.elapsed_time(t1) * 1e-3)
    return times, stats.cpu().numpy(), torch.cuda.get_device_name(0)


def host_run(plans, G: int, seed: int):
    from finite_difference_amd import capi, mc_american
    threads = max(1, int(os.environ.get("OMP_NUM_THREADS", "1")))

    def one(job):
        b, g = job
        r = mc_american.host_subruns(plans[b], [g], True, seed, b)
        return float(r["values"].sum()) / capi.LSM_SUBRUN
    jobs = [(b, g) for b in range(len(plans)) for g in range(G)]
    one(jobs[0])  # warm-up
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=threads) as ex:
        list(ex.map(one, jobs))
    secs = time.perf_counter() - t0
    steps = 3 * len(jobs) * capi.LSM_SUBRUN * plans[0].n_steps
    return {"contracts": len(plans), "subruns": G, "threads": threads, "seconds": secs,
            "path_steps_per_s": steps / secs}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--contracts", type=int, default=1024)
    ap.add_argument("--subruns", type=int, default=32)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host-contracts", type=int, default=7)
    ap.add_argument("--host-subruns", type=int, default=4)
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    ap.add_argument("--dividends", type=int, default=0, metavar="N",
                    help="also time the dividend instance with N dividend steps per contract")
    args = ap.parse_args()

    from finite_difference_amd import capi
    plans = build_batch(args.contracts, args.steps)
    times, stats, name = device_run(plans, args.subruns, args.launches, args.warmup, args.seed)
    med = statistics.median(times)
    paths = args.contracts * args.subruns * capi.LSM_SUBRUN
    rate = 3.0 * paths * args.steps / med
    host = host_run(plans[:args.host_contracts], args.host_subruns, args.seed)
    line = {
        "metric": "mc_lsm_path_steps_per_s",
        "value": rate,
        "device": name,
        "contracts": args.contracts, "subruns": args.subruns, "n_steps": args.steps,
        "paths_per_launch": paths, "passes": 3, "antithetic": True,
        "launch_seconds": {"median": med, "min": min(times), "max": max(times),
                           "launches": args.launches, "warmup": args.warmup},
        "contracts_per_s": args.contracts / med,
        "host_engine": host,
        "speedup_over_host_engine": rate / host["path_steps_per_s"],
        "invalid_fit_steps": float(stats[:, capi.LSM_O_INVALID].sum()),
        "price_range": [float(stats[:, 0].min()), float(stats[:, 0].max())],
    }
    if args.dividends:
        rows = dividend_rows(plans, args.dividends)
        dt, dstats, _ = device_run(plans, args.subruns, args.launches, args.warmup, args.seed,
                                   div=rows)
        dmed = statistics.median(dt)
        line["dividends"] = {
            "steps_with_a_dividend": args.dividends,
            "launch_seconds": {"median": dmed, "min": min(dt), "max": max(dt)},
            "plain_launch_seconds_median": med,
            "ratio_to_plain": dmed / med,
            "price_range": [float(dstats[:, 0].min()), float(dstats[:, 0].max())],
        }
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "mc_lsm_stats.npy"), stats)
        line["dumped"] = {"mc_lsm_stats": list(stats.shape)}
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
