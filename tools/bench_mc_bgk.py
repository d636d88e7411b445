#!/usr/bin/env python3
"""Throughput of the BGK barrier pricer's path kernel (csrc/fdcn_mc_bgk.hip).

Device: B trades x G = 5 scenarios (the Greeks ladder) x n_obs antithetic
observations x 8 steps, normals generated in the kernel, every array resident
on the device, through fdcn_mc_bgk_batch_dev with a planned workspace.
Warm-up, then `--launches` launches timed one by one with device events; the
median is the result.  A scenario-path-step is one `c += drift + diff z` of
one scenario on one path, with its share of the monitor tests and the payoff.

Three rates:
  grouped    the G = 5 launch: an observation's normals are drawn once for
             the five scenarios and both signs
  ungrouped  the same work as 5 B rows at G = 1 (each row draws its own)
  host       the NumPy host engine in this process, `--host-trades` ladders on
             the CPUs the process may use (at most 16), on the same Philox
             streams; its prices check the grouped launch's

The static fp64 count (tools/isa_stats.py FILE.s --kernel
bgk_path_kernelILi5ELb1ELb1E and ...ILi1ELb1ELb1E, FMA = 2) covers one
observation with the step loop rolled: one Box-Muller pair, one step of every
scenario on both signs with its monitor test, and the payoffs.  The kernel
moves no data, so the roof is fp64 VALU issue.

Writes profiles/mc/bench_mc_bgk.json and prints the same JSON line.  Without a
GPU it fails; there is no fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

G = 5
# isa_stats.py, observation loop of bgk_path_kernel<G, true, true>, FMA = 2
F64_OPS_OBS_LOOP = {1: 452, 5: 1660}
PEAK_F64_VALU = 78.6e12         # MI355X vector fp64, FLOP/s
MONITORS = ["2025-08-04", "2025-08-07", "2025-08-12", "2025-08-15", "2025-08-18", "2025-08-22",
            "2025-08-27"]       # with maturity: eight steps, seven monitored


def build_batch(B: int, seed: int = 1):
    """B Greeks ladders (five scenarios each) on an eight-step grid: up-, down-
    and double-out, smoothed and exact, the three rebate modes in turn; spot,
    strike and levels spread by a seeded draw."""
    import copy
    import bgk_fixture as fx
    from finite_difference_amd import capi
    from finite_difference_amd.bgk_barrier import DiscreteBarrierBGKPricer
    cases = {c["name"]: c for c in fx.load_cases()["paths"]}
    pool = []
    for name, over in (("uo_call_smooth_7", {}),
                       ("dbl_out_call_smooth_rebate_hit_7", {}),
                       ("do_put_exact_rebate_hit_7", {}),
                       ("dbl_out_put_exact_rebate_expiry_3", {}),
                       ("dbl_in_call_smooth_7", dict(mc_smooth_payoff_eps=0.0))):
        kw = {**fx.kwargs_for({**cases[name]["inputs"], "monitor_dates": MONITORS}), **over}
        p = DiscreteBarrierBGKPricer(engine="host", **kw)
        pool.append([j.plan for j in p._bumped_jobs(1e-4 * p.spot_price, 1e-4)])
        assert all(pl.n_steps == 8 for pl in pool[-1])
    rng = np.random.default_rng(seed)
    groups = []
    for k in range(B):
        scale = float(rng.uniform(0.9, 1.1))
        grp = copy.deepcopy(pool[k % len(pool)])
        for pl in grp:
            pl.params[capi.BGK_P_LOG_SPOT] += np.log(scale)
            for idx in (capi.BGK_P_STRIKE, capi.BGK_P_UPPER, capi.BGK_P_LOWER):
                pl.params[idx] *= scale
        groups.append(grp)
    return groups


def stack(groups, stream_ids):
    from finite_difference_amd import capi
    P = np.stack([np.stack([p.params for p in grp]) for grp in groups])
    S = np.stack([np.stack([p.step for p in grp]) for grp in groups])
    F = np.stack([grp[0].flags for grp in groups]).astype(np.int32)
    F[:, capi.BGK_F_STREAM] = np.asarray(stream_ids, dtype=np.int32)
    return P, F, S


def device_run(groups, stream_ids, n_obs: int, launches: int, warmup: int, seed: int):
    import torch
    from finite_difference_amd import capi
    capi.require_device()
    dev = torch.device("cuda:0")
    P, F, S = stack(groups, stream_ids)
    B, g, n_steps = P.shape[0], P.shape[1], S.shape[2]
    dP, dF, dS = (torch.from_numpy(a).to(dev) for a in (P, F, S))
    stats = torch.zeros((B, g, capi.BGK_NSTAT), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_bgk_plan(n_obs, g)["ws_bytes_per_trade"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def launch():
        capi.mc_bgk_batch_dev(B, g, n_steps, n_obs, True, dP.data_ptr(), dF.data_ptr(),
                              dS.data_ptr(), None, seed, 0, stats.data_ptr(), None,
                              ws.data_ptr(), ws_bytes, stream.cuda_stream)
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


def host_run(groups, n_obs: int, seed: int):
    """The host engine on the first ladders, on the device's Philox streams."""
    from finite_difference_amd import bgk_barrier
    cpus = min(16, len(os.sched_getaffinity(0)))

    def one(item):
        b, grp = item
        return bgk_barrier.run_paths([grp], engine="host", seed=seed, stream_ids=[b],
                                     n_obs=n_obs)[0]
    one((0, groups[0]))  # warm-up
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=cpus) as ex:
        stats = list(ex.map(one, enumerate(groups)))
    secs = time.perf_counter() - t0
    steps = len(groups) * G * n_obs * 2 * groups[0][0].n_steps
    return np.stack(stats), {"trades": len(groups), "n_obs": n_obs, "threads": cpus,
                             "seconds": secs, "scenario_path_steps_per_s": steps / secs}


def summary(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times),
            "launches": len(times)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--trades", type=int, default=4096)
    ap.add_argument("--obs", type=int, default=1 << 16, help="observations per trade")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host-trades", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc", "bench_mc_bgk.json"))
    args = ap.parse_args()

    from finite_difference_amd.bgk_barrier import compose
    groups = build_batch(args.trades)
    n_steps = groups[0][0].n_steps
    B = len(groups)
    work = B * G * args.obs * 2 * n_steps          # scenario-path-steps per launch
    t5, stats, name = device_run(groups, list(range(B)), args.obs, args.launches, args.warmup,
                                 args.seed)
    # the same work as 5 B single-scenario rows; row (b, g) keeps trade b's stream
    rows = [[grp[g]] for grp in groups for g in range(G)]
    ids = [b for b in range(B) for _ in range(G)]
    t1, stats1, _ = device_run(rows, ids, args.obs, args.launches, args.warmup, args.seed)
    same = bool(np.array_equal(stats.reshape(-1, 4).view(np.uint64),
                               stats1.reshape(-1, 4).view(np.uint64)))
    host_stats, host = host_run(groups[:args.host_trades], args.obs, args.seed)
    worst = 0.0
    n_sim = 2 * args.obs
    for b in range(args.host_trades):
        for g in range(G):
            got = compose(groups[b][g], n_sim, *stats[b, g, :3])[0]
            want = compose(groups[b][g], n_sim, *host_stats[b, g, :3])[0]
            worst = max(worst, abs(got - want) / max(abs(want), 1e-300))
    med5, med1 = statistics.median(t5), statistics.median(t1)
    rate5, rate1 = work / med5, work / med1
    steps_per_obs = 2 * n_steps
    ops5 = F64_OPS_OBS_LOOP[5] / (G * 2)            # static, per scenario-path of the loop body
    line = {
        "metric": "mc_bgk_scenario_path_steps_per_s",
        "value": rate5,
        "device": name,
        "trades": B, "G": G, "n_obs": args.obs, "n_steps": n_steps, "antithetic": True,
        "rng": "philox", "warmup": args.warmup,
        "grouped": {"launch_seconds": summary(t5), "scenario_path_steps_per_s": rate5},
        "ungrouped": {"rows": B * G, "launch_seconds": summary(t1),
                      "scenario_path_steps_per_s": rate1,
                      "sums_bitwise_equal_to_grouped": same},
        "grouped_over_ungrouped": rate5 / rate1,
        "host_engine": host,
        "speedup_over_host_engine": rate5 / host["scenario_path_steps_per_s"],
        "static_f64": {"source": "tools/isa_stats.py, observation loop, FMA = 2, step loop rolled",
                       "ops_obs_loop": F64_OPS_OBS_LOOP,
                       "ops_per_scenario_path_of_loop_body_G5": ops5,
                       "steps_per_observation": steps_per_obs},
        "parity": {"trades": args.host_trades, "worst_rel_price_diff": worst, "bound": 1e-9,
                   "ok": bool(worst <= 1e-9)},
    }
    text = json.dumps(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 0 if line["parity"]["ok"] and same else 3


if __name__ == "__main__":
    sys.exit(main())
