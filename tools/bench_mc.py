#!/usr/bin/env python3
"""Throughput of the Monte Carlo discrete-barrier pricer (csrc/fdcn_mc.hip).

Device: B contracts x n_obs observations x n_steps steps, antithetic, normals
generated in the kernel (rng="philox"), every array resident on the device,
through fdcn_mc_barrier_batch_dev with a planned workspace.  Warm-up, then
`--launches` launches timed one by one with device events; the median is the
result.  A path-step is one `s *= exp(drift + diff z)` with its dividend and
barrier test; an antithetic observation walks two paths.

Yardstick, same process: the host engine (NumPy, the reference's operation
order, default_rng normals) pricing `--host-contracts` contracts concurrently
on the CPUs the process may use (at most 16).  The reference's own recorded
time for one contract (tests/golden/mc_cases.json) is quoted beside it.

Roofline: the kernel moves no data, so the roof is fp64 VALU issue.  The fp64
operations per path-step are a static count of the kernel's inner loop
(tools/isa_stats.py FILE.s --kernel mc_path_kernelILb1ELb1E: one iteration is
one Philox block, one Box-Muller pair and four path-steps), an FMA as two.

--rng sobol times, after the Philox kernel and in the same process, the same
workload through the quasi-Monte Carlo kernel (csrc/fdcn_mc_qmc.hip,
fdcn_mc_qmc_batch_dev): `--replicates` shifted Sobol point sets of
obs / replicates points each, Brownian-bridge construction, antithetic -- the
same number of path-steps -- and reports it under "qmc" beside the Philox
figure, with each kernel's mean standard error over the batch.  The default,
--rng philox, runs and prints what it always did.

Prints one JSON line.  --dump-outputs DIR writes the prices of the last
timed launch as DIR/mc_stats.npy.  Without a GPU it fails; there is no
fallback.
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

F64_OPS_PER_LOOP = 309          # isa_stats.py, mc_path_kernel<true, true>, FMA = 2
PATH_STEPS_PER_LOOP = 4         # two steps x two antithetic paths
PEAK_F64_VALU = 78.6e12         # MI355X vector fp64, FLOP/s


def build_batch(B: int, seed: int = 1):
    """B contracts on the eight-step grid of the fixtures' base trade: the five
    barrier kinds in turn, spot / strike / level spread by a seeded draw."""
    import mc_fixture as fx
    from finite_difference_amd import capi, mc_barrier
    cases = fx.load_cases()["small"]
    base = [mc_barrier.plan_contract(**fx.kwargs_for(c["inputs"], mc_barrier))
            for c in cases if c["result"]["steps"] == 8]
    three = next(c for c in cases if c["name"] == "di_call_3")
    di = mc_barrier.plan_contract(**fx.kwargs_for(three["inputs"], mc_barrier))
    # a down-and-in on the eight-step grid completes the five kinds
    pool = base + [mc_barrier.McContract(**{**base[0].__dict__, "params": di.params,
                                            "flags": di.flags})]
    rng = np.random.default_rng(seed)
    plans = []
    for k in range(B):
        src = pool[k % len(pool)]
        p = mc_barrier.McContract(**{**src.__dict__, "params": src.params.copy(),
                                     "flags": src.flags.copy()})
        scale = float(rng.uniform(0.9, 1.1))
        for idx in (capi.MC_P_SPOT, capi.MC_P_STRIKE, capi.MC_P_THRESHOLD):
            p.params[idx] *= scale
        plans.append(p)
    return plans


def device_run(plans, n_obs: int, launches: int, warmup: int, seed: int):
    import torch
    from finite_difference_amd import capi, mc_barrier
    capi.require_device()
    dev = torch.device("cuda:0")
    B, n_steps = len(plans), plans[0].n_steps
    P, F, S = mc_barrier._stack(plans, list(range(B)))
    dP, dF, dS = (torch.from_numpy(a).to(dev) for a in (P, F, S))
    stats = torch.zeros((B, capi.MC_NSTAT), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_plan(n_obs)["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def launch():
        capi.mc_barrier_batch_dev(B, n_steps, n_obs, True, dP.data_ptr(), dF.data_ptr(),
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


def device_run_qmc(plans, n_obs: int, replicates: int, launches: int, warmup: int, seed: int):
    """The Philox run's workload on the quasi-Monte Carlo kernel: n_obs //
    replicates points in each of `replicates` replicates."""
    import torch
    from finite_difference_amd import capi, mc_barrier
    dev = torch.device("cuda:0")
    B, n_steps = len(plans), plans[0].n_steps
    n_rep = n_obs // replicates
    P, F, S = mc_barrier._stack(plans, list(range(B)))
    dirnum, idx, bw = mc_barrier.qmc_tables(plans, "bridge")
    dP, dF, dS, dW = (torch.from_numpy(a).to(dev) for a in (P, F, S, bw))
    dD = torch.from_numpy(dirnum.view(np.int32)).to(dev)
    stats = torch.zeros((B, capi.MC_NSTAT), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_qmc_plan(n_steps, n_rep, replicates)["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def launch():
        capi.mc_qmc_batch_dev(B, n_steps, n_rep, replicates, True, True, dP.data_ptr(),
                              dF.data_ptr(), dS.data_ptr(), dD.data_ptr(), idx, dW.data_ptr(), seed,
                              0, 0, stats.data_ptr(), None, None, ws.data_ptr(), ws_bytes,
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
    return times, stats.cpu().numpy(), n_rep


def parity_qmc(plans, stats, n_rep: int, replicates: int, seed: int, count: int = 2):
    """The timed launch's prices for the first contracts against the host
    engine on the same points (qmc.py)."""
    from finite_difference_amd import mc_barrier
    worst = 0.0
    for b in range(count):
        reps = mc_barrier.simulate_qmc([plans[b]], n_rep, True, engine="host", seed=seed,
                                       stream_ids=[b], replicates=replicates, chunk_size=1 << 15)
        want = mc_barrier._qmc_stats(n_rep, reps[0, :, 0])[0]
        worst = max(worst, abs(float(stats[b, 0]) - want) / max(abs(want), 1e-300))
    return {"contracts": count, "worst_rel_price_diff": worst, "bound": 1e-9,
            "ok": bool(worst <= 1e-9)}


def parity(plans, stats, n_obs: int, seed: int, count: int = 2):
    """The timed launch's own prices for the first contracts against the host
    engine on the same Philox streams (NumPy restatement of the generator)."""
    from finite_difference_amd import mc_barrier
    worst = 0.0
    for b in range(count):
        sums = mc_barrier.simulate([plans[b]], n_obs, True, engine="host", rng="philox",
                                   seed=seed, stream_ids=[b], chunk_size=1 << 15)
        want = float(sums[0, 0]) / n_obs
        worst = max(worst, abs(float(stats[b, 0]) - want) / max(abs(want), 1e-300))
    return {"contracts": count, "worst_rel_price_diff": worst, "bound": 1e-9,
            "ok": bool(worst <= 1e-9)}


def host_run(plans, n_paths: int, seed: int):
    from finite_difference_amd import mc_barrier
    cpus = min(16, len(os.sched_getaffinity(0)))
    n_obs = n_paths // 2

    def one(p):
        return mc_barrier.simulate([p], n_obs, True, engine="host", rng="numpy", seed=seed,
                                   chunk_size=50_000)
    one(plans[0])  # warm-up
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=cpus) as ex:
        list(ex.map(one, plans))
    secs = time.perf_counter() - t0
    steps = len(plans) * n_obs * 2 * plans[0].n_steps
    return {"contracts": len(plans), "n_paths": n_paths, "threads": cpus, "seconds": secs,
            "path_steps_per_s": steps / secs}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--contracts", type=int, default=4096)
    ap.add_argument("--obs", type=int, default=1 << 17, help="observations per contract")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--host-contracts", type=int, default=16)
    ap.add_argument("--host-paths", type=int, default=1 << 20)
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    ap.add_argument("--rng", choices=("philox", "sobol"), default="philox",
                    help="sobol: also time the quasi-Monte Carlo kernel on the same workload")
    ap.add_argument("--replicates", type=int, default=16, help="with --rng sobol")
    args = ap.parse_args()

    plans = build_batch(args.contracts)
    n_steps = plans[0].n_steps
    times, stats, name = device_run(plans, args.obs, args.launches, args.warmup, args.seed)
    med = statistics.median(times)
    path_steps = args.contracts * args.obs * 2 * n_steps
    rate = path_steps / med
    flops = rate * F64_OPS_PER_LOOP / PATH_STEPS_PER_LOOP
    host = host_run(plans[:args.host_contracts], args.host_paths, args.seed)
    import mc_fixture as fx
    ref = fx.load_cases()["large"][0]
    ref_steps = ref["result"]["n_observations"] * 2 * ref["result"]["steps"]
    line = {
        "metric": "mc_barrier_path_steps_per_s",
        "value": rate,
        "device": name,
        "contracts": args.contracts, "n_obs": args.obs, "n_steps": n_steps, "antithetic": True,
        "rng": "philox",
        "launch_seconds": {"median": med, "min": min(times), "max": max(times),
                           "launches": args.launches, "warmup": args.warmup},
        "contracts_per_s": args.contracts / med,
        "roofline": {"bound": "fp64 VALU issue (no memory traffic)",
                     "f64_ops_per_path_step": F64_OPS_PER_LOOP / PATH_STEPS_PER_LOOP,
                     "source": "static ISA count of the inner loop (tools/isa_stats.py)",
                     "achieved": flops, "peak": PEAK_F64_VALU,
                     "fraction": flops / PEAK_F64_VALU},
        "host_engine": host,
        "speedup_over_host_engine": rate / host["path_steps_per_s"],
        "reference_recorded": {"case": ref["name"], "seconds": ref["reference_seconds"],
                               "path_steps_per_s": ref_steps / ref["reference_seconds"],
                               "note": "one contract, one thread, on the fixture "
                                       "generator's host"},
        "parity": parity(plans, stats, args.obs, args.seed),
        "price_range": [float(stats[:, 0].min()), float(stats[:, 0].max())],
    }
    ok = line["parity"]["ok"]
    if args.rng == "sobol":
        q_times, q_stats, n_rep = device_run_qmc(plans, args.obs, args.replicates, args.launches,
                                                 args.warmup, args.seed)
        q_med = statistics.median(q_times)
        q_rate = args.contracts * n_rep * args.replicates * 2 * n_steps / q_med
        line["qmc"] = {
            "metric": "mc_qmc_path_steps_per_s", "value": q_rate, "rng": "sobol",
            "construction": "bridge", "replicates": args.replicates, "obs_per_replicate": n_rep,
            "launch_seconds": {"median": q_med, "min": min(q_times), "max": max(q_times)},
            "relative_to_philox": q_rate / rate,
            "mean_stderr": float(q_stats[:, 1].mean()),
            "philox_mean_stderr": float(stats[:, 1].mean()),
            "stderr_ratio_philox_over_sobol": float(stats[:, 1].mean() / q_stats[:, 1].mean()),
            "parity": parity_qmc(plans, q_stats, n_rep, args.replicates, args.seed),
        }
        ok = ok and line["qmc"]["parity"]["ok"]
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "mc_stats.npy"), stats)
        line["dumped"] = {"mc_stats": list(stats.shape)}
    print(json.dumps(line))
    return 0 if ok else 3


if __name__ == "__main__":
    sys.exit(main())
