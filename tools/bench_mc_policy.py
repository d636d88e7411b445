#!/usr/bin/env python3
"""Throughput of the table-policy Monte Carlo kernels (csrc/fdcn_mc_policy.hip)
beside the least-squares kernels they stand next to.

Device: bench_mc_lsm.py's batch -- `--contracts` contracts (the seven barrier
kinds in turn, spot and strike spread by a seeded draw) x `--subruns` sub-runs x
4 096 paths x `--steps` steps, antithetic, every array resident on the device --
under a synthetic threshold table: a put stops at and below 0.9 strike, a call
at and above 1.1 strike, at every step.  fdcn_mc_policy_batch_dev with a
planned workspace: warm-up, `--launches` launches timed one by one with device
events, the median is the result; then fdcn_mc_lsm_batch_dev on the same batch
in the same way.  The unit is the nominal path-step, paths x steps of one
forward pass: a path that has stopped walks no further, so the work done is
less, by the share the table stops early.  The LSM launch makes three passes
(bench_mc_lsm.py counts 3 x paths x steps); the record carries both launch
times and their ratio.

Yardstick, same process: the NumPy host engine (mc_american.host_policy_subruns)
on the first `--host-contracts` contracts x `--host-subruns` sub-runs.

--dual also times fdcn_mc_policy_dual_batch_dev beside
fdcn_mc_lsm_dual_batch_dev (under the coefficients the LSM launch has just
fitted), each in inner path-steps as the kernels count them.

--dividends N puts a cash dividend on N steps of every contract
(bench_mc_lsm.py's rows: 0.4 % of the spot, spread over the life, none on the
last step) and times fdcn_mc_policy_div_batch_dev -- with --dual also
fdcn_mc_policy_dual_div_batch_dev and fdcn_mc_lsm_dual_div_batch_dev, under the
same table and coefficients -- beside the plain launches, in the same process;
the record carries the launch times and their ratios to the plain ones.

Prints one JSON line.  --dump-outputs DIR writes the stats of the last timed
launches as DIR/mc_policy_stats.npy (and mc_policy_dual_stats.npy).  Without a
GPU it fails; there is no fallback.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mc_lsm import build_batch, dividend_rows  # noqa: E402


def threshold_policies(plans):
    from finite_difference_amd import capi, mc_american
    out = []
    for c in plans:
        M, k = c.n_steps, float(c.params[capi.LSM_P_STRIKE])
        if c.flags[capi.LSM_F_PUT]:
            out.append(mc_american.ExercisePolicy(np.full(M, -np.inf), np.full(M, np.log(0.9 * k))))
        else:
            out.append(mc_american.ExercisePolicy(np.full(M, np.log(1.1 * k)), np.full(M, np.inf)))
    return out


def _timed(stream, launch, launches: int, warmup: int):
    import torch
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
    return times


def device_run(plans, pols, G: int, launches: int, warmup: int, seed: int, dual, div=None):
    import torch
    from finite_difference_amd import capi, mc_american
    capi.require_device()
    dev = torch.device("cuda:0")
    B, n_steps = len(plans), plans[0].n_steps
    P, F, S = mc_american._stack(plans, list(range(B)))
    T = np.stack([p.table() for p in pols])
    dP, dF, dS, dT = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, F, S, T))
    stats = torch.zeros((B, capi.POLICY_NSTAT), dtype=torch.float64, device=dev)
    lsm_stats = torch.zeros((B, capi.LSM_NSTAT), dtype=torch.float64, device=dev)
    coef = torch.zeros((B, G, n_steps, capi.LSM_NCOEF), dtype=torch.float64, device=dev)
    per = [capi.mc_policy_plan(n_steps, G, True)["ws_bytes_per_contract"],
           capi.mc_lsm_plan(n_steps, G, True)["ws_bytes_per_contract"]]
    if dual:
        per.append(capi.mc_policy_dual_plan(n_steps, G, True, *dual)["ws_bytes_per_contract"])
    ws_bytes = max(per) * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    head = (B, n_steps, G, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr())
    tail = (ws.data_ptr(), ws_bytes, stream.cuda_stream)

    def policy():
        capi.mc_policy_batch_dev(*head, dT.data_ptr(), seed, 0, stats.data_ptr(), None, *tail)

    def lsm():
        capi.mc_lsm_batch_dev(*head, seed, 0, lsm_stats.data_ptr(), None, coef.data_ptr(), *tail)
    out = {"policy": _timed(stream, policy, launches, warmup),
           "lsm": _timed(stream, lsm, launches, warmup),
           "stats": stats.cpu().numpy(), "lsm_stats": lsm_stats.cpu().numpy(),
           "device": torch.cuda.get_device_name(0)}
    if dual:
        n_outer, n_inner = dual
        dstats = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
        fstats = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
        dhead = (B, n_steps, G, True, n_outer, n_inner, dP.data_ptr(), dF.data_ptr(),
                 dS.data_ptr())

        def policy_dual():
            capi.mc_policy_dual_batch_dev(*dhead, dT.data_ptr(), seed, 0, dstats.data_ptr(), None,
                                          None, *tail)

        def fitted_dual():
            capi.mc_dual_batch_dev(*dhead, coef.data_ptr(), seed, 0, fstats.data_ptr(), None, None,
                                   *tail)
        out["policy_dual"] = _timed(stream, policy_dual, launches, warmup)
        out["fitted_dual"] = _timed(stream, fitted_dual, launches, warmup)
        out["dual_stats"], out["fitted_dual_stats"] = dstats.cpu().numpy(), fstats.cpu().numpy()
    if div is not None:  # after every plain launch, so that those are the runs without the flag
        dD = torch.from_numpy(np.ascontiguousarray(div)).to(dev)
        vstats = torch.zeros((B, capi.POLICY_NSTAT), dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        def policy_div():
            capi.mc_policy_div_batch_dev(*head, dD.data_ptr(), dT.data_ptr(), seed, 0,
                                         vstats.data_ptr(), None, *tail)
        out["policy_div"] = _timed(stream, policy_div, launches, warmup)
        out["div_stats"] = vstats.cpu().numpy()
        if dual:
            vd = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
            vf = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
            torch.cuda.synchronize()

            def policy_dual_div():
                capi.mc_policy_dual_div_batch_dev(*dhead, dD.data_ptr(), dT.data_ptr(), seed, 0,
                                                  vd.data_ptr(), None, None, *tail)

            def fitted_dual_div():
                capi.mc_dual_div_batch_dev(*dhead, dD.data_ptr(), coef.data_ptr(), seed, 0,
                                           vf.data_ptr(), None, None, *tail)
            out["policy_dual_div"] = _timed(stream, policy_dual_div, launches, warmup)
            out["fitted_dual_div"] = _timed(stream, fitted_dual_div, launches, warmup)
            out["dual_div_stats"], out["fitted_dual_div_stats"] = vd.cpu().numpy(), vf.cpu().numpy()
    return out


def host_run(plans, pols, G: int, seed: int):
    from finite_difference_amd import capi, mc_american
    mc_american.host_policy_subruns(plans[0], pols[0], [0], True, seed, 0)  # warm-up
    t0 = time.perf_counter()
    for b, (c, pol) in enumerate(zip(plans, pols)):
        mc_american.host_policy_subruns(c, pol, range(G), True, seed, b)
    secs = time.perf_counter() - t0
    steps = len(plans) * G * capi.LSM_SUBRUN * plans[0].n_steps
    return {"contracts": len(plans), "subruns": G, "threads": 1, "seconds": secs,
            "path_steps_per_s": steps / secs}


def _secs(times, launches, warmup):
    return {"median": statistics.median(times), "min": min(times), "max": max(times),
            "launches": launches, "warmup": warmup}


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
    ap.add_argument("--dual", action="store_true",
                    help="also time the table-policy dual beside the fitted dual")
    ap.add_argument("--outer", type=int, default=8)
    ap.add_argument("--inner", type=int, default=2048)
    ap.add_argument("--dump-outputs", default="", metavar="DIR")
    ap.add_argument("--dividends", type=int, default=0, metavar="N",
                    help="also time the dividend instances with N dividend steps per contract")
    args = ap.parse_args()

    from finite_difference_amd import capi
    plans = build_batch(args.contracts, args.steps)
    pols = threshold_policies(plans)
    r = device_run(plans, pols, args.subruns, args.launches, args.warmup, args.seed,
                   (args.outer, args.inner) if args.dual else None,
                   dividend_rows(plans, args.dividends) if args.dividends else None)
    med, lsm_med = statistics.median(r["policy"]), statistics.median(r["lsm"])
    paths = args.contracts * args.subruns * capi.LSM_SUBRUN
    rate = paths * args.steps / med
    nh = min(args.host_contracts, args.contracts)
    host = host_run(plans[:nh], pols[:nh], min(args.host_subruns, args.subruns), args.seed)
    stats = r["stats"]
    line = {
        "metric": "mc_policy_path_steps_per_s",
        "value": rate,
        "device": r["device"],
        "contracts": args.contracts, "subruns": args.subruns, "n_steps": args.steps,
        "paths_per_launch": paths, "passes": 1, "antithetic": True,
        "policy": "put: x <= ln(0.9 strike); call: x >= ln(1.1 strike); every step",
        "launch_seconds": _secs(r["policy"], args.launches, args.warmup),
        "contracts_per_s": args.contracts / med,
        "paths_stopped_by_the_table": float(stats[:, capi.POLICY_O_EXERCISED].sum()) / paths,
        "lsm_launch": {"launch_seconds": _secs(r["lsm"], args.launches, args.warmup),
                       "passes": 3, "path_steps_per_s": 3.0 * paths * args.steps / lsm_med,
                       "seconds_over_policy_launch": lsm_med / med},
        "host_engine": host,
        "speedup_over_host_engine": rate / host["path_steps_per_s"],
        "price_range": [float(stats[:, 0].min()), float(stats[:, 0].max())],
        "median_policy_over_lsm_price": float(np.median(
            stats[:, 0] / np.maximum(r["lsm_stats"][:, capi.LSM_O_PRICE], 1e-300))),
    }
    if args.dual:
        d, f = r["dual_stats"], r["fitted_dual_stats"]
        dm, fm = statistics.median(r["policy_dual"]), statistics.median(r["fitted_dual"])
        ds = float(d[:, capi.DUAL_O_INNER_STEPS].sum())
        fs = float(f[:, capi.DUAL_O_INNER_STEPS].sum())
        line["dual"] = {
            "n_outer": args.outer, "n_inner": args.inner,
            "policy": {"launch_seconds": _secs(r["policy_dual"], args.launches, args.warmup),
                       "inner_path_steps_per_launch": ds, "inner_path_steps_per_s": ds / dm,
                       "gap_range": [float(d[:, 0].min()), float(d[:, 0].max())]},
            "fitted": {"launch_seconds": _secs(r["fitted_dual"], args.launches, args.warmup),
                       "inner_path_steps_per_launch": fs, "inner_path_steps_per_s": fs / fm,
                       "gap_range": [float(f[:, 0].min()), float(f[:, 0].max())]},
        }
    if args.dividends:
        vm = statistics.median(r["policy_div"])
        line["dividends"] = {
            "steps_with_a_dividend": args.dividends,
            "launch_seconds": _secs(r["policy_div"], args.launches, args.warmup),
            "plain_launch_seconds_median": med,
            "ratio_to_plain": vm / med,
            "price_range": [float(r["div_stats"][:, 0].min()), float(r["div_stats"][:, 0].max())],
        }
        if args.dual:
            for key, plain in (("policy_dual", dm), ("fitted_dual", fm)):
                t = r[key + "_div"]
                st = r[("dual_div_stats" if key == "policy_dual" else "fitted_dual_div_stats")]
                steps = float(st[:, capi.DUAL_O_INNER_STEPS].sum())
                line["dividends"][key] = {
                    "launch_seconds": _secs(t, args.launches, args.warmup),
                    "plain_launch_seconds_median": plain,
                    "ratio_to_plain": statistics.median(t) / plain,
                    "inner_path_steps_per_launch": steps,
                    "inner_path_steps_per_s": steps / statistics.median(t)}
    if args.dump_outputs:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "mc_policy_stats.npy"), stats)
        line["dumped"] = {"mc_policy_stats": list(stats.shape)}
        if args.dual:
            np.save(os.path.join(args.dump_outputs, "mc_policy_dual_stats.npy"), r["dual_stats"])
            line["dumped"]["mc_policy_dual_stats"] = list(r["dual_stats"].shape)
    print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
