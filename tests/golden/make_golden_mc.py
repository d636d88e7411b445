"""Generate the Monte Carlo barrier fixtures from the reference code.

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER, where the reference is mounted
read-only at /root/reference (as make_golden.py).  Nothing on the GPU box
runs it; the tests read what it wrote next to itself:

  mc_cases.json  inputs, per-step arrays, the reference's result dict
  mc_cases.npz   "z<n_steps>": the normals default_rng(seed) gives the
                 reference for a 1024-observation case of n_steps steps (all
                 small cases share one seed, so one array per step count);
                 "payoff_<case>": the reference's per-observation payoffs

The reference's path functional (simulate_payoffs) is a closure of
price_discrete_barrier_mc.  Its output is taken where the function sums it:
with chunk_size >= n_obs the whole vector p goes through one `np.sum(p)`, and
the module is run with an `np` that records that argument.

The per-step arrays are this package's (mc_barrier.plan_contract); the
reference keeps its own as locals.  They are tied to the reference through
the payoffs: the generator asserts that the host engine on these arrays and
normals reproduces every reference payoff bit for bit.

Small cases must not sit on a decision edge: no monitored spot within 1e-9
relative of its threshold and no terminal spot within 1e-9 relative of the
strike (asserted below), so an ulp of the device exp cannot flip a payoff.

Usage:  python tests/golden/make_golden_mc.py
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # repository root

import mc_fixture  # noqa: E402

N_OBS = 1024
SEED = 20250728
EDGE = 1e-9


class _NumpyTap:
    """numpy, except that the first array handed to sum() is kept."""

    def __init__(self):
        self.first = None

    def __getattr__(self, name):
        return getattr(np, name)

    def sum(self, a, *args, **kw):
        if self.first is None:
            self.first = np.array(a, dtype=float, copy=True)
        return np.sum(a, *args, **kw)


def load_reference():
    sys.path.insert(0, REF)
    import mc_discrete_barrier_option as ref  # type: ignore
    return ref


def reference_run(ref, inputs, tap_payoffs):
    kw = mc_fixture.kwargs_for(inputs, ref)
    tap = _NumpyTap()
    if tap_payoffs:
        ref.np = tap
    try:
        t0 = time.perf_counter()
        out = ref.price_discrete_barrier_mc(**kw)
        secs = time.perf_counter() - t0
    finally:
        ref.np = np
    out = dict(out)
    out["ci_95"] = list(out["ci_95"])
    return out, tap.first, secs


def base_inputs(**over):
    inputs = dict(
        spot=229.74, strike=220.0, vol=0.26, option_type="call", rate=0.073086,
        valuation="2025-07-28", maturity="2025-08-28",
        dividends=[["2025-08-15", 1.5]],
        monitor_dates=["2025-08-04", "2025-08-07", "2025-08-12", "2025-08-18", "2025-08-22",
                       "2025-08-27"],
        barrier=dict(type="none", level=None, tol_bps=0.0, abs_tol=0.0),
        rebate=dict(amount=0.0, at_hit=False),
        cfg=dict(n_paths=2 * N_OBS, seed=SEED, antithetic=True, chunk_size=4 * N_OBS,
                 dividend_before_monitor=True, spot_floor=1e-12),
        include_maturity_monitor=True)
    for k, v in over.items():
        if isinstance(v, dict):
            inputs[k] = {**inputs[k], **v}
        else:
            inputs[k] = v
    if not inputs["cfg"]["antithetic"]:
        inputs["cfg"]["n_paths"] = N_OBS
    return inputs


WITH_DIV_DATE = ["2025-08-04", "2025-08-07", "2025-08-12", "2025-08-15", "2025-08-18",
                 "2025-08-22", "2025-08-27"]
THREE = dict(dividends=[], monitor_dates=["2025-08-12", "2025-08-22"])
ONE = dict(dividends=[], monitor_dates=[])


def small_cases():
    up = dict(type="up-and-out", level=250.0)
    down = dict(type="down-and-out", level=224.0)
    return [
        ("none_call_8", base_inputs()),
        ("none_put_1", base_inputs(option_type="put", cfg=dict(antithetic=False), **ONE)),
        ("uo_call_rebate_maturity_8", base_inputs(barrier=up, rebate=dict(amount=2.0))),
        ("uo_call_rebate_hit_8", base_inputs(barrier=up, rebate=dict(amount=2.0, at_hit=True),
                                             cfg=dict(antithetic=False))),
        ("do_call_div_first_8", base_inputs(barrier={**down, "tol_bps": 1.0},
                                            rebate=dict(amount=1.0, at_hit=True),
                                            monitor_dates=WITH_DIV_DATE)),
        ("do_call_div_last_8", base_inputs(barrier={**down, "tol_bps": 1.0},
                                           rebate=dict(amount=1.0, at_hit=True),
                                           monitor_dates=WITH_DIV_DATE,
                                           cfg=dict(dividend_before_monitor=False))),
        ("di_call_3", base_inputs(barrier=dict(type="down-and-in", level=222.0), **THREE)),
        ("ui_put_8", base_inputs(option_type="put", barrier=dict(type="up-and-in", level=240.0),
                                 cfg=dict(antithetic=False))),
        ("uo_call_no_maturity_monitor_8", base_inputs(barrier=up,
                                                      rebate=dict(amount=2.0, at_hit=True),
                                                      include_maturity_monitor=False)),
        ("do_put_1", base_inputs(option_type="put", strike=235.0,
                                 barrier=dict(type="down-and-out", level=215.0, tol_bps=1.0),
                                 rebate=dict(amount=0.5), **ONE)),
    ]


def assert_off_the_edges(name, plan, Z, antithetic):
    """No monitored spot within EDGE of the threshold, no terminal spot within
    EDGE of the strike (both signs of Z with antithetic)."""
    from finite_difference_amd import capi
    spot, strike, _, thr = (float(v) for v in plan.params[:4])
    kind = int(plan.flags[capi.MC_F_KIND])
    div_first = bool(plan.flags[capi.MC_F_DIV_FIRST])
    floor = float(plan.params[capi.MC_P_FLOOR])
    gap = np.inf
    for sign in ((1.0, -1.0) if antithetic else (1.0,)):
        s = np.full(Z.shape[0], spot)
        for i, row in enumerate(plan.step):
            s = s * np.exp(row[0] + row[1] * (sign * Z[:, i]))
            if div_first and row[2] != 0.0:
                s = np.maximum(s - row[2], floor)
            if kind != 0 and row[3] != 0.0:
                gap = min(gap, float(np.min(np.abs(s - thr))) / thr)
            if not div_first and row[2] != 0.0:
                s = np.maximum(s - row[2], floor)
        gap = min(gap, float(np.min(np.abs(s - strike))) / strike)
    assert gap > EDGE, (name, gap)
    return gap


def main():
    from finite_difference_amd import mc_barrier
    ref = load_reference()
    arrays, small = {}, []
    for name, inputs in small_cases():
        out, payoffs, _ = reference_run(ref, inputs, tap_payoffs=True)
        assert out["n_observations"] == N_OBS and payoffs.shape == (N_OBS,)
        n_steps = out["steps"]
        Z = np.random.default_rng(SEED).standard_normal(size=(N_OBS, n_steps))
        key = f"z{n_steps}"
        if key in arrays:
            assert np.array_equal(arrays[key], Z)
        arrays[key] = Z
        arrays[f"payoff_{name}"] = payoffs
        plan = mc_barrier.plan_contract(**mc_fixture.kwargs_for(inputs, mc_barrier))
        anti = inputs["cfg"]["antithetic"]
        gap = assert_off_the_edges(name, plan, Z, anti)
        mine = mc_barrier.simulate([plan], N_OBS, anti, engine="host", z=Z, want_payoffs=True)[1]
        assert np.array_equal(mine[0], payoffs), name
        print(f"{name}: steps {n_steps} price {out['price']:.6f} +- {out['stderr']:.6f} "
              f"nonzero {int(np.count_nonzero(payoffs))} edge gap {gap:.2e}")
        small.append(dict(name=name, inputs=inputs, step=plan.step.tolist(),
                          params=plan.params.tolist(), flags=plan.flags.tolist(),
                          normals=key, payoffs=f"payoff_{name}", result=out))
    large = []
    big = dict(n_paths=4_000_000, seed=7, antithetic=True, chunk_size=50_000)
    for name, inputs in [
            ("uo_call_rebate_maturity_4m", base_inputs(barrier=dict(type="up-and-out", level=250.0),
                                                       rebate=dict(amount=2.0), cfg=big)),
            ("vanilla_put_4m", base_inputs(option_type="put", dividends=[], cfg=big))]:
        out, _, secs = reference_run(ref, inputs, tap_payoffs=False)
        print(f"{name}: price {out['price']:.6f} +- {out['stderr']:.6f} n {out['n_observations']} "
              f"reference {secs:.2f} s")
        large.append(dict(name=name, inputs=inputs, result=out, reference_seconds=round(secs, 2)))
    with open(os.path.join(HERE, "mc_cases.json"), "w") as f:
        json.dump(dict(generator="tests/golden/make_golden_mc.py", n_obs=N_OBS, edge=EDGE,
                       small=small, large=large), f, indent=1)
    np.savez(os.path.join(HERE, "mc_cases.npz"), **arrays)
    for fn in ("mc_cases.json", "mc_cases.npz"):
        size = os.path.getsize(os.path.join(HERE, fn))
        print(fn, size, "bytes")
        assert size <= 300 * 1024, fn


if __name__ == "__main__":
    main()
