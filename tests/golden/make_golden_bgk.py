"""Generate the BGK barrier pricer's fixtures from the reference code.

THIS SCRIPT RUNS ONLY IN THE BUILD CONTAINER, where the reference is mounted
read-only at /root/reference (as make_golden_mc.py).  Nothing on the GPU box
runs it; the tests read what it wrote next to itself:

  bgk_cases.json  inputs and the reference's results: closed-form cases
                  (price, Greeks, hazard metrics, the two report strings), path
                  cases (price, standard error), two large path cases
  bgk_cases.npz   "z_numpy_<n_steps>" / "z_torch_<n_steps>": the normals the
                  reference drew for 512 observations of n_steps steps (seed
                  42); "x_<case>", "rebate_<case>": its per-path option_payoff
                  (total_payoff with a rebate at expiry) and rebate_pv

The reference keeps its per-path arrays as locals of _mc_out_price.  They are
taken where it calls np.mean, with an `np` that records those arguments.

The generator asserts that this package's host engine, on the recorded
normals, reproduces every per-path value bit for bit, and that exact-mode
cases (epsilon = 0) sit off the decision edges: no monitored spot within 1e-9
relative of a level, no terminal spot within 1e-9 relative of the strike.  The
smoothed forms are continuous at their band edges and need no such guard.

Usage:  python tests/golden/make_golden_bgk.py
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # repository root

import bgk_fixture  # noqa: E402

EDGE = 1e-9
MONITORS = ["2025-08-04", "2025-08-07", "2025-08-12", "2025-08-18", "2025-08-22", "2025-08-27"]


class _NumpyTap:
    """numpy, except that every array handed to mean() is kept."""

    def __init__(self):
        self.seen = []

    def __getattr__(self, name):
        return getattr(np, name)

    def mean(self, a, *args, **kw):
        self.seen.append(np.array(a, dtype=float, copy=True))
        return np.mean(a, *args, **kw)


def load_reference():
    sys.path.insert(0, REF)
    import discrete_barrier_bgk as ref  # type: ignore
    return ref


def base(**over):
    inputs = dict(spot=229.74, strike=220.0, volatility=0.26, rate=0.073086,
                  valuation_date="2025-07-28", maturity_date="2025-08-28", option_type="call",
                  dividend_schedule=[["2025-08-15", 1.5]], monitor_dates=list(MONITORS))
    inputs.update(over)
    return inputs


def closed_form_cases():
    levels = {"none": {}, "up-and-out": dict(upper_barrier=250.0),
              "down-and-out": dict(lower_barrier=215.0),
              "up-and-in": dict(upper_barrier=250.0), "down-and-in": dict(lower_barrier=215.0),
              "double-out": dict(lower_barrier=210.0, upper_barrier=250.0),
              "double-in": dict(lower_barrier=210.0, upper_barrier=250.0)}
    cases = []
    for bt, lv in levels.items():
        for ot in ("call", "put"):
            cases.append((f"{bt}_{ot}", base(pricing_method="bgk", barrier_type=bt,
                                             option_type=ot, **lv)))
    uo = dict(pricing_method="bgk", barrier_type="up-and-out", upper_barrier=250.0)
    do = dict(pricing_method="bgk", barrier_type="down-and-out", lower_barrier=215.0,
              option_type="put")
    dbl = dict(pricing_method="bgk", barrier_type="double-out", lower_barrier=210.0,
               upper_barrier=250.0)
    cases += [
        ("uo_call_rebate_hit", base(rebate_amount=2.0, rebate_at_hit=True, **uo)),
        ("uo_call_rebate_expiry", base(rebate_amount=2.0, **uo)),
        ("do_put_rebate_hit", base(rebate_amount=2.0, rebate_at_hit=True, **do)),
        ("dbl_call_rebate_expiry", base(rebate_amount=2.0, **dbl)),
        ("dbl_put_rebate_hit", base(rebate_amount=2.0, rebate_at_hit=True, option_type="put",
                                    **dbl)),
        ("uo_call_mean_sqrt_dt", base(use_mean_sqrt_dt=True, **uo)),
        ("dbl_call_mean_sqrt_dt", base(use_mean_sqrt_dt=True, **dbl)),
        ("do_put_theta_from_forward", base(theta_from_forward=True, **do)),
        ("uo_call_no_expiry_monitor", base(include_expiry_monitor=False, **{
            **uo, "monitor_dates": MONITORS + ["2025-08-28"]})),
        ("uo_call_expiry_monitor", base(**{**uo, "monitor_dates": MONITORS + ["2025-08-28"]})),
        ("uo_call_already_hit", base(rebate_amount=2.0, rebate_at_hit=True, already_hit=True,
                                     barrier_hit_date="2025-08-07", **uo)),
        ("uo_call_no_schedule", base(**{**uo, "monitor_dates": None})),
        ("do_put_no_schedule", base(**{**do, "monitor_dates": None})),
        ("dbl_call_short_scaled", base(direction="short", quantity=3, contract_multiplier=10.0,
                                       **dbl)),
        ("auto_dense_bgk", base(pricing_method="auto", barrier_type="up-and-out",
                                upper_barrier=250.0, rebate_amount=2.0, rebate_at_hit=True)),
        ("mc_already_hit", base(pricing_method="mc", barrier_type="up-and-out",
                                upper_barrier=250.0, rebate_amount=2.0, already_hit=True,
                                barrier_hit_date="2025-08-07", mc_n_paths=1024)),
        ("mc_spot_beyond_level", base(pricing_method="mc", barrier_type="double-out",
                                      lower_barrier=230.0, upper_barrier=250.0, mc_n_paths=1024)),
        ("auto_sparse_mc", base(pricing_method="auto", bgk_min_freq=100.0,
                                barrier_type="up-and-out", upper_barrier=250.0, mc_n_paths=1024)),
    ]
    return cases


def path_cases():
    mc = dict(pricing_method="mc", mc_n_paths=1024, mc_use_torch_rng=False)
    up = dict(barrier_type="up-and-out", upper_barrier=250.0)
    down = dict(barrier_type="down-and-out", lower_barrier=215.0)
    dbl = dict(lower_barrier=210.0, upper_barrier=250.0)
    exact = dict(mc_smooth_barrier_eps=0.0, mc_smooth_payoff_eps=0.0)
    three = ["2025-08-12", "2025-08-22"]
    return [
        ("uo_call_smooth_7", base(**mc, **up)),
        ("do_put_exact_rebate_hit_7", base(option_type="put", strike=235.0, rebate_amount=2.0,
                                           rebate_at_hit=True, **mc, **down, **exact)),
        ("dbl_out_call_smooth_rebate_hit_7", base(barrier_type="double-out", rebate_amount=2.0,
                                                  rebate_at_hit=True, **mc, **dbl)),
        ("dbl_out_put_exact_rebate_expiry_3", base(barrier_type="double-out", option_type="put",
                                                   strike=235.0, rebate_amount=2.0,
                                                   mc_smooth_barrier_eps=0.0, monitor_dates=three,
                                                   **mc, **dbl)),
        ("uo_put_single_sign_2", base(option_type="put", strike=235.0, mc_use_antithetic=False,
                                      mc_smooth_payoff_eps=0.0, monitor_dates=["2025-08-12"],
                                      **{**mc, "mc_n_paths": 512}, **up)),
        ("do_call_exact_1", base(monitor_dates=["2025-08-28"], **mc, **down, **exact)),
        ("dbl_in_call_smooth_7", base(barrier_type="double-in", **mc, **dbl)),
        ("uo_call_exact_3", base(monitor_dates=three, **mc, **up, **exact)),
        ("uo_call_smooth_torch_7", base(**{**mc, "mc_use_torch_rng": True}, **up)),
    ]


def large_cases():
    big = dict(pricing_method="mc", mc_n_paths=2_000_000, mc_use_torch_rng=False)
    return [
        ("uo_call_smooth_2m", base(barrier_type="up-and-out", upper_barrier=250.0, **big)),
        ("dbl_out_put_2m", base(barrier_type="double-out", option_type="put", strike=235.0,
                                lower_barrier=210.0, upper_barrier=250.0, **big)),
    ]


def reference_record(ref, inputs):
    p = ref.DiscreteBarrierBGKPricer(**bgk_fixture.kwargs_for(inputs))
    out = dict(price=p.price(), mc_std_error=p._last_mc_std_error, method=p._select_method(),
               greeks=p.greeks(), metrics=bgk_fixture.metrics_to_json(p.barrier_hit_metrics()),
               report=p.report(), hazard_table=p.report_hazard_table(), m=p.m,
               forward_price=p.forward_price, carry_rate_nacc=p.carry_rate_nacc,
               div_yield_nacc=p.div_yield_nacc, discount_rate_nacc=p.discount_rate_nacc)
    return out


def reference_paths(ref, inputs):
    p = ref.DiscreteBarrierBGKPricer(**bgk_fixture.kwargs_for(inputs))
    tap = _NumpyTap()
    ref.np = tap
    try:
        price = p.price()
    finally:
        ref.np = np
    return p, price, p._last_mc_std_error, tap.seen


def reference_normals(inputs, n_half, n_steps):
    if inputs.get("mc_use_torch_rng", True):
        import torch
        torch.manual_seed(42)
        return "torch", torch.randn(n_half, n_steps, dtype=torch.float64).numpy()
    return "numpy", np.random.default_rng(42).standard_normal((n_half, n_steps))


def assert_off_the_edges(name, plan, Z):
    from finite_difference_amd import capi
    P, S = plan.params, plan.step
    spots = np.exp(P[capi.BGK_P_LOG_SPOT]
                   + np.cumsum(S[:, capi.BGK_S_DRIFT][None, :] + S[:, capi.BGK_S_DIFF][None, :] * Z,
                               axis=1))
    gap = np.inf
    sides = int(plan.flags[capi.BGK_F_SIDES])
    if P[capi.BGK_P_EPS_BARRIER] == 0.0:
        for k in np.nonzero(S[:, capi.BGK_S_MONITOR])[0]:
            for bit, lv in ((1, P[capi.BGK_P_UPPER]), (2, P[capi.BGK_P_LOWER])):
                if sides & bit:
                    gap = min(gap, float(np.min(np.abs(spots[:, k] - lv))) / lv)
    if P[capi.BGK_P_EPS_PAYOFF] == 0.0:
        K = P[capi.BGK_P_STRIKE]
        gap = min(gap, float(np.min(np.abs(spots[:, -1] - K))) / K)
    assert gap > EDGE, (name, gap)
    return gap


def main():
    from finite_difference_amd import bgk_barrier
    ref = load_reference()
    closed = []
    for name, inputs in closed_form_cases():
        rec = reference_record(ref, inputs)
        mine = bgk_barrier.DiscreteBarrierBGKPricer(engine="host",
                                                    **bgk_fixture.kwargs_for(inputs))
        assert mine.price() == rec["price"], (name, mine.price(), rec["price"])
        assert mine.greeks() == rec["greeks"], name
        assert mine.report() == rec["report"], name
        print(f"{name}: {rec['method']} price {rec['price']:.8f} m {rec['m']}")
        closed.append(dict(name=name, inputs=inputs, result=rec))

    arrays, paths = {}, []
    for name, inputs in path_cases():
        p, price, se, seen = reference_paths(ref, inputs)
        mine = bgk_barrier.DiscreteBarrierBGKPricer(engine="host",
                                                    **bgk_fixture.kwargs_for(inputs))
        job = mine._job()
        plan = job.plan
        assert plan.n_half == 512, (name, plan.n_half)
        kind, Z = reference_normals(inputs, plan.n_half, plan.n_steps)
        key = f"z_{kind}_{plan.n_steps}"
        if key in arrays:
            assert np.array_equal(arrays[key], Z)
        arrays[key] = Z
        Zf = np.concatenate([Z, -Z], axis=0) if plan.antithetic else Z
        x, rp, _ = bgk_barrier.host_paths(plan, Zf)
        assert seen[0].shape == (plan.n_sim,)
        assert np.array_equal(x, seen[0]), name
        arrays[f"x_{name}"] = seen[0]
        if plan.rebate_mode == 2:
            assert np.array_equal(rp, seen[1]), name
            arrays[f"rebate_{name}"] = seen[1]
        else:
            assert not rp.any(), name
        gap = assert_off_the_edges(name, plan, Zf)
        my_price = mine.price()
        assert my_price == price and mine._last_mc_std_error == se, (name, my_price, price)
        print(f"{name}: steps {plan.n_steps} price {price:.8f} +- {se:.6f} "
              f"nonzero {int(np.count_nonzero(seen[0]))} edge gap {gap:.2e}")
        paths.append(dict(name=name, inputs=inputs, normals=key, n_steps=plan.n_steps,
                          n_sim=plan.n_sim, price=price, mc_std_error=se))

    large = []
    for name, inputs in large_cases():
        p = ref.DiscreteBarrierBGKPricer(**bgk_fixture.kwargs_for(inputs))
        price = p.price()
        print(f"{name}: price {price:.6f} +- {p._last_mc_std_error:.6f}")
        large.append(dict(name=name, inputs=inputs, price=price,
                          mc_std_error=p._last_mc_std_error))

    with open(os.path.join(HERE, "bgk_cases.json"), "w", encoding="utf-8") as f:
        json.dump(dict(generator="tests/golden/make_golden_bgk.py", edge=EDGE, closed=closed,
                       paths=paths, large=large), f, indent=1, ensure_ascii=False)
    np.savez_compressed(os.path.join(HERE, "bgk_cases.npz"), **arrays)
    for fn in ("bgk_cases.json", "bgk_cases.npz"):
        size = os.path.getsize(os.path.join(HERE, fn))
        print(fn, size, "bytes")
        assert size <= 300 * 1024, fn


if __name__ == "__main__":
    main()
