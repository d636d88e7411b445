"""Helpers shared by the BGK barrier tests and tests/golden/make_golden_bgk.py:
the fixtures of tests/golden/bgk_cases.json / bgk_cases.npz turned into the
constructor keywords of DiscreteBarrierBGKPricer (this package's or the
reference's: the keywords are the same)."""
import datetime as dt
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVE_END = dt.date(2025, 9, 30)  # the flat curve covers valuation .. this date
_DATE_KEYS = ("valuation_date", "maturity_date", "barrier_hit_date")


def load_cases():
    with open(os.path.join(GOLDEN, "bgk_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def load_arrays():
    """normals "z_numpy_<n_steps>" / "z_torch_<n_steps>" [512, n_steps] and the
    reference's per-path values "x_<case>", "rebate_<case>" [n_sim]."""
    with np.load(os.path.join(GOLDEN, "bgk_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def flat_curve(rate, valuation):
    import pandas as pd
    days = pd.date_range(start=valuation, end=CURVE_END, freq="D")
    return pd.DataFrame({"Date": days.strftime("%Y-%m-%d"), "NACA": rate})


def kwargs_for(inputs):
    """Constructor keywords of a fixture's inputs (JSON: ISO dates, a flat
    rate for both curves)."""
    kw = dict(inputs)
    rate = kw.pop("rate")
    for k in _DATE_KEYS:
        if kw.get(k) is not None:
            kw[k] = dt.date.fromisoformat(kw[k])
    if kw.get("monitor_dates") is not None:
        kw["monitor_dates"] = [dt.date.fromisoformat(d) for d in kw["monitor_dates"]]
    kw["dividend_schedule"] = [(dt.date.fromisoformat(d), a)
                               for d, a in kw.get("dividend_schedule") or []]
    curve = flat_curve(rate, kw["valuation_date"])
    kw["discount_curve"] = curve
    kw["forward_curve"] = curve
    return kw


def metrics_to_json(mets):
    out = dict(mets)
    out["hazard"] = [[d.isoformat(), p, DF, c] for d, p, DF, c in mets["hazard"]]
    for k in ("expected_hit_date", "mode_hit_date"):
        out[k] = mets[k].isoformat() if mets[k] is not None else None
    return out


def path_bounds(plan, Z, x_ref):
    """Per-path bounds of |device - host| for x and rebate_pv on the normals Z
    [n_sim, n_steps] (both signs stacked).

    Host and device form logS0 + c from the same separately rounded
    operations, so they differ only through the two exps, at most 2 ulp:
    a spot S moves by at most 2^-51 S.  Inside a smoothed band of half-width
    e_b that moves one monitor's breach amount by 2^-51 S / (2 e_b) and alive by
    at most n_mon times that; the terminal spot moves intrinsic by at most
    2^-51 S (slope <= 1).  So |dx| <= 2^-51 S_max (1 + n_mon intrinsic / (2 e_b))
    with S_max the path's largest spot; the bound carries a factor 4:

        4 * 2^-51 * S_max * (1 + n_mon * intrinsic / (2 e_b)).

    rebate_pv (rebate at hit) is a sum of R * DF * newly terms, newly moving
    with the breach amount: 4 * 2^-51 * S_max * n_mon * R / (2 e_b).
    For e_b = 0 no decision flips (the fixtures are kept off the edges) and
    rebate_pv is exact: 1e-11 relative to x_ref + 1e-12 * spot for x, as for
    the single-barrier engine."""
    from finite_difference_amd import bgk_barrier, capi
    P, S = plan.params, plan.step
    spots = np.exp(P[capi.BGK_P_LOG_SPOT]
                   + np.cumsum(S[:, capi.BGK_S_DRIFT][None, :]
                               + S[:, capi.BGK_S_DIFF][None, :] * Z, axis=1))
    d = spots[:, -1] - P[capi.BGK_P_STRIKE]
    d = -d if plan.flags[capi.BGK_F_PUT] else d
    eps_p = float(P[capi.BGK_P_EPS_PAYOFF])
    intrinsic = bgk_barrier.smooth_relu(d, eps=eps_p) if eps_p > 0.0 else np.maximum(d, 0.0)
    eps_b = float(P[capi.BGK_P_EPS_BARRIER])
    if eps_b == 0.0:
        spot = float(np.exp(P[capi.BGK_P_LOG_SPOT]))
        return 1e-11 * np.abs(x_ref) + 1e-12 * spot, np.zeros(Z.shape[0])
    n_mon = int(np.count_nonzero(S[:, capi.BGK_S_MONITOR]))
    s_max = spots.max(axis=1)
    unit = 4.0 * 2.0 ** -51 * s_max
    return (unit * (1.0 + n_mon * intrinsic / (2.0 * eps_b)),
            unit * n_mon * float(P[capi.BGK_P_REBATE]) / (2.0 * eps_b))
