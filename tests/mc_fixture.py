"""Helpers shared by the Monte Carlo tests and tests/golden/make_golden_mc.py:
the fixtures of tests/golden/mc_cases.json / mc_cases.npz turned into the
keyword arguments of price_discrete_barrier_mc, for this package's module or
for any module with the same names."""
import datetime as dt
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CURVE_END = dt.date(2025, 9, 30)  # the flat curve covers valuation .. this date


def load_cases():
    with open(os.path.join(GOLDEN, "mc_cases.json")) as f:
        return json.load(f)


def load_arrays():
    """normals "z<n_steps>" [1024, n_steps] and payoffs "payoff_<name>" [1024]."""
    with np.load(os.path.join(GOLDEN, "mc_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def _date(s):
    return dt.date.fromisoformat(s)


def flat_curve(mod, rate, valuation, day_count="ACT/365F"):
    import pandas as pd
    days = pd.date_range(start=valuation, end=CURVE_END, freq="D")
    df = pd.DataFrame({"Date": days.strftime("%Y-%m-%d"), "NACA": rate})
    return mod.NacaCurve(df, valuation_date=valuation, day_count=day_count)


def kwargs_for(inputs, mod, curve=None):
    """price_discrete_barrier_mc keyword arguments of a fixture's inputs, built
    from `mod`'s classes (this package's mc_barrier or the reference)."""
    valuation = _date(inputs["valuation"])
    curve = curve or flat_curve(mod, inputs["rate"], valuation)
    b, r, c = inputs["barrier"], inputs["rebate"], inputs["cfg"]
    return dict(
        spot=inputs["spot"], strike=inputs["strike"], vol=inputs["vol"],
        option_type=inputs["option_type"], valuation=valuation,
        maturity=_date(inputs["maturity"]), discount_curve=curve, forward_curve=curve,
        dividends=[(_date(d), a) for d, a in inputs["dividends"]],
        monitor_dates=[_date(d) for d in inputs["monitor_dates"]],
        barrier=mod.BarrierSpec(b["type"], b["level"], b["tol_bps"], b["abs_tol"]),
        rebate=mod.RebateSpec(r["amount"], r["at_hit"]),
        cfg=mod.MCConfig(n_paths=c["n_paths"], seed=c["seed"], antithetic=c["antithetic"],
                         chunk_size=c["chunk_size"],
                         dividend_before_monitor=c["dividend_before_monitor"],
                         spot_floor=c["spot_floor"]),
        include_maturity_monitor=inputs["include_maturity_monitor"])


# ---------------------------------------------------------------------------
# The generator contract of include/fdcn.h, restated for the tests (not the
# package's code): Philox4x32-10 and the map from its words to normals.
# ---------------------------------------------------------------------------
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays (or ints) holding 32-bit words -> x0..x3."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    for r in range(10):
        ka = np.uint64((k0 + r * _W0) & 0xFFFFFFFF)
        kb = np.uint64((k1 + r * _W1) & 0xFFFFFFFF)
        prod0 = c0 * np.uint64(_M0)          # < 2^64: both factors are below 2^32
        prod1 = c2 * np.uint64(_M1)
        c0, c1, c2, c3 = ((prod1 >> _32) ^ c1 ^ ka, prod1 & _LO,
                          (prod0 >> _32) ^ c3 ^ kb, prod0 & _LO)
    return c0, c1, c2, c3


def expected_normals(n_obs, n_steps, seed, stream_id=0, obs_first=0):
    """z [n_obs, n_steps]: counter (o lo, o hi, j, stream id), o = obs_first + i;
    key (seed lo, seed hi); u = ((a >> 5) 2^26 + (b >> 6) + 0.5) 2^-53;
    z[2j] = sqrt(-2 ln u1) cos(2 pi u2), z[2j+1] the sine; an odd n_steps
    drops the last sine."""
    z = np.empty((n_obs, n_steps))
    o = np.arange(n_obs, dtype=np.uint64) + np.uint64(obs_first)
    for j in range((n_steps + 1) // 2):
        x0, x1, x2, x3 = philox(o & _LO, o >> _32, j, stream_id, seed & 0xFFFFFFFF, seed >> 32)
        u1 = ((x0 >> np.uint64(5)).astype(float) * 2.0 ** 26 + (x1 >> np.uint64(6)).astype(float)
              + 0.5) * 2.0 ** -53
        u2 = ((x2 >> np.uint64(5)).astype(float) * 2.0 ** 26 + (x3 >> np.uint64(6)).astype(float)
              + 0.5) * 2.0 ** -53
        radius = np.sqrt(-2.0 * np.log(u1))
        z[:, 2 * j] = radius * np.cos(2.0 * np.pi * u2)
        if 2 * j + 1 < n_steps:
            z[:, 2 * j + 1] = radius * np.sin(2.0 * np.pi * u2)
    return z
