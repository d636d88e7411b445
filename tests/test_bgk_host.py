"""BGK barrier pricer, CPU side: the closed forms and the façade's host engine
against the reference's recorded numbers (tests/golden/bgk_cases.json / .npz,
written by make_golden_bgk.py), the errors the constructor raises, the two
recorded deviations, the batch API, and the C ABI's argument validation (which
happens before any device call)."""
import ctypes
import datetime as dt
import math

import numpy as np
import pytest

import bgk_fixture as fx
import finite_difference_amd as fda
from finite_difference_amd import bgk_barrier, capi
from finite_difference_amd.bgk_barrier import DiscreteBarrierBGKPricer

CASES = fx.load_cases()
ARRAYS = fx.load_arrays()
REL = 1e-13


def _pricer(inputs, **over):
    return DiscreteBarrierBGKPricer(engine="host", **{**fx.kwargs_for(inputs), **over})


def _close(got, ref, rel=REL):
    assert abs(got - ref) <= rel * abs(ref), (got, ref)


def _path_case(name):
    return next(c for c in CASES["paths"] if c["name"] == name)


# ---------------------------------------------------------------- closed forms
@pytest.mark.parametrize("case", CASES["closed"], ids=lambda c: c["name"])
def test_closed_forms_equal_the_reference(case):
    """Scalar math in the reference's order: price, Greeks, hazard tuples,
    derived attributes and both reports are equal, not close."""
    p = _pricer(case["inputs"])
    ref = case["result"]
    assert p._select_method() == ref["method"]
    assert p.price() == ref["price"]
    if ref["method"] == "mc":
        assert p._last_mc_std_error == ref["mc_std_error"]
    assert p.greeks() == ref["greeks"]
    assert fx.metrics_to_json(p.barrier_hit_metrics()) == ref["metrics"]
    assert p.report() == ref["report"]
    assert p.report_hazard_table() == ref["hazard_table"]
    for key in ("m", "forward_price", "carry_rate_nacc", "div_yield_nacc", "discount_rate_nacc"):
        assert getattr(p, key) == ref[key], key


def test_closed_form_fixtures_cover_what_they_must():
    ins = [c["inputs"] for c in CASES["closed"]]
    kinds = {"none", "up-and-out", "down-and-out", "up-and-in", "down-and-in", "double-out",
             "double-in"}
    assert {(i["barrier_type"], i["option_type"]) for i in ins} >= {
        (k, o) for k in kinds for o in ("call", "put")}
    assert any(i.get("rebate_amount") and i.get("rebate_at_hit") for i in ins)
    assert any(i.get("rebate_amount") and not i.get("rebate_at_hit") for i in ins)
    for flag in ("use_mean_sqrt_dt", "theta_from_forward", "already_hit"):
        assert any(i.get(flag) for i in ins), flag
    assert any(i.get("include_expiry_monitor") is False for i in ins)
    assert any(i["monitor_dates"] is None for i in ins)
    autos = {c["result"]["method"] for c in CASES["closed"]
             if c["inputs"]["pricing_method"] == "auto"}
    assert autos == {"bgk", "mc"}


# ----------------------------------------------------------------------- paths
@pytest.mark.parametrize("case", CASES["paths"], ids=lambda c: c["name"])
def test_host_paths_equal_the_reference_bit_for_bit(case):
    p = _pricer(case["inputs"])
    plan = p._job().plan
    assert (plan.n_steps, plan.n_sim) == (case["n_steps"], case["n_sim"])
    z = ARRAYS[case["normals"]]
    zf = np.concatenate([z, -z], axis=0) if plan.antithetic else z
    x, rebate, alive = bgk_barrier.host_paths(plan, zf)
    assert np.array_equal(x, ARRAYS["x_" + case["name"]])
    if plan.rebate_mode == 2:
        assert np.array_equal(rebate, ARRAYS["rebate_" + case["name"]])
    else:
        assert not rebate.any()
    assert np.all((alive >= 0.0) & (alive <= 1.0))


@pytest.mark.parametrize("case", CASES["paths"], ids=lambda c: c["name"])
def test_host_engine_price_and_standard_error(case):
    """The façade draws the reference's normals itself (NumPy or a local torch
    generator): price and standard error to 1e-13 relative."""
    p = _pricer(case["inputs"])
    _close(p.price(), case["price"])
    _close(p._last_mc_std_error, case["mc_std_error"])
    # from the raw sums (what the device returns) the same numbers follow
    plan = p._job().plan
    z = ARRAYS[case["normals"]]
    stats = bgk_barrier.run_paths([[plan]], engine="host", z=z)[0, 0]
    px, se = bgk_barrier.compose(plan, plan.n_sim, *stats[:3])
    if not case["inputs"]["barrier_type"].endswith("-in"):   # in = vanilla - out
        _close(px, case["price"], 1e-12)
    _close(se, case["mc_std_error"], 1e-10)


def test_path_fixtures_cover_what_they_must():
    ins = [c["inputs"] for c in CASES["paths"]]
    assert {c["n_steps"] for c in CASES["paths"]} == {1, 2, 3, 7}
    assert {i["option_type"] for i in ins} == {"call", "put"}
    assert {i["barrier_type"] for i in ins} >= {"up-and-out", "down-and-out", "double-out",
                                                "double-in"}
    assert {i.get("mc_smooth_barrier_eps", 0.01) > 0 for i in ins} == {True, False}
    assert {i.get("mc_smooth_payoff_eps", 0.005) > 0 for i in ins} == {True, False}
    modes = {(bool(i.get("rebate_amount")), bool(i.get("rebate_at_hit"))) for i in ins}
    assert modes >= {(False, False), (True, False), (True, True)}
    assert any(i.get("mc_use_antithetic") is False for i in ins)
    assert any(i.get("mc_use_torch_rng") for i in ins)
    for c in CASES["paths"]:
        assert c["n_sim"] // (1 if c["inputs"].get("mc_use_antithetic") is False else 2) == 512


def test_module_names_and_exports():
    assert fda.DiscreteBarrierBGKPricer is DiscreteBarrierBGKPricer
    assert fda.bgk_price_batch is bgk_barrier.bgk_price_batch
    assert bgk_barrier.BETA_BGK == 0.5826
    x = np.array([-1.0, -0.004, 0.0, 0.004, 1.0])
    assert bgk_barrier.smooth_relu(x, eps=0.005)[0] == 0.0
    assert bgk_barrier.smooth_relu(x, eps=0.005)[4] == 1.0
    assert bgk_barrier.smooth_relu(x, eps=0.005)[2] == 0.5 * 0.005 ** 2 / 0.01
    up = bgk_barrier.smooth_heaviside_up(np.array([249.0, 250.0, 251.0]), 250.0, eps=0.01)
    dn = bgk_barrier.smooth_heaviside_down(np.array([249.0, 250.0, 251.0]), 250.0, eps=0.01)
    assert up.tolist() == [0.0, 0.5, 1.0] and dn.tolist() == [1.0, 0.5, 0.0]


def test_constructor_errors_match_the_reference():
    kw = fx.kwargs_for(CASES["closed"][0]["inputs"])
    for bad in (dict(spot=0.0), dict(strike=-1.0), dict(volatility=0.0)):
        with pytest.raises(ValueError, match="spot, strike, volatility must be positive."):
            DiscreteBarrierBGKPricer(**{**kw, **bad})
    with pytest.raises(ValueError, match="maturity_date must be after valuation_date."):
        DiscreteBarrierBGKPricer(**{**kw, "maturity_date": kw["valuation_date"]})
    with pytest.raises(ValueError, match="engine"):
        DiscreteBarrierBGKPricer(engine="eager", **kw)
    with pytest.raises(ValueError, match="mc_rng"):
        DiscreteBarrierBGKPricer(mc_rng="mt19937", **kw)
    p = DiscreteBarrierBGKPricer(engine="host", **{**kw, "barrier_type": "double-out",
                                                   "pricing_method": "bgk",
                                                   "upper_barrier": 250.0})
    with pytest.raises(ValueError, match="Double barrier requires both"):
        p.price()
    p = DiscreteBarrierBGKPricer(engine="host", **{**kw, "barrier_type": "sideways",
                                                   "pricing_method": "bgk"})
    with pytest.raises(ValueError, match="Unsupported barrier_type"):
        p.price()
    import pandas as pd
    p = DiscreteBarrierBGKPricer(engine="host", **kw)
    with pytest.raises(ValueError, match="Curve must have"):
        p._df_from_curve(pd.DataFrame({"when": ["2025-08-01"], "rate": [0.07]}),
                         dt.date(2025, 8, 1))


def test_curve_lookup_falls_back_to_the_nearest_prior_date():
    import pandas as pd
    kw = fx.kwargs_for(CASES["closed"][0]["inputs"])
    p = DiscreteBarrierBGKPricer(engine="host", **kw)
    naca = pd.DataFrame({"Date": ["2025-07-28", "2025-08-10"], "NACA": [0.05, 0.08]})
    assert p._df_from_curve(naca, dt.date(2025, 8, 20)) == (1.0 + 0.08) ** (-23 / 365.0)
    assert p._df_from_curve(naca, dt.date(2025, 8, 5)) == (1.0 + 0.05) ** (-8 / 365.0)
    dfs = pd.DataFrame({"date": ["2025-07-28", "2025-08-10"], "df": [1.0, 0.99]})
    assert p._df_from_curve(dfs, dt.date(2025, 8, 20)) == 0.99
    assert p._df_from_curve(dfs, dt.date(2025, 7, 1)) == 1.0
    assert p._df_from_curve(None, dt.date(2025, 8, 20)) == 1.0


def test_smoothed_barrier_with_rebate_at_expiry_prices():
    """Deviation 1: the reference raises UnboundLocalError here; this package
    pays R * (1 - alive).  With eps = 0 that is the reference's own number."""
    exact = _path_case("dbl_out_put_exact_rebate_expiry_3")
    _close(_pricer(exact["inputs"]).price(), exact["price"])
    smooth = _pricer(exact["inputs"], mc_smooth_barrier_eps=0.01)
    px = smooth.price()
    assert math.isfinite(px) and math.isfinite(smooth._last_mc_std_error)
    # a band of 0.01 around two levels moves few of 1024 paths: close to the exact price
    assert abs(px - exact["price"]) < 3.0 * exact["mc_std_error"]
    plan = smooth._job().plan
    z = ARRAYS[exact["normals"]]
    x, _, alive = bgk_barrier.host_paths(plan, np.concatenate([z, -z], axis=0))
    dead = alive == 0.0
    assert dead.any() and np.all(x[dead] == 2.0)


def test_torch_normals_leave_the_global_generator_alone():
    """Deviation 2: the façade's torch normals come from a local generator and
    equal what the reference draws after torch.manual_seed."""
    import torch
    torch.manual_seed(1234)
    before = torch.get_rng_state().clone()
    case = _path_case("uo_call_smooth_torch_7")
    _pricer(case["inputs"]).price()
    assert torch.equal(torch.get_rng_state(), before)
    z = bgk_barrier.draw_normals("torch", 42, 512, 7)
    assert np.array_equal(z, ARRAYS["z_torch_7"])
    torch.manual_seed(42)
    assert np.array_equal(z, torch.randn(512, 7, dtype=torch.float64).numpy())


def test_settlement_lags_use_the_package_calendar():
    kw = fx.kwargs_for(CASES["closed"][2]["inputs"])
    p = DiscreteBarrierBGKPricer(engine="host", underlying_spot_days=3, option_days=1,
                                 option_settlement_days=2, **kw)
    assert p.carry_start_date == dt.date(2025, 7, 31)
    assert p.discount_end_date == dt.date(2025, 9, 1)
    assert p.time_to_carry > 0 and math.isfinite(p.price())
    assert "Spot lag (carry)   : 3bd  (2025-07-31 -> " in p.report()


def test_missing_gpu_under_hip_is_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(capi, "device_count", lambda: 0)
    case = _path_case("uo_call_smooth_7")
    p = DiscreteBarrierBGKPricer(engine="hip", **fx.kwargs_for(case["inputs"]))
    with pytest.raises(capi.FdcnError):
        p.price()


# ------------------------------------------------------------------- batch API
def test_batch_host_engine_equals_the_single_pricers():
    trades = [fx.kwargs_for(c["inputs"]) for c in CASES["paths"]]
    trades.append(fx.kwargs_for(CASES["closed"][4]["inputs"]))
    out = bgk_barrier.bgk_price_batch(trades, engine="host")
    for res, case in zip(out, CASES["paths"]):
        assert res["method"] == "mc" and res["n_paths"] == case["n_sim"]
        _close(res["price"], case["price"])
        _close(res["mc_std_error"], case["mc_std_error"], 1e-10)
        assert len(res["sums"]) == 4
    assert out[-1]["method"] == "bgk" and out[-1]["sums"] is None
    assert out[-1]["price"] == CASES["closed"][4]["result"]["price"]


def test_batch_greeks_equal_the_single_pricer():
    case = next(c for c in CASES["closed"] if c["name"] == "auto_sparse_mc")
    res = bgk_barrier.bgk_price_batch([fx.kwargs_for(case["inputs"])], greeks=True,
                                      engine="host")[0]
    assert res["price"] == case["result"]["price"]
    for k, v in case["result"]["greeks"].items():
        assert res[k] == v, k


def test_raw_sums_of_disjoint_ranges_add():
    case = _path_case("dbl_out_call_smooth_rebate_hit_7")
    trades = [fx.kwargs_for(case["inputs"])] * 2
    kw = dict(engine="host", mc_rng="philox")
    whole = bgk_barrier.bgk_price_batch(trades, **kw)
    a = bgk_barrier.bgk_price_batch(trades, obs_range=range(0, 200), **kw)
    b = bgk_barrier.bgk_price_batch(trades, obs_range=range(200, 512), **kw)
    for w, pa, pb in zip(whole, a, b):
        assert pa["n_paths"] + pb["n_paths"] == w["n_paths"] == 1024
        np.testing.assert_allclose(np.add(pa["sums"], pb["sums"]), w["sums"], rtol=1e-12)
    assert whole[0]["sums"] != whole[1]["sums"]          # stream id = index in the batch
    with pytest.raises(ValueError, match="obs_range needs"):
        bgk_barrier.bgk_price_batch(trades, engine="host", obs_range=range(0, 10))


# ------------------------------------------------------------------- C ABI
def _abi_arrays(G=1, n_steps=2):
    P = np.zeros((1, G, capi.BGK_NPARAM))
    P[..., capi.BGK_P_LOG_SPOT] = math.log(100.0)
    P[..., capi.BGK_P_STRIKE] = 100.0
    P[..., capi.BGK_P_UPPER] = 120.0
    P[..., capi.BGK_P_LOWER] = 80.0
    P[..., capi.BGK_P_EPS_BARRIER] = 0.01
    F = np.array([[0, 3, 0, 0]], dtype=np.int32)
    S = np.zeros((1, G, n_steps, capi.BGK_NSTEP))
    S[..., capi.BGK_S_DIFF] = 0.1
    S[..., capi.BGK_S_MONITOR] = 1.0
    S[..., capi.BGK_S_DF_END] = 1.0
    return P, F, S


def _call(P, F, S, *, G=None, n_obs=8, anti=1, null=()):
    L = capi.lib()
    B = P.shape[0]
    G = P.shape[1] if G is None else G
    stats = np.zeros((B, max(G, 1), capi.BGK_NSTAT))
    ptr = dict(params=P.ctypes.data, flags=F.ctypes.data, step=S.ctypes.data,
               stats=stats.ctypes.data)
    for k in null:
        ptr[k] = None
    rc = L.fdcn_mc_bgk_batch(B, G, S.shape[2], n_obs, anti, ptr["params"], ptr["flags"],
                             ptr["step"], None, 1, 0, ptr["stats"], None)
    return rc, L.fdcn_last_error().decode()


def test_c_abi_rejects_bad_arguments_before_any_device_call():
    EINVAL = -1
    P, F, S = _abi_arrays()
    for G in (0, 9, -1):
        rc, msg = _call(P, F, S, G=G)
        assert rc == EINVAL and "G must be in 1 .. 8" in msg, (G, rc, msg)
    for col, bad, text in ((capi.BGK_F_SIDES, 4, "sides"), (capi.BGK_F_SIDES, -1, "sides"),
                           (capi.BGK_F_REBATE_MODE, 3, "rebate mode"),
                           (capi.BGK_F_REBATE_MODE, -1, "rebate mode"),
                           (capi.BGK_F_PUT, 2, "put"), (capi.BGK_F_STREAM, -1, "stream")):
        F2 = F.copy()
        F2[0, col] = bad
        rc, msg = _call(P, F2, S)
        assert rc == EINVAL and text in msg, (col, bad, rc, msg)
    for col, bad, text in ((capi.BGK_P_EPS_BARRIER, -0.01, "barrier epsilon"),
                           (capi.BGK_P_EPS_PAYOFF, -1e-9, "payoff epsilon"),
                           (capi.BGK_P_UPPER, 0.0, "upper level"),
                           (capi.BGK_P_LOWER, -5.0, "lower level"),
                           (capi.BGK_P_STRIKE, 0.0, "strike"),
                           (capi.BGK_P_LOG_SPOT, float("nan"), "log-spot")):
        P2 = P.copy()
        P2[0, 0, col] = bad
        rc, msg = _call(P2, F, S)
        assert rc == EINVAL and text in msg, (col, bad, rc, msg)
    # an inactive side's level is not read
    F1 = F.copy()
    F1[0, capi.BGK_F_SIDES] = 1
    P2 = P.copy()
    P2[0, 0, capi.BGK_P_LOWER] = 0.0
    rc, msg = _call(P2, F1, S)
    assert rc != EINVAL or "level" not in msg
    for name in ("params", "flags", "step", "stats"):
        rc, msg = _call(P, F, S, null=(name,))
        assert rc == EINVAL and f"{name} is NULL" in msg, (name, rc, msg)
    for kw, text in ((dict(n_obs=0), "n_obs"), (dict(anti=2), "antithetic")):
        rc, msg = _call(P, F, S, **kw)
        assert rc == EINVAL and text in msg
    # the second scenario of a group is checked too
    P8, F8, S8 = _abi_arrays(G=8)
    P8[0, 7, capi.BGK_P_EPS_BARRIER] = -1.0
    rc, msg = _call(P8, F8, S8)
    assert rc == EINVAL and "barrier epsilon" in msg


def test_c_abi_dev_entry_rejects_a_small_workspace_and_plan_sizes_it():
    EINVAL = -1
    L = capi.lib()
    plan = capi.mc_bgk_plan(10_000, 5)
    chunk = plan["obs_per_block"]
    assert plan["blocks_per_trade"] == -(-10_000 // chunk)
    assert plan["ws_bytes_per_trade"] == plan["blocks_per_trade"] * 5 * 4 * 8
    assert capi.mc_bgk_plan(1, 5)["obs_per_block"] == capi.mc_bgk_plan(10 ** 9, 1)["obs_per_block"]
    with pytest.raises(capi.FdcnError):
        capi.mc_bgk_plan(100, 9)
    need = 3 * plan["ws_bytes_per_trade"]
    fake = 4096  # never dereferenced: validation comes first
    rc = L.fdcn_mc_bgk_batch_dev(3, 5, 7, 10_000, 1, fake, fake, fake, None, 1, 0, fake, None,
                                 fake, need - 1, None)
    assert rc == EINVAL and "workspace" in L.fdcn_last_error().decode()
    for G in (0, 9):
        rc = L.fdcn_mc_bgk_batch_dev(3, G, 7, 10_000, 1, fake, fake, fake, None, 1, 0, fake, None,
                                     fake, 1 << 30, None)
        assert rc == EINVAL and "G must be" in L.fdcn_last_error().decode()
    rc = L.fdcn_mc_bgk_batch_dev(3, 5, 7, 10_000, 1, fake, None, fake, None, 1, 0, fake, None,
                                 fake, need, None)
    assert rc == EINVAL and "flags is NULL" in L.fdcn_last_error().decode()
    assert ctypes.sizeof(ctypes.c_double) == 8
