"""BGK barrier pricer's Monte Carlo paths on the GPU (csrc/fdcn_mc_bgk.hip):
per-path parity with the reference on its own normals, grouped Greeks against
single launches, bitwise determinism under grouping / batching / splitting, the
tails, statistical parity on the device generator, a cross-check against the
single-barrier engine, and the device-pointer entry.  Every launch has valid
arguments or is rejected on the host before the device is touched."""
import datetime as dt
import math

import numpy as np
import pytest

import bgk_fixture as fx
import mc_fixture
from finite_difference_amd import bgk_barrier, capi, mc_barrier
from finite_difference_amd.bgk_barrier import DiscreteBarrierBGKPricer, run_paths

pytestmark = pytest.mark.gpu

CASES = fx.load_cases()
ARRAYS = fx.load_arrays()


def _pricer(case, engine="hip", **over):
    return DiscreteBarrierBGKPricer(engine=engine, **{**fx.kwargs_for(case["inputs"]), **over})


def _case(name):
    return next(c for c in CASES["paths"] + CASES["closed"] if c["name"] == name)


def _both_signs(plan, z):
    return np.concatenate([z, -z], axis=0) if plan.antithetic else z


def _bitwise(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.fixture(scope="module")
def chunk():
    return capi.mc_bgk_plan(1, 1)["obs_per_block"]


@pytest.fixture(scope="module")
def seven_step_plans():
    """One plan per seven-step path fixture: smoothed and exact tests, single
    and double levels, every rebate mode but the one at expiry."""
    return [_pricer(c)._job().plan for c in CASES["paths"] if c["n_steps"] == 7]


@pytest.fixture(scope="module")
def ladder():
    """The five Greeks scenarios of one trade (double-out call, smoothed,
    rebate at hit): they share the trade's flags, as a group must."""
    p = _pricer(_case("dbl_out_call_smooth_rebate_hit_7"))
    plans = [j.plan for j in p._bumped_jobs(1e-4 * p.spot_price, 1e-4)]
    assert len(plans) == 5 and all(pl is not None for pl in plans)
    return plans


# ---------------------------------------------------------------------------
# 1. per-path parity, normals supplied
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["paths"], ids=lambda c: c["name"])
def test_path_parity_on_the_references_normals(case):
    """Per path |gpu - ref| <= 4 * 2^-51 * S_max * (1 + n_mon * intrinsic /
    (2 eps_b)), or 1e-11 relative + 1e-12 * spot for eps_b = 0 (derivation:
    bgk_fixture.path_bounds).  Price and standard error through the façade
    agree with the fixture to the largest per-path bound (a mean of errors is
    at most their maximum; no sqrt(n) is taken off)."""
    p = _pricer(case)
    plan = p._job().plan
    z = ARRAYS[case["normals"]]
    x_ref = ARRAYS["x_" + case["name"]]
    bound_x, bound_r = fx.path_bounds(plan, _both_signs(plan, z), x_ref)
    stats, pay = run_paths([[plan]], engine="hip", z=z, want_payoffs=True)
    err = np.abs(pay[0, 0, 0] - x_ref)
    k = int(np.argmax(err / bound_x))
    print(f"{case['name']}: worst x error {err[k]:.3e} (bound there {bound_x[k]:.3e})")
    assert np.all(err <= bound_x)
    r_ref = ARRAYS.get("rebate_" + case["name"], np.zeros_like(x_ref))
    err_r = np.abs(pay[0, 0, 1] - r_ref)
    print(f"  worst rebate_pv error {err_r.max():.3e} (largest bound {bound_r.max():.3e})")
    assert np.all(err_r <= bound_r)
    # the four raw sums are those of the per-path values
    assert abs(stats[0, 0, 0] - np.sum(pay[0, 0, 0])) <= 1e-12 * np.sum(np.abs(pay[0, 0, 0]))
    assert abs(stats[0, 0, 2] - np.sum(pay[0, 0, 1])) <= 1e-12 * np.sum(np.abs(r_ref)) + 1e-300
    # through the façade, as a user calls it (it draws the same normals itself)
    tol = float(bound_x.max() + bound_r.max())
    price = p.price()
    print(f"  price error {abs(price - case['price']):.3e}  stderr error "
          f"{abs(p._last_mc_std_error - case['mc_std_error']):.3e}  (bound {tol:.3e})")
    assert abs(price - case["price"]) <= tol
    assert abs(p._last_mc_std_error - case["mc_std_error"]) <= tol


def test_torch_normals_by_default():
    """mc_use_torch_rng=True, mc_rng=None: the façade's local torch generator
    against the host engine on torch.randn drawn here."""
    import torch
    case = _case("uo_call_smooth_torch_7")
    p = _pricer(case)
    plan = p._job().plan
    torch.manual_seed(42)
    z = torch.randn(512, 7, dtype=torch.float64).numpy()
    x, rebate, _ = bgk_barrier.host_paths(plan, _both_signs(plan, z))
    want = plan.df_T * float(np.mean(x))
    bound_x, _ = fx.path_bounds(plan, _both_signs(plan, z), x)
    got = p.price()
    print(f"torch: price error {abs(got - want):.3e} (bound {bound_x.max():.3e})")
    assert abs(got - want) <= bound_x.max()
    assert abs(got - case["price"]) <= bound_x.max()


# ---------------------------------------------------------------------------
# 2. grouping
# ---------------------------------------------------------------------------
def test_greeks_launch_equals_five_single_launches(ladder):
    """One G = 5 launch against five G = 1 launches with the same stream id:
    all four sums bit for bit, on the device generator and on supplied z."""
    plans = ladder
    z = ARRAYS["z_numpy_7"]
    for kw in (dict(seed=31, stream_ids=[6]), dict(z=z, stream_ids=[6])):
        grouped = run_paths([plans], engine="hip", **kw)
        for g, plan in enumerate(plans):
            alone = run_paths([[plan]], engine="hip", **kw)
            assert _bitwise(alone[0, 0], grouped[0, g]), (g, alone[0, 0], grouped[0, g])
    # the scenarios differ: the bumps are not lost in the grouping
    assert len({tuple(grouped[0, g]) for g in range(5)}) == 5


def test_greeks_agree_with_the_fixture():
    """Each of the five prices is a mean of per-path values, so it carries at
    most e = max per-path bound (test 1).  The quotients propagate it:
      delta = (up - dn) / (2 ds)            -> 2 e / (2 ds)  = e / ds
      gamma = (up - 2 base + dn) / ds^2     -> 4 e / ds^2
      vega  = (upv - dnv) / (2 dv)          -> 2 e / (2 dv)  = e / dv
    with ds = 1e-4 * spot and dv = 1e-4 (quantity and multiplier are 1)."""
    case = _case("auto_sparse_mc")
    p = _pricer(case)
    got = p.greeks()
    ref = case["result"]["greeks"]
    plan = p._job().plan
    z = ARRAYS["z_torch_7"]
    x, _, _ = bgk_barrier.host_paths(plan, _both_signs(plan, z))
    e = float(fx.path_bounds(plan, _both_signs(plan, z), x)[0].max())
    ds, dv = 1e-4 * p.spot_price, 1e-4
    tol = {"delta": e / ds, "gamma": 4.0 * e / (ds * ds), "vega": e / dv}
    for k in ("delta", "gamma", "vega"):
        print(f"{k}: {got[k]:.10f} ref {ref[k]:.10f} diff {abs(got[k] - ref[k]):.3e} "
              f"tol {tol[k]:.3e}")
        assert abs(got[k] - ref[k]) <= tol[k], k
    # the standard error left behind is that of sigma - dsigma, the last scenario
    host = _pricer(case, engine="host")
    host.greeks()
    assert abs(p._last_mc_std_error - host._last_mc_std_error) <= e


# ---------------------------------------------------------------------------
# 3. determinism (bitwise)
# ---------------------------------------------------------------------------
def test_sums_do_not_depend_on_the_group_or_the_slot(ladder, chunk):
    plan, other = ladder[2], ladder[0]
    n_obs = chunk + 904
    kw = dict(engine="hip", seed=99, stream_ids=[5], n_obs=n_obs)
    alone = run_paths([[plan]], **kw)
    pair = run_paths([[plan, other]], **kw)
    eight = run_paths([[other] * 7 + [plan]], **kw)
    assert _bitwise(alone[0, 0], pair[0, 0])
    assert _bitwise(alone[0, 0], eight[0, 7])
    assert _bitwise(pair[0, 1], eight[0, 0])
    assert _bitwise(run_paths([[plan]], **kw), alone)      # run to run
    # another stream id is another sample
    assert not np.array_equal(run_paths([[plan]], **{**kw, "stream_ids": [6]}), alone)


def test_sums_do_not_depend_on_the_batch(seven_step_plans, chunk):
    pool = seven_step_plans
    assert len({(int(p.flags[1]), int(p.flags[2]), p.params[4] > 0) for p in pool}) >= 3
    batch = [[pool[k % len(pool)]] for k in range(37)]
    n_obs = chunk + 904
    kw = dict(engine="hip", seed=99, n_obs=n_obs, want_payoffs=True)
    alone = run_paths([batch[17]], stream_ids=[17], **kw)
    mixed = run_paths(batch, **kw)
    again = run_paths(batch, **kw)
    assert _bitwise(alone[0][0], mixed[0][17]) and _bitwise(alone[1][0], mixed[1][17])
    assert _bitwise(mixed[0], again[0]) and _bitwise(mixed[1], again[1])
    assert not np.array_equal(mixed[1][17], mixed[1][17 + len(pool)])


def test_ranges_continue_one_stream(seven_step_plans, chunk):
    plan = seven_step_plans[2]
    n, k = chunk + 1904, 1500
    assert k % chunk != 0
    kw = dict(engine="hip", seed=5, stream_ids=[4], want_payoffs=True)
    whole = run_paths([[plan] * 2], n_obs=n, **kw)
    head = run_paths([[plan] * 2], n_obs=k, **kw)
    tail = run_paths([[plan] * 2], n_obs=n - k, obs_first=k, **kw)
    for g in range(2):
        for which in range(2):          # x, rebate_pv
            for sign in range(2):       # +z paths, then -z paths
                w = whole[1][0, g, which, sign * n:(sign + 1) * n]
                h = head[1][0, g, which, sign * k:(sign + 1) * k]
                t = tail[1][0, g, which, sign * (n - k):(sign + 1) * (n - k)]
                assert _bitwise(w, np.concatenate([h, t]))
    np.testing.assert_allclose(head[0] + tail[0], whole[0], rtol=1e-13)


# ---------------------------------------------------------------------------
# 4. tails, against the host engine on the same normals
# ---------------------------------------------------------------------------
def _assert_paths_match(plan, normals, **kw):
    """Device paths (launched with **kw) against the host engine on `normals`."""
    zf = _both_signs(plan, normals)
    x, rebate, alive = bgk_barrier.host_paths(plan, zf)
    bound_x, bound_r = fx.path_bounds(plan, zf, x)
    stats, pay = run_paths([[plan]], engine="hip", n_obs=normals.shape[0], want_payoffs=True,
                           **kw)
    assert pay.shape == (1, 1, 2, zf.shape[0])
    assert np.all(np.abs(pay[0, 0, 0] - x) <= bound_x)
    assert np.all(np.abs(pay[0, 0, 1] - rebate) <= bound_r)
    n = zf.shape[0]
    want = (np.sum(x), np.sum(x * x), np.sum(rebate), np.sum(1.0 - alive))
    scale = (bound_x.max(), 2.0 * np.abs(x).max() * bound_x.max() + 1e-300, bound_r.max(),
             bound_x.max())
    for s in range(3):
        assert abs(stats[0, 0, s] - want[s]) <= n * scale[s] + 1e-12 * abs(want[s]), s
    return stats, pay


def test_observation_tails(seven_step_plans, chunk):
    plan = seven_step_plans[2]      # double-out, smoothed, rebate at hit
    assert plan.antithetic
    for n_obs in (1, 255, 256, 257, chunk + 1):
        z = np.random.default_rng(n_obs).standard_normal((n_obs, plan.n_steps))
        _assert_paths_match(plan, z, z=z)


def test_path_count_tails():
    """mc_n_paths 1 and 3 with antithetic: n_half = max(1, n // 2) = 1, two paths."""
    case = _case("dbl_out_call_smooth_rebate_hit_7")
    for n_paths in (1, 3):
        gpu = _pricer(case, mc_n_paths=n_paths)
        host = _pricer(case, engine="host", mc_n_paths=n_paths)
        plan = gpu._job().plan
        assert (plan.n_half, plan.n_sim) == (1, 2)
        z = bgk_barrier.draw_normals("numpy", 42, 1, plan.n_steps)
        x, _, _ = bgk_barrier.host_paths(plan, _both_signs(plan, z))
        bounds = fx.path_bounds(plan, _both_signs(plan, z), x)
        bound = float(bounds[0].max() + bounds[1].max())
        assert abs(gpu.price() - host.price()) <= bound
        assert abs(gpu._last_mc_std_error - host._last_mc_std_error) <= bound


@pytest.mark.parametrize("name", ["do_call_exact_1", "uo_call_exact_3",
                                  "dbl_out_put_exact_rebate_expiry_3"])
def test_step_tails_on_the_device_generator(name, chunk):
    """n_steps 1 and 3: the last Box-Muller pair is half used.  The kernel's
    own normals (fdcn_mc_normals) through the host engine."""
    plan = _pricer(_case(name))._job().plan
    assert plan.n_steps in (1, 3)
    n_obs = 257
    z = capi.mc_normals(n_obs, plan.n_steps, seed=77, stream_id=2, obs_first=10)
    _assert_paths_match(plan, z, seed=77, stream_ids=[2], obs_first=10)


# ---------------------------------------------------------------------------
# 5. statistical parity, device generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["large"], ids=lambda c: c["name"])
def test_statistical_parity_with_the_device_generator(case):
    """2^20 antithetic observations on Philox against the reference's
    2 000 000 NumPy paths: |dprice| <= 5 sqrt(se_ref^2 + se_run^2)."""
    p = _pricer(case, mc_n_paths=2 ** 21, mc_rng="philox", mc_seed=7)
    price = p.price()
    se = p._last_mc_std_error
    bound = 5.0 * math.sqrt(case["mc_std_error"] ** 2 + se ** 2)
    print(f"{case['name']}: price {price:.6f} ref {case['price']:.6f} "
          f"diff {price - case['price']:.3e} bound {bound:.3e} stderr {se:.3e}")
    assert p._job().plan.n_half == 2 ** 20
    assert math.isfinite(se) and 0.0 < se < case["mc_std_error"] * 1.2
    assert abs(price - case["price"]) <= bound


# ---------------------------------------------------------------------------
# 6. cross-check against the single-barrier engine
# ---------------------------------------------------------------------------
def test_cross_check_against_the_single_barrier_engine():
    """An exact-mode up-and-out call without dividends on a grid both engines
    see alike (ACT/360, nine-day steps: every year fraction is a short
    decimal), one supplied z: exponential of the sum here, product of
    exponentials there.  Per observation within 1e-12 * spot."""
    import pandas as pd
    val = dt.date(2025, 7, 28)
    mons = [val + dt.timedelta(days=9 * k) for k in (1, 2, 3, 4)]
    mat = val + dt.timedelta(days=45)
    spot, strike, vol, level, rebate, rate = 229.74, 220.0, 0.26, 250.0, 2.0, 0.073086
    days = pd.date_range(start=val, end=mc_fixture.CURVE_END, freq="D")
    frame = pd.DataFrame({"Date": days.strftime("%Y-%m-%d"), "NACA": rate})
    p = DiscreteBarrierBGKPricer(
        spot=spot, strike=strike, valuation_date=val, maturity_date=mat, option_type="call",
        barrier_type="up-and-out", upper_barrier=level, monitor_dates=mons, rebate_amount=rebate,
        discount_curve=frame, forward_curve=frame, volatility=vol, day_count="ACT/360",
        pricing_method="mc", mc_n_paths=1024, mc_smooth_barrier_eps=0.0,
        mc_smooth_payoff_eps=0.0, engine="hip")
    plan = p._job().plan
    curve = mc_barrier.NacaCurve(frame, valuation_date=val, day_count="ACT/360")
    old = mc_barrier.plan_contract(
        spot=spot, strike=strike, vol=vol, option_type="call", valuation=val, maturity=mat,
        discount_curve=curve, monitor_dates=mons,
        barrier=mc_barrier.BarrierSpec("up-and-out", level),
        rebate=mc_barrier.RebateSpec(rebate, False), include_maturity_monitor=False)
    assert plan.n_steps == old.n_steps == 5
    np.testing.assert_allclose(plan.step[:, :2], old.step[:, :2], rtol=1e-12)
    assert plan.step[:, capi.BGK_S_MONITOR].tolist() == old.step[:, capi.MC_S_MONITOR].tolist()
    n_obs = 512
    z = np.random.default_rng(2025).standard_normal((n_obs, 5))
    # off the decision edges, so that an ulp cannot flip a payoff
    zf = np.concatenate([z, -z], axis=0)
    spots = np.exp(plan.params[0] + np.cumsum(plan.step[:, 0][None, :]
                                              + plan.step[:, 1][None, :] * zf, axis=1))
    assert np.min(np.abs(spots[:, :4] - level)) / level > 1e-9
    assert np.min(np.abs(spots[:, 4] - strike)) / strike > 1e-9
    _, pay = run_paths([[plan]], engine="hip", z=z, want_payoffs=True)
    x = pay[0, 0, 0]
    mine = plan.df_T * (0.5 * (x[:n_obs] + x[n_obs:]))
    _, theirs = mc_barrier.simulate([old], n_obs, True, engine="hip", z=z, want_payoffs=True)
    err = np.abs(mine - theirs[0])
    print(f"cross-check: worst per-observation difference {err.max():.3e} "
          f"(bound {1e-12 * spot:.3e})")
    assert np.count_nonzero(theirs[0] == rebate * old.params[capi.MC_P_DF_T]) > 0
    assert np.all(err <= 1e-12 * spot)


# ---------------------------------------------------------------------------
# 7. device-pointer entry
# ---------------------------------------------------------------------------
def test_dev_entry_matches_the_host_entry(chunk):
    import torch
    G, n_obs = 5, chunk + 77
    groups = []
    for name in ("uo_call_smooth_7", "do_put_exact_rebate_hit_7",
                 "dbl_out_call_smooth_rebate_hit_7"):
        p = _pricer(_case(name))
        groups.append([j.plan for j in p._bumped_jobs(1e-4 * p.spot_price, 1e-4)])
    B = len(groups)
    P = np.stack([np.stack([p.params for p in grp]) for grp in groups])
    S = np.stack([np.stack([p.step for p in grp]) for grp in groups])
    F = np.stack([grp[0].flags for grp in groups]).astype(np.int32)
    F[:, capi.BGK_F_STREAM] = np.arange(B)
    want, want_pay = capi.mc_bgk_batch(P, F, S, n_obs, True, seed=21, want_payoffs=True)
    dev = torch.device("cuda:0")
    dP, dF, dS = (torch.from_numpy(a).to(dev) for a in (P, F, S))
    stats = torch.zeros((B, G, capi.BGK_NSTAT), dtype=torch.float64, device=dev)
    pay = torch.zeros((B, G, 2, 2 * n_obs), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_bgk_plan(n_obs, G)["ws_bytes_per_trade"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    args = (B, G, 7, n_obs, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), None, 21, 0)
    with torch.cuda.stream(stream):
        capi.mc_bgk_batch_dev(*args, stats.data_ptr(), pay.data_ptr(), ws.data_ptr(), ws_bytes,
                              stream.cuda_stream)
    stream.synchronize()
    assert _bitwise(stats.cpu().numpy(), want)
    assert _bitwise(pay.cpu().numpy(), want_pay)
    # library-owned scratch (NULL workspace) gives the same numbers
    stats2 = torch.zeros_like(stats)
    capi.mc_bgk_batch_dev(*args, stats2.data_ptr(), None, None, 0, stream.cuda_stream)
    stream.synchronize()
    assert _bitwise(stats2.cpu().numpy(), want)
    # one byte short: refused on the host, nothing launched
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_bgk_batch_dev(*args, stats.data_ptr(), None, ws.data_ptr(), ws_bytes - 1,
                              stream.cuda_stream)
