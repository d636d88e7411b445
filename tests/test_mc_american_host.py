"""Least-squares Monte Carlo for American options with discrete barriers, on
the CPU: plan building and its refusals, identities of the NumPy host engine,
the FD gap the feature exists for (against the fixture of
golden/make_golden_lsm.py), and the argument checks of the three C entry
points (nothing is launched)."""
import math

import numpy as np
import pytest

import lsm_fixture as lf
from backends import oracle_engine
from conftest import load_golden
from finite_difference_amd import (AmericanBarrierFDMPricer, capi, mc_american, merge_lsm_stats,
                                   plan_american_contract, price_american_mc, simulate_lsm)
from finite_difference_amd.barrier import rebate_value

GOLDEN = load_golden("lsm_cases.json")
BASE = dict(spot=100.0, strike=100.0, vol=0.3, option_type="put", discount_rate=0.05,
            carry_rate=0.03, time_to_expiry=0.5)
N = capi.LSM_SUBRUN


def plan(**kw):
    return plan_american_contract(**{**BASE, **kw})


# ---------------------------------------------------------------------------
# 1. plan building
# ---------------------------------------------------------------------------
def test_step_grid_is_the_merged_union_with_flags():
    mon = [0.1, 0.25 + 3e-13, 0.3, 0.5 - 2e-13, 0.7, -0.1]  # 0.25 and T merge; two outside
    c = plan(barrier_type="up-and-out", upper_barrier=120.0, monitor_times=mon, n_exercise=4)
    assert np.allclose(c.times, [0.1, 0.125, 0.25, 0.3, 0.375, 0.5], rtol=0, atol=1e-12)
    assert c.times[-1] == 0.5
    S = c.step
    assert S[:, capi.LSM_S_EXERCISE].tolist() == [0, 1, 1, 0, 1, 1]
    assert S[:, capi.LSM_S_MONITOR].tolist() == [1, 0, 1, 1, 0, 1]
    dt = np.diff(np.concatenate([[0.0], c.times]))
    assert np.allclose(S[:, capi.LSM_S_DRIFT], (0.03 - 0.045) * dt, rtol=1e-15)
    assert np.allclose(S[:, capi.LSM_S_DIFF], 0.3 * np.sqrt(dt), rtol=1e-15)
    assert np.allclose(S[:, capi.LSM_S_DF_STEP], np.exp(-0.05 * dt), rtol=1e-15)
    assert np.allclose(S[:, capi.LSM_S_DF_END], np.exp(-0.05 * c.times), rtol=1e-15)
    assert np.allclose(np.cumprod(S[:, capi.LSM_S_DF_STEP]), S[:, capi.LSM_S_DF_END], rtol=1e-14)
    assert np.allclose(S[:, capi.LSM_S_CENTRE],
                       math.log(100.0) + np.cumsum(S[:, capi.LSM_S_DRIFT]), rtol=1e-15)
    assert np.allclose(S[:, capi.LSM_S_ISCALE], 1.0 / (0.3 * np.sqrt(c.times)), rtol=1e-13)
    assert c.flags.tolist() == [1, capi.LSM_KIND["up-and-out"], 0]
    assert c.params.tolist() == [100.0, 100.0, 0.0, 120.0]
    # without a barrier the monitor times are no steps; no exercise dates: European
    assert plan(monitor_times=mon, n_exercise=4).n_steps == 4
    eu = plan(barrier_type="down-and-in", lower_barrier=90.0, monitor_times=[0.2], n_exercise=0)
    assert eu.times.tolist() == [0.2, 0.5] and not eu.step[:, capi.LSM_S_EXERCISE].any()
    ex = plan(exercise_times=[0.3, 0.1])
    assert ex.times.tolist() == [0.1, 0.3, 0.5]
    assert ex.step[:, capi.LSM_S_EXERCISE].tolist() == [1, 1, 0]


@pytest.mark.parametrize("kind,at_hit", [("up-and-out", True), ("up-and-out", False),
                                         ("double-out", False), ("up-and-in", False)])
def test_rebate_column_is_the_fd_pricers_number(kind, at_hit):
    c = plan(barrier_type=kind, upper_barrier=120.0, lower_barrier=80.0, monitor_times=[0.2, 0.4],
             rebate_amount=2.5, rebate_at_hit=at_hit, n_exercise=8)
    want = [rebate_value(2.5, at_hit, 0.03, 0.5 - t) for t in c.times]
    assert c.step[:, capi.LSM_S_REBATE].tolist() == want
    assert c.step[-1, capi.LSM_S_REBATE] == 2.5
    assert not plan(rebate_amount=2.5).step[:, capi.LSM_S_REBATE].any()


def test_contract_from_pricer_reads_the_snapped_trade():
    p = lf.trade_pricer("up-and-out", oracle_engine(), 400)
    c = mc_american.contract_from_pricer(p, n_exercise=16)
    assert c.params[0] == p.spot_snapped and c.params[1] == p.strike_snapped
    assert (c.params[0], c.params[1]) != (p.spot, p.strike)
    taus, at_mat = p._monitor_taus()
    assert at_mat and int(c.step[:, capi.LSM_S_MONITOR].sum()) == len(taus) + 1
    mon_t = c.times[c.step[:, capi.LSM_S_MONITOR] != 0.0]
    assert np.allclose(mon_t[:-1], sorted(p.time_to_expiry - t for t in taus), atol=1e-12)
    assert int(c.step[:, capi.LSM_S_EXERCISE].sum()) == 16
    assert c.step[3, capi.LSM_S_DF_END] == math.exp(-p.discount_rate_nacc * c.times[3])
    assert c.barrier_type == "up-and-out" and c.fixed_price is None
    # answered by the pricer's own rule, without a launch (engine="hip" on a
    # machine without a GPU would raise)
    hit = lf.trade_pricer("up-and-out", oracle_engine(), 400)
    hit.already_hit, hit.rebate_amount = True, 3.0
    r = price_american_mc(mc_american.contract_from_pricer(hit), engine="hip")
    assert r["price"] == hit.price_log() == 3.0 and r["n_paths"] == 0 and r["stderr"] == 0.0
    ki = lf.trade_pricer("up-and-in", oracle_engine(), 400)
    ki.already_in = True
    assert mc_american.contract_from_pricer(ki).barrier_type == "none"
    never = lf.trade_pricer("up-and-in", oracle_engine(), 400)
    never.monitor_dates, never.rebate_amount = [], 2.0
    r = price_american_mc(mc_american.contract_from_pricer(never), engine="hip")
    assert r["price"] == never.price_log() > 0.0


def test_refusals():
    with pytest.raises(ValueError, match="dividend"):
        plan(dividends=[(0.2, 1.0)])
    cls, kw = lf.TRADES["up-and-out"]
    div = AmericanBarrierFDMPricer(
        spot=229.74, strike=220.0, valuation_date=lf.VAL, maturity_date=lf.MAT, sigma=0.26,
        option_type="put", discount_curve=lf.CURVE, forward_curve=lf.CURVE,
        dividend_schedule=[(lf.WEEKDAYS[5], 1.0)], engine=oracle_engine(), **kw)
    with pytest.raises(ValueError, match="dividend"):
        mc_american.contract_from_pricer(div)
    for vol in (0.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="vol"):
            plan(vol=vol)
    with pytest.raises(ValueError, match="512"):
        plan(n_exercise=513)
    assert plan(n_exercise=512).n_steps == 512
    with pytest.raises(ValueError, match="rebate_at_hit"):
        plan(barrier_type="up-and-in", upper_barrier=120.0, rebate_at_hit=True)
    with pytest.raises(ValueError, match="upper_barrier"):
        plan(barrier_type="double-out", lower_barrier=90.0)
    with pytest.raises(ValueError, match="barrier_type"):
        plan(barrier_type="sideways")
    c = plan(n_exercise=2)
    with pytest.raises(ValueError, match="subrun_first"):
        simulate_lsm([c], 1, True, engine="host", subrun_first=0.5)
    with pytest.raises(ValueError, match="subrun_first"):
        simulate_lsm([c], 1, True, engine="host", subrun_first=-1)
    with pytest.raises(ValueError, match="stream id"):
        simulate_lsm([c], 1, True, engine="host", stream_ids=[2 ** 30])
    with pytest.raises(ValueError, match="share n_steps"):
        simulate_lsm([c, plan(n_exercise=3)], 1, True, engine="host")
    with pytest.raises(ValueError, match="subrun_range"):
        mc_american.mc_american_batch([c], mc_american.LsmConfig(n_subruns=4), engine="host",
                                      subrun_range=range(2, 5))


# ---------------------------------------------------------------------------
# 2. host-engine identities
# ---------------------------------------------------------------------------
def _price_normals(c, g, anti, seed, sid):
    per = mc_american.obs_per_subrun(anti)
    return mc_american._path_normals(c.n_steps, seed, 2 * sid + 1, g * per, anti)


@pytest.mark.parametrize("anti", [False, True])
def test_one_step_is_the_discounted_mean_payoff(anti):
    c = plan(n_exercise=1, strike=104.0)
    r = simulate_lsm([c], 2, anti, engine="host", seed=3, stream_ids=[9], want_values=True)
    want = []
    for g in range(2):
        z = _price_normals(c, g, anti, 3, 9)[:, 0]
        x = float(np.log(100.0)) + (c.step[0, capi.LSM_S_DRIFT] + c.step[0, capi.LSM_S_DIFF] * z)
        want.append(np.maximum(104.0 - np.exp(x), 0.0) * c.step[0, capi.LSM_S_DF_END])
    want = np.concatenate(want)
    assert np.array_equal(r["values"][0], want)
    assert r["stats"][0, capi.LSM_O_PRICE] == pytest.approx(want.mean(), rel=1e-14)
    assert r["stats"][0, capi.LSM_O_INVALID] == 0 and math.isinf(r["stats"][0, 7])
    if anti:  # path p and its mirror are slots k and k + 1 of one thread
        z = _price_normals(c, 0, True, 3, 9)[:, 0].reshape(16, 256)
        assert np.array_equal(z[0::2], -z[1::2])


def test_unreachable_knock_out_is_kind_none_value_for_value():
    mon = [0.1, 0.2, 0.3, 0.4, 0.5]
    none = plan(n_exercise=5)
    ko = plan(n_exercise=5, barrier_type="double-out", lower_barrier=1e-3, upper_barrier=1e6,
              monitor_times=mon, rebate_amount=5.0)
    kw = dict(engine="host", seed=8, stream_ids=[4], want_values=True, want_coef=True)
    a, b = simulate_lsm([none], 2, True, **kw), simulate_lsm([ko], 2, True, **kw)
    assert np.array_equal(a["values"], b["values"]) and np.array_equal(a["coef"], b["coef"])
    assert np.array_equal(a["stats"], b["stats"])


def test_european_in_plus_out_is_kind_none_path_by_path():
    """Zero rebate, no exercise flags, an up barrier above a put's strike (the
    exercise floor at the hit is then max(0, 0)): in + out = vanilla."""
    mon = [0.1, 0.3, 0.5]
    parts = [plan(n_exercise=0, exercise_times=mon)]  # the same grid, then no exercise
    parts += [plan(n_exercise=0, barrier_type=k, upper_barrier=108.0, monitor_times=mon)
              for k in ("up-and-out", "up-and-in")]
    parts[0].step[:, capi.LSM_S_EXERCISE] = 0.0
    v = [simulate_lsm([c], 1, False, engine="host", seed=2, stream_ids=[1],
                      want_values=True)["values"][0] for c in parts]
    assert (v[1] > 0).any() and (v[2] > 0).any() and ((v[1] > 0) & (v[2] > 0)).sum() == 0
    assert np.array_equal(v[1] + v[2], v[0])


def test_deep_in_the_money_put_is_exercised_at_the_first_step():
    """Strike 100 x spot: waiting one step costs K r dt ~ 31 against a fit whose
    error stays of the order of the spot's own spread, tails included."""
    c = plan(strike=10000.0, n_exercise=8)
    r = simulate_lsm([c], 1, False, engine="host", seed=6, stream_ids=[0], want_values=True)
    z = _price_normals(c, 0, False, 6, 0)[:, 0]
    x = float(np.log(100.0)) + (c.step[0, capi.LSM_S_DRIFT] + c.step[0, capi.LSM_S_DIFF] * z)
    want = (10000.0 - np.exp(x)) * c.step[0, capi.LSM_S_DF_END]
    assert np.array_equal(r["values"][0], want)
    assert r["stats"][0, capi.LSM_O_INVALID] == 0


def test_merged_shards_equal_the_whole():
    c = plan(n_exercise=6, barrier_type="down-and-out", lower_barrier=90.0,
             monitor_times=[0.25, 0.5], rebate_amount=1.0)
    cfg = mc_american.LsmConfig(n_subruns=5, antithetic=True, seed=10)
    whole = mc_american.mc_american_batch([c], cfg, engine="host", stream_ids=[3])[0]
    parts = [mc_american.mc_american_batch([c], cfg, engine="host", stream_ids=[3],
                                           subrun_range=r)[0] for r in (range(0, 2), range(2, 5))]
    m = merge_lsm_stats(parts)
    assert m["n_subruns"] == 5
    assert m["price"] == pytest.approx(whole["price"], rel=1e-14)
    assert m["stderr"] == pytest.approx(whole["stderr"], rel=1e-10)
    assert whole["n_paths"] == 5 * N and whole["ci_95"][0] < whole["price"] < whole["ci_95"][1]
    assert set(price_american_mc(c, n_subruns=1, engine="host")) == {
        "price", "stderr", "ci_95", "fit_value", "fit_stderr", "n_paths", "n_subruns", "steps",
        "invalid_fit_steps", "min_margin", "barrier_type"}


def test_fixture_batches_keep_their_margins():
    """The condition of the device parity test, checked where it is cheap: at
    the fixture's stream ids every batch contract's host-engine min_margin is
    the recorded one and at least 100 tau_c."""
    assert GOLDEN["min_margin_required"] == lf.MIN_MARGIN == 100 * lf.TAU_C_REL * lf.BATCH_STRIKE
    for name, (G, anti, seed, kws) in lf.batches().items():
        fix = GOLDEN["batches"][name]
        for c, sid, want in zip(lf.plan_batch(kws), fix["stream_ids"], fix["min_margin"]):
            m = float(mc_american.host_subruns(c, range(G), anti, seed, sid)["margin"].min())
            assert lf.finite(m) == want and m >= lf.MIN_MARGIN, (name, sid, m)


# ---------------------------------------------------------------------------
# 3. the FD gap
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lf.TRADES))
def test_fd_price_against_the_out_of_sample_monte_carlo(name):
    """|FD_3200 - LSM| <= 1 % FD_3200 + 5 s + 2 |FD_3200 - FD_1600| on the
    fixture's numbers (oracle-engine FD, host-engine LSM at G = 1 024), and the
    host engine re-run at G = 64 reproduces the fixture's price within
    5 sqrt(s^2 + s_64^2)."""
    fix = GOLDEN["trades"][name]
    gap = abs(fix["fd_3200"] - fix["price"])
    bound = lf.fd_gap_bound(fix["fd_3200"], fix["fd_1600"], fix["stderr"])
    print(f"{name}: FD 1600 / 3200 {fix['fd_1600']:.6f} / {fix['fd_3200']:.6f}, LSM "
          f"{fix['price']:.6f} +- {fix['stderr']:.6f} (in-sample {fix['fit_value']:.6f}), gap "
          f"{gap:.6f} of {bound:.6f}")
    assert fix["n_subruns"] >= 1024
    assert gap <= bound
    c = mc_american.contract_from_pricer(lf.trade_pricer(name, oracle_engine(), 400))
    assert (float(c.params[0]), float(c.params[1]), c.n_steps) == (fix["spot"], fix["strike"],
                                                                   fix["n_steps"])
    r = price_american_mc(c, n_subruns=64, seed=fix["seed"] + 1, stream_id=fix["stream_id"],
                          engine="host")
    assert abs(r["price"] - fix["price"]) <= 5.0 * math.hypot(fix["stderr"], r["stderr"])


# ---------------------------------------------------------------------------
# 4. the C entry points' argument checks (nothing launched)
# ---------------------------------------------------------------------------
EINVAL, ENODEV = -1, -3


def _dev(B=3, n_steps=7, G=5, anti=1, obs_first=0, ws_bytes=1 << 20, null=None):
    L = capi.lib()
    fake = 4096  # never dereferenced: validation comes first
    ptr = {k: fake for k in ("params", "flags", "step", "stats", "ws")}
    if null:
        ptr[null] = None
    rc = L.fdcn_mc_lsm_batch_dev(B, n_steps, G, anti, ptr["params"], ptr["flags"], ptr["step"], 1,
                                 obs_first, ptr["stats"], None, None, ptr["ws"], ws_bytes, None)
    return rc, L.fdcn_last_error().decode()


def test_plan_entry_and_dev_entry_argument_checks():
    p = capi.mc_lsm_plan(7, 5, True)
    assert p == dict(obs_per_subrun=2048, ws_bytes_per_contract=5 * 4 * 8,
                     values_per_contract=5 * 4096, coef_per_contract=5 * 7 * 5)
    assert capi.mc_lsm_plan(512, 1, False)["obs_per_subrun"] == 4096
    for bad in ((0, 1, True), (513, 1, True), (7, 0, True)):
        with pytest.raises(capi.FdcnError):
            capi.mc_lsm_plan(*bad)
    need = 3 * p["ws_bytes_per_contract"]
    rc, msg = _dev(ws_bytes=need - 1)
    assert rc == EINVAL and "workspace" in msg
    for kw, word in ((dict(B=0), "B must"), (dict(G=0), "G must"), (dict(n_steps=0), "n_steps"),
                     (dict(n_steps=513), "n_steps"), (dict(anti=2), "antithetic"),
                     (dict(obs_first=2047), "obs_first"), (dict(obs_first=-2048), "obs_first"),
                     (dict(anti=0, obs_first=2048), "obs_first"),
                     (dict(null="flags"), "flags is NULL"), (dict(null="stats"), "stats is NULL")):
        rc, msg = _dev(**kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)


def _host(c, *, kind=None, stream=0, G=1, obs_first=0):
    P, F, S = mc_american._stack([c], [0])
    F[0, capi.LSM_F_STREAM] = stream
    if kind is not None:
        F[0, capi.LSM_F_KIND] = kind
    stats = np.empty((1, capi.LSM_NSTAT))
    L = capi.lib()
    rc = L.fdcn_mc_lsm_batch(1, c.n_steps, G, 1, P.ctypes.data, F.ctypes.data, S.ctypes.data, 1,
                             obs_first, stats.ctypes.data, None, None)
    return rc, L.fdcn_last_error().decode()


def test_host_entry_checks_the_contracts_before_the_device():
    c = plan(n_exercise=3, barrier_type="double-out", lower_barrier=80.0, upper_barrier=120.0,
             monitor_times=[0.5])
    assert _host(c)[0] in (0, ENODEV)  # valid: runs, or finds no device here
    for kw, word in ((dict(kind=7), "kind"), (dict(stream=2 ** 30), "stream id"),
                     (dict(stream=-1), "stream id"), (dict(obs_first=100), "obs_first")):
        rc, msg = _host(c, **kw)
        assert rc == EINVAL and word in msg, (kw, rc, msg)
    for col, value, word in ((capi.LSM_S_DIFF, 0.0, "sigma"), (capi.LSM_S_ISCALE, -1.0, "ISCALE"),
                             (capi.LSM_S_REBATE, float("inf"), "finite")):
        bad = plan(n_exercise=3)
        bad.step[1, col] = value
        rc, msg = _host(bad)
        assert rc == EINVAL and word in msg, (col, rc, msg)
    for k, value, word in ((capi.LSM_P_SPOT, 0.0, "spot"), (capi.LSM_P_STRIKE, -1.0, "strike"),
                           (capi.LSM_P_LOWER, 0.0, "lower"), (capi.LSM_P_UPPER, 70.0, "below")):
        bad = plan(n_exercise=3, barrier_type="double-out", lower_barrier=80.0,
                   upper_barrier=120.0, monitor_times=[0.5])
        bad.params[k] = value
        rc, msg = _host(bad)
        assert rc == EINVAL and word in msg, (k, rc, msg)
