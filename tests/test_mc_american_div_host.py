"""Cash dividends on the path of the least-squares Monte Carlo, on the CPU:
the opt-in keyword and the planner's event ordering per pricer class, the
invertible dividend map, identities of the NumPy host engine that owe nothing
to this project, the FD pricers with a dividend against the host LSM (the
tests that need the feature), and the argument checks of the two new C entry
points (nothing is launched).  DESIGN.md section 13.2."""
import math

import numpy as np
import pytest

import lsm_div_cases as dc
import lsm_fixture as lf
import mc_fixture
from backends import oracle_engine
from finite_difference_amd import (analytic, capi, mc_american, mc_barrier, merge_lsm_stats,
                                   plan_american_contract, price_american_mc, simulate_lsm)

BASE = dict(spot=100.0, strike=100.0, vol=0.3, option_type="put", discount_rate=0.05,
            carry_rate=0.03, time_to_expiry=0.5)
N = capi.LSM_SUBRUN
S = capi


def plan(**kw):
    return plan_american_contract(**{**BASE, **kw})


def col(c, k):
    return c.step[:, k].tolist()


# ---------------------------------------------------------------------------
# 1. opt-in: without a dividend nothing changes
# ---------------------------------------------------------------------------
def test_path_mode_without_a_dividend_is_todays_contract_and_run_bitwise():
    kw = dict(n_exercise=6, barrier_type="down-and-out", lower_barrier=90.0,
              monitor_times=[0.25, 0.5], rebate_amount=1.0)
    old = plan(**kw)
    # dividends outside (0, T) are dropped, a zero amount is none
    new = plan(cash_dividends="path", dividends=[(0.0, 1.0), (0.5, 1.0), (0.7, 2.0), (-0.1, 1.0),
                                                 (0.2, 0.0)], **kw)
    assert old.div is None and not old.has_dividends
    assert new.div.tolist() == [0.0] * old.n_steps and not new.has_dividends
    assert np.array_equal(old.step, new.step) and np.array_equal(old.times, new.times)
    assert np.array_equal(old.params, new.params) and np.array_equal(old.flags, new.flags)
    run = dict(engine="host", seed=10, stream_ids=[3], want_values=True, want_coef=True)
    a, b = simulate_lsm([old], 2, True, **run), simulate_lsm([new], 2, True, **run)
    for key in ("stats", "values", "coef"):
        assert np.array_equal(a[key], b[key]), key
    # the facade, with the keyword and without
    cfg = mc_american.LsmConfig(n_subruns=2, seed=10)
    one = mc_american.mc_american_batch([dict(BASE, **kw)], cfg, engine="host")[0]
    two = mc_american.mc_american_batch([dict(BASE, **kw)], cfg, engine="host",
                                        cash_dividends="path")[0]
    assert one == two
    assert price_american_mc(n_subruns=2, seed=10, engine="host", **BASE, **kw) == \
        price_american_mc(n_subruns=2, seed=10, engine="host", cash_dividends="path", **BASE, **kw)


def test_refuse_is_the_default_and_keeps_its_message():
    for kw in (dict(), dict(cash_dividends="refuse")):
        with pytest.raises(ValueError, match="cash dividends are not supported"):
            plan(dividends=[(0.2, 1.0)], **kw)
    p = dc.american_call(oracle_engine(), 100)
    for kw in (dict(), dict(cash_dividends="refuse")):
        with pytest.raises(ValueError, match="cash dividends are not supported"):
            mc_american.contract_from_pricer(p, **kw)


def test_refusals_of_the_path_mode():
    for bad in ("yes", "PATH", None, True):
        with pytest.raises(ValueError, match="cash_dividends"):
            plan(cash_dividends=bad)
        with pytest.raises(ValueError, match="cash_dividends"):
            mc_american.contract_from_pricer(dc.american_call(oracle_engine(), 100),
                                             cash_dividends=bad)
        with pytest.raises(ValueError, match="cash_dividends"):
            mc_american.mc_american_batch([plan()], engine="host", cash_dividends=bad)
        with pytest.raises(ValueError, match="cash_dividends"):
            price_american_mc(plan(), engine="host", cash_dividends=bad)
    for cash in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and >= 0"):
            plan(cash_dividends="path", dividends=[(0.2, cash)])
    with pytest.raises(ValueError, match="sum to the spot"):
        plan(cash_dividends="path", dividends=[(0.1, 60.0), (0.3, 40.0)])
    with pytest.raises(ValueError, match="sum to the spot"):
        plan(cash_dividends="path", dividends=[(0.1, 100.5)])
    # one of them outside the life: the rest stays under the spot
    assert plan(cash_dividends="path", dividends=[(0.1, 60.0), (0.6, 40.0)]).has_dividends


# ---------------------------------------------------------------------------
# 2. the planner's step table on a dividend date
# ---------------------------------------------------------------------------
def test_american_dividend_date_is_two_steps():
    """Exercise on the cum-dividend spot, the dividend, then the monitor test
    and a second exercise on the ex-dividend spot."""
    c = plan(cash_dividends="path", n_exercise=4, dividends=[(0.25, 2.0)],
             barrier_type="up-and-out", upper_barrier=120.0, monitor_times=[0.125, 0.25],
             rebate_amount=1.5, rebate_at_hit=True)
    assert c.times.tolist() == [0.125, 0.25, 0.25, 0.375, 0.5]
    assert c.div.tolist() == [0.0, 0.0, 2.0, 0.0, 0.0] and c.has_dividends
    assert col(c, S.LSM_S_EXERCISE) == [1, 1, 1, 1, 1]
    assert col(c, S.LSM_S_MONITOR) == [1, 0, 1, 0, 0]   # the first of the two: no monitor flag
    first, second = c.step[1], c.step[2]
    assert (second[S.LSM_S_DRIFT], second[S.LSM_S_DIFF], second[S.LSM_S_DF_STEP]) == (0.0, 1e-300,
                                                                                      1.0)
    assert second[S.LSM_S_DF_END] == first[S.LSM_S_DF_END] == math.exp(-0.05 * 0.25)
    assert second[S.LSM_S_REBATE] == first[S.LSM_S_REBATE]
    assert second[S.LSM_S_ISCALE] == first[S.LSM_S_ISCALE]          # ISCALE is left alone
    assert second[S.LSM_S_CENTRE] == math.log(math.exp(first[S.LSM_S_CENTRE]) - 2.0)
    assert c.step[3, S.LSM_S_CENTRE] == second[S.LSM_S_CENTRE] + c.step[3, S.LSM_S_DRIFT]
    plain = plan(n_exercise=4, barrier_type="up-and-out", upper_barrier=120.0,
                 monitor_times=[0.125, 0.25], rebate_amount=1.5, rebate_at_hit=True)
    keep = [0, 1, 3, 4]
    other = [k for k in range(S.LSM_NSTEP) if k not in (S.LSM_S_CENTRE, S.LSM_S_MONITOR)]
    assert np.array_equal(c.step[keep][:, other], plain.step[:, other])
    # a dividend date off the exercise grid is a date of its own, two steps again
    off = plan(cash_dividends="path", n_exercise=2, dividends=[(0.1, 1.0)])
    assert off.times.tolist() == [0.1, 0.1, 0.25, 0.5] and off.div.tolist() == [0, 1.0, 0, 0]
    assert col(off, S.LSM_S_EXERCISE) == [1, 1, 1, 1]
    # every kind, knock-ins included, takes the same form
    ki = plan(cash_dividends="path", n_exercise=2, dividends=[(0.25, 1.0)],
              barrier_type="down-and-in", lower_barrier=90.0, monitor_times=[0.25])
    assert col(ki, S.LSM_S_MONITOR) == [0, 1, 0] and col(ki, S.LSM_S_EXERCISE) == [1, 1, 1]
    # two dividends on one date add up
    both = plan(cash_dividends="path", n_exercise=2, dividends=[(0.25, 1.0), (0.25 + 1e-13, 0.5)])
    assert both.div.tolist() == [0.0, 1.5, 0.0]


def test_bermudan_and_european_dividend_date_is_one_step():
    """The dividend first, then the date's own events on the ex-dividend spot
    (BermudanFDMPricer._job_events: `ex` and `kop` before `div` in tau)."""
    c = plan(cash_dividends="path", exercise_times=[0.1, 0.25, 0.4], barrier_type="up-and-out",
             upper_barrier=120.0, monitor_times=[0.25], dividends=[(0.25, 2.0), (0.3, 1.0)])
    assert c.times.tolist() == [0.1, 0.25, 0.3, 0.4, 0.5]
    assert c.div.tolist() == [0.0, 2.0, 1.0, 0.0, 0.0]
    assert col(c, S.LSM_S_EXERCISE) == [1, 1, 0, 1, 0]
    assert col(c, S.LSM_S_MONITOR) == [0, 1, 0, 0, 0]   # 0.3 is a step of its own, no flag
    assert np.all(c.step[:, S.LSM_S_DIFF] > 1e-3)
    x = math.log(100.0) + c.step[0, S.LSM_S_DRIFT] + c.step[1, S.LSM_S_DRIFT]
    assert c.step[1, S.LSM_S_CENTRE] == math.log(math.exp(x) - 2.0)
    assert np.allclose(c.step[:, S.LSM_S_ISCALE], 1.0 / (0.3 * np.sqrt(c.times)), rtol=1e-13)
    eu = plan(cash_dividends="path", n_exercise=0, dividends=[(0.2, 3.0)])
    assert eu.times.tolist() == [0.2, 0.5] and eu.div.tolist() == [3.0, 0.0]
    assert not eu.step[:, S.LSM_S_EXERCISE].any()


def test_max_steps_counts_the_extra_steps():
    on_grid = [(0.5 * 100 / 511, 1.0)]
    assert plan(cash_dividends="path", n_exercise=511, dividends=on_grid).n_steps == 512
    with pytest.raises(ValueError, match="512"):
        plan(cash_dividends="path", n_exercise=512, dividends=[(0.5 * 100 / 512, 1.0)])
    with pytest.raises(ValueError, match="512"):
        plan(cash_dividends="path", n_exercise=511, dividends=[(0.123456, 1.0)])  # off the grid: 2
    assert plan(cash_dividends="path", n_exercise=510, dividends=[(0.123456, 1.0)]).n_steps == 512


def test_contract_from_pricer_reads_the_pricers_dividends():
    eng = oracle_engine()
    p = dc.american_call(eng, 100)
    (tau, cash), = p._div_times_tau()
    c = dc.fd_contract("american_call", p)
    assert c.n_steps == dc.FD_N_EXERCISE + 2 and c.div.sum() == cash == 8.0
    m = int(np.nonzero(c.div)[0][0])
    assert c.times[m] == c.times[m - 1] == p.time_to_expiry - tau
    assert c.step[m, S.LSM_S_DIFF] == 1e-300 and col(c, S.LSM_S_EXERCISE) == [1.0] * c.n_steps
    # Bermudan: the dividend sits on the exercise date's own step
    b = dc.fd_contract("bermudan_call", dc.bermudan_call(eng, 100))
    assert b.n_steps == 5 and b.div.tolist() == [0.0, 2.5, 0.0, 0.0, 0.0]
    assert col(b, S.LSM_S_EXERCISE) == [1, 1, 1, 1, 0]
    # knock-out: the monitoring flag moves to the ex-dividend step
    k = dc.fd_contract("knock_out_put", dc.knock_out_put(eng, 100))
    m = int(np.nonzero(k.div)[0][0])
    assert k.step[m - 1, S.LSM_S_MONITOR] == 0.0 and k.step[m, S.LSM_S_MONITOR] == 1.0
    assert k.step[m - 1, S.LSM_S_EXERCISE] == k.step[m, S.LSM_S_EXERCISE] == 1.0
    assert int(k.step[:, S.LSM_S_MONITOR].sum()) == 4


# ---------------------------------------------------------------------------
# 3. the dividend map
# ---------------------------------------------------------------------------
def test_the_map_and_its_inverse_round_trip_within_the_derived_bound():
    d = 3.7
    ratio = np.concatenate([np.logspace(-3, 6, 2001), [1.0, 2.0]])
    x = np.log(ratio * d)
    edge = math.log(2.0 * d)
    x = np.concatenate([x, [edge, np.nextafter(edge, 0.0), np.nextafter(edge, 9.0)]])
    y = mc_american._div_forward(x, d)
    back = mc_american._div_backward(y, d)
    err, bound = np.abs(back - x), dc.round_trip_bound(x, d)
    print(f"round trip: worst error / bound {float(np.max(err / bound)):.3f}")
    assert np.all(err <= bound)
    # g itself: s - D from 2 D on, s / 2 below, continuous and increasing
    s = np.exp(x)
    want = np.where(s >= 2.0 * d, s - d, 0.5 * s)
    assert np.allclose(np.exp(y), want, rtol=8 * dc.EPS * (1.0 + np.abs(y)))
    order = np.argsort(x)
    assert np.all(np.diff(y[order]) >= 0.0) and np.all(np.isfinite(y))
    assert abs(float(mc_american._div_forward(np.float64(edge), d)) - math.log(d)) <= 4 * dc.EPS


STEERED_SEED, STEERED_SID = 91, 0


def steered():
    """D comparable to the spot: a quarter of the paths is below 2 D at the
    dividend date and takes the lower branch."""
    return plan(cash_dividends="path", strike=60.0, exercise_times=[0.25, 0.375],
                dividends=[(0.25, 45.0)])


def test_both_branches_against_a_stored_walk_replay():
    """The host engine walks the fit set back through the inverse map; the
    replay stores the forward walk and never inverts.  With every decision at
    least 100 tau_c from its fit the values agree within the Monte Carlo
    bound."""
    c = steered()
    tau_c = lf.TAU_C_REL * 60.0
    for anti in (False, True):
        want, margin, pre, coef = dc.replay_subrun(c, 1, anti, STEERED_SEED, STEERED_SID)
        s_cum = np.exp(pre[0])
        upper, lower = int((s_cum >= 90.0).sum()), int((s_cum < 90.0).sum())
        assert upper >= 16 and lower >= 16, (upper, lower)
        r = mc_american.host_subruns(c, [1], anti, STEERED_SEED, STEERED_SID)
        assert margin >= 100.0 * tau_c and float(r["margin"][0]) >= 100.0 * tau_c
        assert r["coef"][0, :, 4].tolist() == [1.0, 1.0, 0.0]
        u = np.linspace(-4.0, 4.0, 81)[None, :]
        gap = np.abs(lf.cubic(r["coef"][0], u) - lf.cubic(coef, u))
        assert float(gap.max()) <= tau_c, gap.max()
        err = np.abs(r["values"][0] - want)
        bound = 1e-11 * np.abs(want) + 1e-12 * 100.0
        print(f"anti {anti}: {upper} / {lower} paths per branch, worst value error "
              f"{float(np.max(err / bound)):.3e} of its bound")
        assert np.all(err <= bound)
        assert len(np.unique(want)) > 100


def test_parity_batches_keep_their_margins_and_cover_their_menu():
    """The condition of the device parity test, checked where it is cheap:
    at the stored stream ids every contract's host-engine min_margin is at
    least 100 tau_c; and the batches hold what they must."""
    batches = dc.div_batches()
    kinds, types, placed = set(), set(), set()
    for name, (G, anti, seed, cs) in batches.items():
        assert len(cs) <= 8 and 1 <= G <= 3 and len(dc.STREAM_IDS[name]) == len(cs)
        for c, sid in zip(cs, dc.STREAM_IDS[name]):
            r = mc_american.host_subruns(c, range(G), anti, seed, sid)
            assert float(r["margin"].min()) >= dc.min_margin(c), (name, sid)
            kinds.add(int(c.flags[S.LSM_F_KIND]))
            types.add(int(c.flags[S.LSM_F_PUT]))
            rows = np.nonzero(c.div)[0]
            placed |= {"first"} if 0 in rows else set()
            placed |= {"last"} if c.n_steps - 1 in rows and c.n_steps > 1 else set()
            placed |= {"odd" if (i + 1) % 2 else "even" for i in rows}
            placed |= {"consecutive"} if np.any(np.diff(rows) == 1) else set()
            placed |= {"zero-length"} if any(c.step[i, S.LSM_S_DIFF] == 1e-300 for i in rows) \
                else set()
    assert kinds == set(range(7)) and types == {0, 1}
    assert placed == {"first", "last", "odd", "even", "consecutive", "zero-length"}
    assert {cs[0].n_steps for _, _, _, cs in batches.values()} == {1, 2, 3, 8}
    assert {anti for _, anti, _, _ in batches.values()} == {False, True}
    for name in ("m8_div", "m3_div"):  # the BIG_D contract takes both branches
        G, anti, seed, cs = batches[name]
        z = mc_american._path_normals(cs[-1].n_steps, seed, 2 * dc.STREAM_IDS[name][-1], 0, anti)
        pre, _ = dc.stored_walk(cs[-1], z)
        s = np.exp(pre[int(np.nonzero(cs[-1].div)[0][0])])
        assert (s >= 2 * dc.BIG_D).sum() >= 16 and (s < 2 * dc.BIG_D).sum() >= 16


# ---------------------------------------------------------------------------
# 4. facts that owe nothing to this project
# ---------------------------------------------------------------------------
def test_all_zero_div_through_the_dividend_path_is_bitwise_todays_run():
    c = plan(n_exercise=3)
    z = dc.contract("none", "put", c.times, (), range(3), {})
    assert z.div.tolist() == [0.0, 0.0, 0.0] and np.array_equal(z.step, c.step)
    a = mc_american.host_subruns(c, [0, 1], True, 4, 2)
    b = mc_american.host_subruns(z, [0, 1], True, 4, 2)
    for key in ("values", "fit_mean", "coef", "invalid", "margin"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("option_type", ["put", "call"])
def test_initial_dividend_is_black_scholes_at_spot_minus_d(option_type):
    eu = plan(n_exercise=0, option_type=option_type, strike=95.0)
    c = dc.with_initial_dividend(eu, 6.0)
    r = price_american_mc(c, n_subruns=32, seed=5, engine="host")
    ref = float(analytic.black_scholes(option_type[0], 94.0, 95.0, 0.05, 0.03, 0.3, 0.5))
    print(f"{option_type}: {r['price']:.5f} +- {r['stderr']:.5f}, Black-Scholes {ref:.5f}")
    assert r["steps"] == 2 and r["stderr"] > 0.0
    assert abs(r["price"] - ref) <= 5.0 * r["stderr"]
    plain = price_american_mc(eu, n_subruns=32, seed=5, engine="host")
    assert abs(plain["price"] - ref) > 5.0 * plain["stderr"]  # the dividend is seen


def test_european_put_agrees_with_the_barrier_monte_carlo():
    """price_discrete_barrier_mc puts the cash dividend on the path itself
    (FDCN_MC_F_DIV_FIRST); its barrier is out of reach here."""
    import datetime as dt
    val, mat, day = dt.date(2025, 7, 28), dt.date(2025, 9, 29), dt.date(2025, 8, 25)
    naca = 0.073086
    curve = mc_fixture.flat_curve(mc_barrier, naca, val)
    ref = mc_barrier.price_discrete_barrier_mc(
        spot=100.0, strike=102.0, vol=0.3, option_type="put", valuation=val, maturity=mat,
        discount_curve=curve, dividends=[(day, 3.0)], monitor_dates=[day],
        barrier=mc_barrier.BarrierSpec("up-and-out", 1e9), engine="host", rng="numpy")
    rate = math.log(1.0 + naca)
    r = price_american_mc(spot=100.0, strike=102.0, vol=0.3, option_type="put", discount_rate=rate,
                          carry_rate=rate, time_to_expiry=(mat - val).days / 365.0, n_exercise=0,
                          dividends=[((day - val).days / 365.0, 3.0)], cash_dividends="path",
                          n_subruns=32, seed=6, engine="host")
    both = math.hypot(r["stderr"], ref["stderr"])
    print(f"LSM {r['price']:.5f} +- {r['stderr']:.5f}, barrier MC {ref['price']:.5f} +- "
          f"{ref['stderr']:.5f}")
    assert r["steps"] == 2 and abs(r["price"] - ref["price"]) <= 5.0 * both


def test_european_in_plus_out_is_vanilla_path_by_path_with_a_dividend():
    """The barrier on the out-of-the-money side of a put (the exercise floor at
    the hit is max(0, 0)), zero rebate, the dividend on a monitored step."""
    t, mon = [0.1, 0.3, 0.5], (0, 1, 2)
    parts = [dc.contract(k, "put", t, mon if k != "none" else (), (), {1: 4.0}, upper=108.0)
             for k in ("none", "up-and-out", "up-and-in")]
    v = [simulate_lsm([c], 1, False, engine="host", seed=2, stream_ids=[1],
                      want_values=True)["values"][0] for c in parts]
    assert (v[1] > 0).any() and (v[2] > 0).any() and ((v[1] > 0) & (v[2] > 0)).sum() == 0
    assert np.array_equal(v[1] + v[2], v[0])
    without = dc.contract("none", "put", t, (), (), {})
    v0 = simulate_lsm([without], 1, False, engine="host", seed=2, stream_ids=[1],
                      want_values=True)["values"][0]
    assert v[0].mean() > v0.mean() + 1.0  # the put gains most of the dividend


def test_merged_shards_equal_the_whole_with_a_dividend():
    c = plan(cash_dividends="path", n_exercise=4, dividends=[(0.2, 2.0)])
    cfg = mc_american.LsmConfig(n_subruns=4, antithetic=True, seed=10)
    whole = mc_american.mc_american_batch([c], cfg, engine="host", stream_ids=[3])[0]
    parts = [mc_american.mc_american_batch([c], cfg, engine="host", stream_ids=[3],
                                           subrun_range=r)[0] for r in (range(0, 1), range(1, 4))]
    m = merge_lsm_stats(parts)
    assert m["price"] == pytest.approx(whole["price"], rel=1e-14)
    assert m["stderr"] == pytest.approx(whole["stderr"], rel=1e-10)
    assert whole["steps"] == 6


# ---------------------------------------------------------------------------
# 5. the FD pricers with a dividend against the host LSM
# ---------------------------------------------------------------------------
def _fd_and_lsm(name):
    eng = oracle_engine()
    make = dc.FD_TRADES[name]
    fd_200, fd_400 = float(make(eng, 200).price_log()), float(make(eng, 400).price_log())
    c = dc.fd_contract(name, make(eng, 400))
    assert c.has_dividends and c.n_steps <= 40
    r = price_american_mc(c, n_subruns=32, engine="host")
    bound = lf.fd_gap_bound(fd_400, fd_200, r["stderr"])
    print(f"{name}: FD 200 / 400 {fd_200:.6f} / {fd_400:.6f}, LSM {r['price']:.6f} +- "
          f"{r['stderr']:.6f} ({c.n_steps} steps), gap {abs(fd_400 - r['price']):.6f} of "
          f"{bound:.6f}")
    return fd_400, r, bound


def test_american_call_is_exercised_an_instant_before_the_dividend():
    """|FD_400 - LSM| <= 1 % FD_400 + 5 s + 2 |FD_400 - FD_200|.  From the FD
    side alone the early-exercise premium -- the American price less the same
    trade exercised at maturity only -- is more than ten times that bound: a
    planner without the exercise on the cum-dividend spot could not pass."""
    eng = oracle_engine()
    american = float(dc.american_call(eng, 400).price_log())
    european = float(dc.american_call(eng, 400, cls=dc.BermudanFDMPricer).price_log())
    fd, r, bound = _fd_and_lsm("american_call")
    print(f"premium {american - european:.6f} = {(american - european) / bound:.1f} bounds")
    assert fd == american and american - european > 10.0 * bound
    assert abs(fd - r["price"]) <= bound


def test_bermudan_call_with_a_dividend_on_an_exercise_date():
    """The same bound; the trade without its dividend is outside it, so the
    dividend is on the path."""
    fd, r, bound = _fd_and_lsm("bermudan_call")
    assert abs(fd - r["price"]) <= bound
    without = float(dc.bermudan_call(oracle_engine(), 400, dividend=False).price_log())
    assert abs(without - r["price"]) > bound


def test_knock_out_put_with_a_dividend_on_a_monitoring_date():
    fd, r, bound = _fd_and_lsm("knock_out_put")
    assert abs(fd - r["price"]) <= bound
    without = float(dc.knock_out_put(oracle_engine(), 400, dividend=False).price_log())
    assert abs(without - r["price"]) > bound


# ---------------------------------------------------------------------------
# 6. the C entry points (nothing launched)
# ---------------------------------------------------------------------------
EINVAL, ENODEV = -1, -3


def test_library_exports_the_two_symbols_at_abi_8():
    import ctypes
    raw = ctypes.CDLL(capi.LIB_PATH)
    header = open(capi.HEADER_PATH).read()
    for name in ("fdcn_mc_lsm_div_batch", "fdcn_mc_lsm_div_batch_dev"):
        assert name in capi.EXPORTED and hasattr(raw, name) and f"int {name}(" in header
    assert capi.lib().fdcn_abi_version() == capi.ABI_VERSION == 8
    assert "#define FDCN_LSM_NSTEP 9" in header


def _host(c, div, G=1):
    P, F, St = mc_american._stack([c], [0])
    stats = np.empty((1, capi.LSM_NSTAT))
    D = None if div is None else np.ascontiguousarray(div, dtype=np.float64)
    L = capi.lib()
    rc = L.fdcn_mc_lsm_div_batch(1, c.n_steps, G, 1, P.ctypes.data, F.ctypes.data, St.ctypes.data,
                                 None if D is None else D.ctypes.data, 1, 0, stats.ctypes.data,
                                 None, None)
    return rc, L.fdcn_last_error().decode()


def test_host_entry_checks_the_dividends_before_the_device():
    c = plan(n_exercise=3)
    assert _host(c, [0.0, 2.0, 1.0])[0] in (0, ENODEV)   # the last step may pay one
    rc, msg = _host(c, None)
    assert rc == EINVAL and "div is NULL" in msg
    for bad, word in ((-1.0, "negative"), (float("nan"), "not finite"),
                      (float("inf"), "not finite")):
        rc, msg = _host(c, [0.0, bad, 0.0])
        assert rc == EINVAL and word in msg and "step 2" in msg, (bad, rc, msg)
    # the contract checks of the plain entry still come first
    c.step[1, capi.LSM_S_DIFF] = 0.0
    rc, msg = _host(c, [0.0, 0.0, 0.0])
    assert rc == EINVAL and "sigma" in msg
    rc, msg = _host(plan(n_exercise=3), [0.0] * 3, G=0)
    assert rc == EINVAL and "G must" in msg


def test_dev_entry_argument_checks():
    L = capi.lib()
    fake = 4096  # never dereferenced: validation comes first

    def dev(div=fake, ws_bytes=1 << 20, stats=fake, n_steps=7):
        rc = L.fdcn_mc_lsm_div_batch_dev(3, n_steps, 5, 1, fake, fake, fake, div, 1, 0, stats,
                                         None, None, fake, ws_bytes, None)
        return rc, L.fdcn_last_error().decode()
    rc, msg = dev(div=None)
    assert rc == EINVAL and "div is NULL" in msg
    rc, msg = dev(stats=None)
    assert rc == EINVAL and "stats is NULL" in msg
    rc, msg = dev(n_steps=513)
    assert rc == EINVAL and "n_steps" in msg
    need = 3 * capi.mc_lsm_plan(7, 5, True)["ws_bytes_per_contract"]
    rc, msg = dev(ws_bytes=need - 1)
    assert rc == EINVAL and "workspace" in msg
