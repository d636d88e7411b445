"""AmericanBarrierFDMPricer host logic on the CPU oracle: an American option
with a discretely monitored knock-out is the Ikonen-Toivanen march cut at the
monitoring dates, with V <- max(payoff, rebate) on the knocked nodes at each
date (american_barrier.py).  There is no reference implementation of this
product; the checks are identities with the vanilla pricer, hand-composed
segment chains, bounds, and the convergence behaviour that tells the
exercise floor from the plain projection ("American knock-out")."""
import datetime as dt

import numpy as np
import pytest

from backends import oracle_engine
from conftest import load_golden
from finite_difference_amd import AmericanBarrierFDMPricer, market
from finite_difference_amd.american import AmericanFDMPricer, prefetch_many

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
CASES = load_golden("american_cases.json")["cases"]
WEEKDAYS = [VAL + dt.timedelta(days=k) for k in range(32)
            if (VAL + dt.timedelta(days=k)).weekday() < 5]
FIVE = [VAL + dt.timedelta(days=k) for k in (0, 4, 10, 15, 22, 31)]  # valuation: skipped
CURVE = market.iso_curve(market.create_rate_df(0.073086))


def golden_kw(case, engine):
    inp = case["inputs"]
    curve = market.iso_curve(market.create_rate_df(inp["naca"]))
    divs = [(dt.date.fromisoformat(d), a) for d, a in inp["divs"]]
    return dict(spot=inp["spot"], strike=inp["strike"], valuation_date=VAL, maturity_date=MAT,
                sigma=inp["sigma"], option_type=inp["option_type"], discount_curve=curve,
                forward_curve=curve, dividend_schedule=divs, num_space_nodes=inp["N"],
                num_time_steps=inp["M"], rannacher_steps=2, engine=engine)


def trade(engine, option_type="put", strike=220.0, n=400, m=400, divs=None, **barrier):
    """The trade of the design table: spot 229.74, sigma 0.26, flat NACA
    0.073086, one month."""
    return AmericanBarrierFDMPricer(
        spot=229.74, strike=strike, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
        option_type=option_type, discount_curve=CURVE, forward_curve=CURVE,
        dividend_schedule=divs, num_space_nodes=n, num_time_steps=m, rannacher_steps=2,
        engine=engine, **barrier)


def vanilla(engine, option_type="put", strike=220.0, n=400, m=400, divs=None):
    return AmericanFDMPricer(
        spot=229.74, strike=strike, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
        option_type=option_type, discount_curve=CURVE, forward_curve=CURVE,
        dividend_schedule=divs, num_space_nodes=n, num_time_steps=m, rannacher_steps=2,
        engine=engine)


def compose(p, engine, it, floor, n_time=None):
    """The chain of p's own segments and events marched by hand: every
    segment one engine.run (Ikonen-Toivanen, or plain Crank-Nicolson with
    it=False), every event applied here in NumPy -- with the exercise floor
    max(payoff, R) or the plain projection V <- R on the knocked nodes."""
    p._build_log_grid()
    events, pts, steps, restart = p._job_events(n_time or p.num_time_steps)
    pay = p._payoff_array()
    j = np.arange(pay.shape[0])

    def knock(v, ko_lo, ko_hi, reb):
        knocked = (j <= ko_lo) | (j >= ko_hi)
        return np.where(knocked, np.maximum(pay, reb) if floor else reb, v)

    v = pay
    if p._monitor_taus()[1]:
        v = knock(v, *p._ko_event(0.0)[1:])
    for seg, ns in enumerate(steps):
        s = p._segment_solve(v, pts[seg], pts[seg + 1], ns, restart[seg])
        if not it:
            s.it, s.payoff = False, None
        v = engine.run([s])[0]
        if seg < len(events):
            for e in events[seg]:
                v = (np.asarray(p._apply_dividend_jump(v, e[1])) if e[0] == "div"
                     else knock(v, *e[1:]))
    return np.asarray(v), steps


# ------------------------------------------------------------------ identity
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("barrier", [
    dict(barrier_type="none", lower_barrier=150.0, monitor_dates=WEEKDAYS),
    dict(barrier_type="down-and-out", lower_barrier=150.0, monitor_dates=[]),
    dict(barrier_type="double-out", lower_barrier=150.0, upper_barrier=200.0,
         monitor_dates=[VAL, VAL - dt.timedelta(days=3), MAT + dt.timedelta(days=1)]),
], ids=["none", "no_dates", "dates_outside"])
def test_without_a_usable_barrier_it_is_the_vanilla_pricer(case, barrier):
    a = AmericanFDMPricer(**golden_kw(case, oracle_engine()))
    b = AmericanBarrierFDMPricer(**golden_kw(case, oracle_engine()), **barrier)
    assert b._solve_grid() == a._solve_grid() == case["V"]
    assert b.s_nodes == a.s_nodes
    assert b.price_log2() == a.price_log2() == case["price_log2"]
    assert b.greeks_log2() == a.greeks_log2() == case["greeks_log2"]


# ------------------------------------------------------- no-exercise identity
@pytest.mark.parametrize("n,m", [(400, 400), (128, 96)])
def test_call_never_exercised_equals_the_european_chain(n, m):
    """Down-and-out call, carry = discount, no dividends: early exercise
    never binds and the floor max(payoff, 0) is 0 below the barrier, so the
    American chain equals plain Crank-Nicolson segments with the plain
    projection, node for node."""
    eng = oracle_engine()
    kw = dict(option_type="call", strike=230.0, n=n, m=m, barrier_type="down-and-out",
              lower_barrier=210.0, monitor_dates=WEEKDAYS)
    p = trade(eng, **kw)
    assert p.carry_rate_nacc == p.discount_rate_nacc
    V = np.array(p._solve_grid())
    ref, steps = compose(trade(eng, **kw), eng, it=False, floor=False)
    assert len(steps) == 23
    err = float(np.max(np.abs(V - ref)))
    print(f"american vs european chain {n}x{m}: max abs diff {err:.3e}")
    assert err <= 1e-12 * max(1.0, float(np.max(np.abs(ref))))


# --------------------------------------------------------------- lower bound
FOUR = [
    ("put_down_out", dict(option_type="put", barrier_type="down-and-out", lower_barrier=200.0)),
    ("put_up_out", dict(option_type="put", barrier_type="up-and-out", upper_barrier=250.0)),
    ("call_up_out", dict(option_type="call", barrier_type="up-and-out", upper_barrier=250.0)),
    ("put_double_out", dict(option_type="put", barrier_type="double-out", lower_barrier=200.0,
                            upper_barrier=250.0)),
]


@pytest.mark.parametrize("name,kw", FOUR, ids=[n for n, _ in FOUR])
def test_american_knockout_dominates_european_knockout(name, kw):
    eng = oracle_engine()
    p = trade(eng, n=128, m=96, monitor_dates=FIVE, **kw)
    V = np.array(p._solve_grid())
    # the hand-composed American chain is the pricer's, bit for bit
    am, steps = compose(trade(eng, n=128, m=96, monitor_dates=FIVE, **kw), eng, it=True,
                        floor=True)
    assert steps == [28, 22, 15, 19, 12]
    assert np.array_equal(V, am)
    eu, _ = compose(trade(eng, n=128, m=96, monitor_dates=FIVE, **kw), eng, it=False,
                    floor=False)
    diff = V - eu
    print(f"{name}: min(V_am - V_eu) = {diff.min():.3e}, max = {diff.max():.3e}")
    assert diff.min() >= 0.0
    assert diff.max() > 0.0 or kw["option_type"] == "call"


# ---------------------------------------------------- floor and convergence
def test_exercise_floor_converges_in_time_and_stays_below_vanilla():
    """Down-and-out put K 220, H 200, 400 nodes, weekday monitoring.  With the
    floor the 400-step price is within 3.1e-4 of the 6 400-step one; with the
    plain projection (V <- rebate) the next IT step builds a multiplier of
    payoff/dt on the knocked nodes and the gap is 4.4e-2 (CPU oracle)."""
    kw = dict(barrier_type="down-and-out", lower_barrier=200.0, monitor_dates=WEEKDAYS)
    p400 = trade(oracle_engine(), m=400, **kw).price_log()
    p6400 = trade(oracle_engine(), m=6400, **kw).price_log()
    van = vanilla(oracle_engine(), m=400).price_log()
    print(f"p400 {p400:.6f} p6400 {p6400:.6f} vanilla400 {van:.6f}")
    assert abs(p400 - p6400) <= 2e-3
    assert p400 <= van
    # the plain projection, marched by hand on the same segments, fails it
    eng = oracle_engine()
    q = trade(eng, m=400, **kw)
    bare, _ = compose(q, eng, it=True, floor=False)
    assert abs(q._interp_price(bare) - p6400) > 2e-3


def test_far_barrier_is_the_vanilla_price_up_to_segmentation():
    """lower_barrier = 1e-3 knocks nothing; the 23 segments still restart
    lambda (and Rannacher), so the price is close, not bitwise (2.0e-4)."""
    far = trade(oracle_engine(), barrier_type="down-and-out", lower_barrier=1e-3,
                monitor_dates=WEEKDAYS).price_log()
    van = vanilla(oracle_engine()).price_log()
    print(f"far barrier {far:.6f} vanilla {van:.6f}")
    assert abs(far - van) <= 5e-4


# --------------------------------------------------------------- event order
@pytest.mark.parametrize("opt", ["put", "call"])
def test_dividend_on_a_monitoring_date_knocks_out_first(opt):
    """Backward in time the knock-out is applied first (monitoring sees the
    ex-dividend spot), then the dividend jump: two events, no steps between."""
    d = VAL + dt.timedelta(days=10)
    kw = dict(option_type=opt, n=128, m=96, divs=[(d, 2.5)], barrier_type="double-out",
              lower_barrier=205.0, upper_barrier=250.0, rebate_amount=1.5,
              monitor_dates=[VAL + dt.timedelta(days=4), d, VAL + dt.timedelta(days=22)])
    eng = oracle_engine()
    p = trade(eng, **kw)
    p._build_log_grid()
    events, pts, steps, restart = p._job_events(96)
    assert [[e[0] for e in evs] for evs in events] == [["ko"], ["ko", "div"], ["ko"]]
    assert len(steps) == 4 and sum(steps) == 96
    assert restart == [True] * 4
    V = np.array(trade(eng, **kw)._solve_grid())
    ref, _ = compose(trade(eng, **kw), eng, it=True, floor=True)
    assert np.array_equal(V, ref)
    # and the other order is a different number
    q = trade(eng, **kw)
    inner = q._job_events

    def swapped(n_time):
        ev, *rest = inner(n_time)
        return ([e[::-1] for e in ev], *rest)
    q._job_events = swapped
    assert not np.array_equal(np.array(q._solve_grid()), V)


def test_restart_on_monitoring_false_keeps_the_reference_rule():
    kw = dict(n=128, m=96, barrier_type="down-and-out", lower_barrier=200.0, monitor_dates=FIVE)
    for opt, want in (("put", [True, False, False, False, False]), ("call", [True] * 5)):
        p = trade(oracle_engine(), option_type=opt, restart_on_monitoring=False, **kw)
        p._build_log_grid()
        assert p._job_events(96)[3] == want
        q = trade(oracle_engine(), option_type=opt, **kw)
        q._build_log_grid()
        assert q._job_events(96)[3] == [True] * 5


# ------------------------------------------------------ maturity monitoring
def test_monitoring_at_maturity_projects_the_payoff():
    kw = dict(n=128, m=96, barrier_type="double-out", lower_barrier=200.0, upper_barrier=250.0,
              rebate_amount=3.0, rebate_at_hit=True)
    p = trade(oracle_engine(), monitor_dates=[MAT], **kw)
    p._build_log_grid()
    s, pay = np.array(p.s_nodes), p._payoff_array()
    knocked = (s <= 200.0) | (s >= 250.0)
    assert knocked.any() and not knocked.all()
    want = np.where(knocked, np.maximum(pay, 3.0), pay)
    assert np.array_equal(p._initial_vector(), want)
    events, pts, steps, _ = p._job_events(96)
    assert events == [] and steps == [96]  # one segment: maturity is no cut
    V = np.array(p._solve_grid())
    ref = oracle_engine().run([p._segment_solve(want, 0.0, p.time_to_expiry, 96, True)])[0]
    assert np.array_equal(V, ref)
    q = trade(oracle_engine(), monitor_dates=[], **kw)
    assert not np.array_equal(np.array(q._solve_grid()), V)


def test_discounted_rebate_is_the_barrier_pricers():
    from finite_difference_amd.barrier import rebate_value
    import math
    p = trade(oracle_engine(), n=128, m=96, barrier_type="down-and-out", lower_barrier=200.0,
              rebate_amount=2.0, monitor_dates=FIVE)
    assert p._rebate(0.05) == 2.0 * math.exp(-p.carry_rate_nacc * 0.05)
    assert p._rebate(0.05) == rebate_value(2.0, False, p.carry_rate_nacc, 0.05)
    p.rebate_at_hit = True
    assert p._rebate(0.05) == 2.0


# -------------------------------------------------------------------- errors
def test_constructor_errors_and_already_hit():
    eng = oracle_engine()
    for bt in ("up-and-in", "down-and-in", "double-in"):
        with pytest.raises(ValueError):
            trade(eng, barrier_type=bt, lower_barrier=200.0, upper_barrier=250.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="down-and-out", upper_barrier=250.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="up-and-out", lower_barrier=200.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="double-out", lower_barrier=200.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="sideways")
    p = trade(eng, barrier_type="down-and-out", lower_barrier=200.0, monitor_dates=WEEKDAYS,
              rebate_amount=1.25, already_hit=True)
    assert p.price_log() == p.price_log2() == 1.25
    assert p.greeks_log2() == {"price": 1.25, "delta": 0.0, "gamma": 0.0, "vega": 0.0,
                               "theta": 0.0}
    prefetch_many([p])
    assert eng.launches == 0


# ------------------------------------------------------------ mixed batches
def test_mixed_prefetch_leaves_vanilla_results_unchanged_and_shares_launches():
    div_cases = [c for c in CASES if c["inputs"]["divs"]]
    nodiv = [c for c in CASES if not c["inputs"]["divs"]]
    bar = dict(barrier_type="down-and-out", lower_barrier=160.0, monitor_dates=FIVE)
    alone = oracle_engine()
    va = [AmericanFDMPricer(**golden_kw(c, alone)) for c in CASES]
    prefetch_many(va)
    eng = oracle_engine()
    vm = [AmericanFDMPricer(**golden_kw(c, eng)) for c in CASES]
    bm = [AmericanBarrierFDMPricer(**golden_kw(c, eng), **bar) for c in nodiv[:1] + div_cases[:1]]
    prefetch_many(vm[:2] + bm + vm[2:])
    used = eng.launches
    for a, m, c in zip(va, vm, CASES):
        assert m.price_log2() == a.price_log2() == c["price_log2"]
        assert m.greeks_log2() == a.greeks_log2() == c["greeks_log2"]
    solo = oracle_engine()
    for c in nodiv[:1] + div_cases[:1]:
        q = AmericanBarrierFDMPricer(**golden_kw(c, solo), **bar)
        prefetch_many([q])
        b = bm.pop(0)
        assert b.price_log2() == q.price_log2()
        assert b.greeks_log2() == q.greeks_log2()
    assert eng.launches == used  # everything came from the one prefetch

    # two barrier trades with the same dates march in the same launches
    two = oracle_engine()
    c = nodiv[0]
    ps = [AmericanBarrierFDMPricer(**golden_kw(c, two), **bar) for _ in range(2)]
    ps[1]._reset_trade(ps[1].spot, ps[1].strike * 1.01, ps[1].sigma)
    prefetch_many(ps)
    one = oracle_engine()
    prefetch_many([AmericanBarrierFDMPricer(**golden_kw(c, one), **bar)])
    assert two.launches == one.launches and two.solves == 2 * one.solves
