"""BermudanFDMPricer host logic on the CPU oracle: plain Crank-Nicolson
segments cut at the exercise, monitoring and dividend dates, with
V <- max(V, payoff) at the exercise dates (bermudan.py).  There is no
reference implementation of this product; the checks are hand-composed segment
chains, the design table's prices ("Bermudan"), the strict ordering
European < weekly < weekdays < American, and identities."""
import datetime as dt

import numpy as np
import pytest

from backends import oracle_engine
from finite_difference_amd import AmericanBarrierFDMPricer, BermudanFDMPricer, capi, market
from finite_difference_amd.american import AmericanFDMPricer

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
CURVE = market.iso_curve(market.create_rate_df(0.073086))
WEEKLY = [VAL + dt.timedelta(days=k) for k in (7, 14, 21, 28)]
WEEKDAYS = [VAL + dt.timedelta(days=k) for k in range(1, 31)
            if (VAL + dt.timedelta(days=k)).weekday() < 5]  # the 22 inside the life
DIV_DAY = WEEKLY[1]

# the three trades of the chain tests (also marched on the device in
# test_bermudan_device_loop.py and test_gpu_bermudan.py)
CHAIN_TRADES = [
    ("put_weekly", dict(option_type="put", exercise_dates=WEEKLY)),
    ("put_up_out_three_kinds", dict(option_type="put", exercise_dates=WEEKLY,
                                    barrier_type="up-and-out", upper_barrier=240.0,
                                    rebate_amount=1.5, rebate_at_hit=True,
                                    monitor_dates=WEEKDAYS + [MAT])),
    ("call_div_on_exercise", dict(option_type="call", strike=230.0, exercise_dates=WEEKLY,
                                  dividend_schedule=[(DIV_DAY, 2.5)])),
]


def trade(engine, cls=BermudanFDMPricer, option_type="put", strike=220.0, n=400, m=400, **kw):
    """The trade of the design table: spot 229.74, sigma 0.26, flat NACA
    0.073086, one month."""
    return cls(spot=229.74, strike=strike, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
               option_type=option_type, discount_curve=CURVE, forward_curve=CURVE,
               num_space_nodes=n, num_time_steps=m, rannacher_steps=2, engine=engine, **kw)


def compose(p, engine, exercise=True):
    """The Bermudan chain marched by hand from the rules of the module's
    docstring, not from the pricer's event list: one engine.run per segment
    (it=False, no payoff), the events in NumPy.  exercise=False leaves the
    exercise events out (the same segments, the same restarts).  Returns the
    vector, the step counts and the (lo, hi, count) of every exercise date in
    the order of the march."""
    p._build_log_grid()
    T, n_time = p.time_to_expiry, p.num_time_steps
    tau_of = lambda d: T - p._year_fraction(VAL, d)  # noqa: E731
    inside = lambda d: VAL < d and tau_of(d) > 1e-14  # noqa: E731
    ex = {tau_of(d) for d in p.exercise_dates if inside(d)}
    mon = {tau_of(d) for d in p.monitor_dates if inside(d)} if p.barrier_type != "none" else set()
    div = {tau_of(d): cash for d, cash in p.dividend_schedule}
    taus = sorted(ex | mon | set(div))
    pts, steps = p._segments_over(taus, n_time)
    pay = p._payoff_array()
    j = np.arange(pay.shape[0])
    ko_lo, ko_hi = p._ko_thresholds()
    knocked = (j <= ko_lo) | (j >= ko_hi)
    v = pay
    if p.barrier_type != "none" and any(d == MAT for d in p.monitor_dates):
        v = np.where(knocked, np.maximum(pay, p._rebate(0.0)), pay)
    regions = []
    for seg, ns in enumerate(steps):
        prev = taus[seg - 1] if seg else None
        restart = (seg == 0 or (prev in ex and p.restart_on_exercise)
                   or (prev in mon and p.restart_on_monitoring)
                   or (prev in div and p.option_type == "call"))
        s = p._segment_solve(v, pts[seg], pts[seg + 1], ns, restart)
        s.it, s.payoff = False, None
        v = engine.run([s])[0]
        if seg == len(taus):
            break
        tau = taus[seg]
        R = p._rebate(tau)
        if tau in ex:
            k = knocked if tau in mon else np.zeros_like(knocked)
            idx = np.nonzero(~k & (pay > v))[0]
            regions.append((int(idx[0]), int(idx[-1]), len(idx)) if len(idx)
                           else (len(pay), -1, 0))
            if exercise:
                v = np.where(k, np.maximum(pay, R), np.maximum(v, pay))
            elif tau in mon:
                v = np.where(k, np.maximum(pay, R), v)
        elif tau in mon:
            v = np.where(knocked, R, v)
        if tau in div:
            v = capi.dividend_jump(p.s_nodes, v, div[tau], -1.0)
    return np.asarray(v), steps, regions


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("n,m", [(128, 96), (400, 400)])
@pytest.mark.parametrize("name,kw", CHAIN_TRADES, ids=[t[0] for t in CHAIN_TRADES])
def test_solve_grid_is_the_hand_composed_chain_bitwise(name, kw, n, m):
    eng = oracle_engine()
    V = np.array(trade(eng, n=n, m=m, **kw)._solve_grid())
    ref, steps, _ = compose(trade(eng, n=n, m=m, **kw), eng)
    assert len(steps) == (23 if "three_kinds" in name else 5)
    assert np.array_equal(V, ref)


def test_the_three_kinds_of_event_and_their_order():
    p = trade(oracle_engine(), **CHAIN_TRADES[1][1])
    p._build_log_grid()
    events, _, steps, restart = p._job_events(p.num_time_steps)
    kinds = [e[0][0] for e in events]
    assert kinds.count("ex") == 4 and kinds.count("kop") == 18 and all(restart)
    n = len(p.s_nodes)
    assert all(e[0][2] < n for e in events)  # exercise dates are monitored here: knocked nodes
    q = trade(oracle_engine(), **CHAIN_TRADES[0][1])
    q._build_log_grid()
    assert all(e == [("ex", -1, n, 0.0)] for e in q._job_events(400)[0])
    c = trade(oracle_engine(), **CHAIN_TRADES[2][1])
    c._build_log_grid()
    ev = c._job_events(400)[0]
    # tau ascending: the dividend is on the third date from maturity, after the event
    assert [[e[0] for e in evs] for evs in ev] == [["ex"], ["ex"], ["ex", "div"], ["ex"]]
    assert c._jump_chains({}, 2) == [("v", -1.0)]
    r = trade(oracle_engine(), restart_on_exercise=False, **CHAIN_TRADES[0][1])
    r._build_log_grid()
    assert r._job_events(400)[3] == [True, False, False, False, False]


# ------------------------------------------------------------ design table
TABLE = {  # (strike, grid): European, weekly, weekdays, AmericanFDMPricer
    (220.0, 400): (2.657941, 2.679876, 2.687944, 2.692215),
    (220.0, 128): (2.543458, 2.563718, 2.568462, 2.574738),
    (250.0, 400): (19.441744, 19.907126, 19.965820, 19.984923),
    (250.0, 128): (21.694955, 22.249631, 22.322426, 22.342162),
}


@pytest.mark.parametrize("strike,n,m", [(220.0, 400, 400), (220.0, 128, 96), (250.0, 400, 400),
                                        (250.0, 128, 96)])
def test_prices_of_the_table_and_their_strict_ordering(strike, n, m):
    eng = oracle_engine()
    got = (trade(eng, strike=strike, n=n, m=m).price_log(),
           trade(eng, strike=strike, n=n, m=m, exercise_dates=WEEKLY).price_log(),
           trade(eng, strike=strike, n=n, m=m, exercise_dates=WEEKDAYS).price_log(),
           trade(eng, cls=AmericanFDMPricer, strike=strike, n=n, m=m).price_log())
    print(strike, n, m, got)
    assert got[0] < got[1] < got[2] < got[3]
    if n == 400:
        for x, want in zip(got, TABLE[(strike, n)]):
            assert abs(x - want) <= 5e-6


UP_OUT = {  # (strike, rebate): FD Bermudan, FD European KO (no exercise dates)
    (220.0, 0.0): (2.621319, 2.599514), (220.0, 1.5): (3.203957, 3.182155),
    (250.0, 0.0): (19.110481, 16.439254), (250.0, 1.5): (19.161740, 17.047876),
}


@pytest.mark.parametrize("strike,rebate", sorted(UP_OUT))
def test_up_and_out_prices_of_the_table(strike, rebate):
    eng = oracle_engine()
    kw = dict(strike=strike, barrier_type="up-and-out", upper_barrier=240.0,
              rebate_amount=rebate, rebate_at_hit=True, monitor_dates=WEEKLY)
    got = (trade(eng, exercise_dates=WEEKLY, **kw).price_log(), trade(eng, **kw).price_log())
    print(strike, rebate, got)
    for x, want in zip(got, UP_OUT[(strike, rebate)]):
        assert abs(x - want) <= 5e-6


# ------------------------------------------------------------- identities
def test_call_without_dividends_is_never_exercised():
    eng = oracle_engine()
    kw = dict(option_type="call", strike=230.0, exercise_dates=WEEKLY)
    p = trade(eng, **kw)
    V = np.array(p._solve_grid())
    ref, _, _ = compose(trade(eng, **kw), eng, exercise=False)
    assert np.array_equal(V, ref)
    assert abs(p.price_log() - 7.632519364296134) <= 5e-6
    n = len(p.s_nodes)
    b = p.exercise_boundary()
    assert [r[0] for r in b] == WEEKLY
    assert all(r[2] is None and r[3:] == (n, -1, 0) for r in b)


def test_down_and_out_inside_the_exercise_region_changes_nothing():
    eng = oracle_engine()
    plain = trade(eng, exercise_dates=WEEKLY)
    ko = trade(eng, exercise_dates=WEEKLY, barrier_type="down-and-out", lower_barrier=200.0,
               monitor_dates=WEEKLY)
    # the knocked nodes lie inside the exercise region and max(payoff, 0) is the
    # payoff: the same price exactly.  (The vectors differ on the lowest nodes,
    # which the lower Dirichlet value keeps out of the region, far from the spot.)
    assert ko.price_log() == plain.price_log()
    assert abs(ko.price_log() - 2.679876) <= 5e-6
    # weekday monitoring, weekly exercise: the monitoring-only branch matters
    mixed = trade(eng, exercise_dates=WEEKLY, barrier_type="down-and-out", lower_barrier=200.0,
                  monitor_dates=WEEKDAYS)
    assert abs(mixed.price_log() - 2.603855) <= 5e-6


@pytest.mark.parametrize("kw", [
    dict(), dict(exercise_dates=[VAL, VAL - dt.timedelta(days=2), MAT, MAT + dt.timedelta(days=1)]),
    dict(barrier_type="down-and-out", lower_barrier=200.0, monitor_dates=[VAL]),
], ids=["nothing", "dates_outside_or_at_maturity", "barrier_without_dates"])
def test_without_events_it_is_one_uncut_crank_nicolson_march(kw):
    eng = oracle_engine()
    p = trade(eng, n=128, m=96, **kw)
    V = np.array(p._solve_grid())
    q = trade(eng, n=128, m=96)
    q._build_log_grid()
    s = q._segment_solve(q._payoff_array(), 0.0, q.time_to_expiry, 96, True)
    s.it, s.payoff = False, None
    assert np.array_equal(V, eng.run([s])[0])
    assert p.exercise_boundary() == []


# ------------------------------------------------------- exercise boundary
BOUNDARY = {  # weekly, 400 x 400, in tau order 0.0082, 0.0274, 0.0466, 0.0658
    220.0: [(22, 183, 162), (36, 176, 141), (46, 171, 126), (53, 168, 116)],
    250.0: [(21, 200, 180), (35, 194, 160), (44, 189, 146), (51, 185, 135)],
}


@pytest.mark.parametrize("strike", sorted(BOUNDARY))
def test_exercise_boundary_of_the_table(strike):
    eng = oracle_engine()
    p = trade(eng, strike=strike, exercise_dates=WEEKLY)
    b = p.exercise_boundary()
    assert [r[0] for r in b] == WEEKLY  # calendar order: tau descending
    assert [r[3:] for r in b] == BOUNDARY[strike][::-1]
    T = p.time_to_expiry
    assert [round(T - r[1], 4) for r in b] == [0.0658, 0.0466, 0.0274, 0.0082]
    s = p._cache[p._state_key(p.sigma, 400)][1]["s_nodes"]
    assert [r[2] for r in b] == [s[r[4]] for r in b]  # a put: the upper edge
    s_star = [r[2] for r in b]
    assert all(a < c for a, c in zip(s_star, s_star[1:]))  # lower towards valuation
    _, _, regions = compose(trade(eng, strike=strike, exercise_dates=WEEKLY), eng)
    assert regions == BOUNDARY[strike]


def test_exercise_boundary_leaves_out_the_knocked_nodes():
    eng = oracle_engine()
    kw = dict(exercise_dates=WEEKLY, barrier_type="down-and-out", lower_barrier=200.0,
              monitor_dates=WEEKLY)
    p = trade(eng, **kw)
    b = p.exercise_boundary()
    p._build_log_grid()
    ko_lo, _ = p._ko_thresholds()
    assert ko_lo > 53 and all(r[3] == ko_lo + 1 for r in b)
    assert [r[4] for r in b] == [168, 171, 176, 183]
    assert all(r[5] == r[4] - r[3] + 1 for r in b)
    _, _, regions = compose(trade(eng, **kw), eng)
    assert [r[3:] for r in b] == regions[::-1]


# ---------------------------------------------------------------- keywords
@pytest.mark.parametrize("bt", ["up-and-in", "down-and-in", "double-in"])
def test_knock_in_types_raise(bt):
    with pytest.raises(ValueError, match="knock-in"):
        trade(oracle_engine(), exercise_dates=WEEKLY, barrier_type=bt, lower_barrier=200.0,
              upper_barrier=250.0)


def test_already_hit_is_the_parent_class():
    kw = dict(barrier_type="up-and-out", upper_barrier=240.0, rebate_amount=1.5,
              monitor_dates=WEEKLY, already_hit=True)
    p = trade(oracle_engine(), exercise_dates=WEEKLY, **kw)
    q = trade(oracle_engine(), cls=AmericanBarrierFDMPricer, **kw)
    assert p.price_log() == q.price_log() == 1.5
    assert p.price_log2() == q.price_log2() and p.greeks_log2() == q.greeks_log2()
    assert p.exercise_boundary() == []


def test_state_key_tells_the_keywords_apart():
    eng = oracle_engine()
    keys = {trade(eng, **kw)._state_key(0.26, 400) for kw in (
        dict(), dict(exercise_dates=WEEKLY), dict(exercise_dates=WEEKLY[:3]),
        dict(exercise_dates=WEEKLY, restart_on_exercise=False))}
    assert len(keys) == 4
    american = trade(eng, cls=AmericanBarrierFDMPricer)._state_key(0.26, 400)
    assert american not in keys
