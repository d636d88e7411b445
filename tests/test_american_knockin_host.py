"""AmericanKnockInFDMPricer host logic on the CPU oracle: an American option
with a discretely monitored knock-in is two coupled chains over the segments
of the knock-out march -- W, the vanilla American Ikonen-Toivanen march, and
U, plain Crank-Nicolson, with U <- W on the knocked nodes at each monitoring
date (american_knockin.py).  There is no reference implementation of this
product; the checks are hand-composed chains, in/out parity in the European
limit, bounds, convergence in time and identities with the vanilla pricer
("American knock-in")."""
import datetime as dt
import math

import numpy as np
import pytest

from backends import oracle_engine
from conftest import load_golden
from finite_difference_amd import (AmericanBarrierFDMPricer, AmericanKnockInFDMPricer, capi,
                                   market)
from finite_difference_amd.american import AmericanFDMPricer, prefetch_many
from finite_difference_amd.engine import FORM_SUM, Boundary

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
CASES = load_golden("american_cases.json")["cases"]
WEEKDAYS = [VAL + dt.timedelta(days=k) for k in range(32)
            if (VAL + dt.timedelta(days=k)).weekday() < 5]
FIVE = [VAL + dt.timedelta(days=k) for k in (0, 4, 10, 15, 22, 31)]  # valuation: skipped
CURVE = market.iso_curve(market.create_rate_df(0.073086))
OUT = {"up-and-in": "up-and-out", "down-and-in": "down-and-out", "double-in": "double-out"}


def golden_kw(case, engine):
    inp = case["inputs"]
    curve = market.iso_curve(market.create_rate_df(inp["naca"]))
    divs = [(dt.date.fromisoformat(d), a) for d, a in inp["divs"]]
    return dict(spot=inp["spot"], strike=inp["strike"], valuation_date=VAL, maturity_date=MAT,
                sigma=inp["sigma"], option_type=inp["option_type"], discount_curve=curve,
                forward_curve=curve, dividend_schedule=divs, num_space_nodes=inp["N"],
                num_time_steps=inp["M"], rannacher_steps=2, engine=engine)


def trade(engine, cls=AmericanKnockInFDMPricer, option_type="put", strike=220.0, n=400, m=400,
          divs=None, **barrier):
    """The trade of the design table: spot 229.74, sigma 0.26, flat NACA
    0.073086, one month."""
    return cls(spot=229.74, strike=strike, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
               option_type=option_type, discount_curve=CURVE, forward_curve=CURVE,
               dividend_schedule=divs, num_space_nodes=n, num_time_steps=m, rannacher_steps=2,
               engine=engine, **barrier)


def knocked_nodes(p):
    """The knocked nodes from the barrier levels and the grid, without the
    pricer's thresholds."""
    s = np.array(p.s_nodes)
    k = np.zeros(s.shape[0], dtype=bool)
    if p.barrier_type in ("down-and-in", "double-in"):
        k |= s <= p.lower_barrier
    if p.barrier_type in ("up-and-in", "double-in"):
        k |= s >= p.upper_barrier
    return k


def u_boundaries(p, knocked):
    """Vanilla boundary on a side whose edge node is knocked, else the rebate
    discounted at the discount rate."""
    lower, upper = p._boundaries()
    R = p.rebate_amount
    reb = Boundary(FORM_SUM, R, -p.discount_rate_nacc, 0.0, 0.0) if R != 0.0 else Boundary()
    return (lower if knocked[0] else reb), (upper if knocked[-1] else reb)


def cn(p, v, a, b, ns, restart, lower, upper):
    """One plain Crank-Nicolson segment with p's coefficients."""
    s = p._segment_solve(v, a, b, ns, restart)
    s.it, s.payoff, s.lower, s.upper = False, None, lower, upper
    return s


def compose_ki(p, engine, w_it=True, floor_u=False, n_time=None):
    """W and U of p's own segments marched by hand, one engine.run per chain
    and segment, every event applied here in NumPy: the knock-in first, then
    the dividend jump of both chains (U's without the call's exercise floor,
    unless floor_u).  With w_it=False W is plain Crank-Nicolson (the European
    limit); either way it keeps the reference's Rannacher rule (the first
    segment, and every segment of a call).  Returns (U, W, steps)."""
    p._build_log_grid()
    events, pts, steps, restart = p._job_events(n_time or p.num_time_steps)
    pay = p._payoff_array()
    knocked = knocked_nodes(p)
    call = p.option_type == "call"
    lower, upper = u_boundaries(p, knocked)
    w = pay
    u = np.full(pay.shape[0], p.rebate_amount)
    if p._monitor_taus()[1]:
        u = np.where(knocked, pay, u)
    for seg, ns in enumerate(steps):
        a, b = pts[seg], pts[seg + 1]
        sw = p._segment_solve(w, a, b, ns, seg == 0 or call)
        if not w_it:
            sw.it, sw.payoff = False, None
        w = engine.run([sw])[0]
        u = engine.run([cn(p, u, a, b, ns, restart[seg], lower, upper)])[0]
        if seg < len(events):
            for e in events[seg]:
                if e[0] == "ki":
                    u = np.where(knocked, w, u)
                else:
                    k = p._strike_for_pde() if call else -1.0
                    u = capi.dividend_jump(p.s_nodes, u, e[1], k if floor_u else -1.0)
                    w = capi.dividend_jump(p.s_nodes, w, e[1], k)
    return np.asarray(u), np.asarray(w), steps


def compose_eu_ko(p, engine):
    """The European knock-out chain that complements p: plain Crank-Nicolson
    over p's segments with p's restart flags, projection to 0 on the knocked
    nodes, zero boundary on a knocked side and the vanilla one on the other."""
    p._build_log_grid()
    events, pts, steps, restart = p._job_events(p.num_time_steps)
    knocked = knocked_nodes(p)
    lower, upper = p._boundaries()
    lower = Boundary() if knocked[0] else lower
    upper = Boundary() if knocked[-1] else upper
    v = p._payoff_array()
    if p._monitor_taus()[1]:
        v = np.where(knocked, 0.0, v)
    for seg, ns in enumerate(steps):
        v = engine.run([cn(p, v, pts[seg], pts[seg + 1], ns, restart[seg], lower, upper)])[0]
        if seg < len(events):
            assert [e[0] for e in events[seg]] == ["ki"]
            v = np.where(knocked, 0.0, v)
    return np.asarray(v)


FOUR = [
    ("put_down_in", dict(option_type="put", barrier_type="down-and-in", lower_barrier=200.0)),
    ("put_up_in", dict(option_type="put", barrier_type="up-and-in", upper_barrier=250.0)),
    ("call_up_in", dict(option_type="call", barrier_type="up-and-in", upper_barrier=250.0)),
    ("put_double_in", dict(option_type="put", barrier_type="double-in", lower_barrier=200.0,
                           upper_barrier=250.0)),
]
PUTS = [t for t in FOUR if t[1]["option_type"] == "put"]


# ------------------------------------------------------- 1. hand-composed chain
@pytest.mark.parametrize("name,kw", FOUR, ids=[n for n, _ in FOUR])
def test_pricer_is_the_hand_composed_pair_of_chains_bitwise(name, kw):
    eng = oracle_engine()
    V = np.array(trade(eng, n=128, m=96, monitor_dates=FIVE, **kw)._solve_grid())
    q = trade(eng, n=128, m=96, monitor_dates=FIVE, **kw)
    U, W, steps = compose_ki(q, eng)
    assert steps == [28, 22, 15, 19, 12]
    k = knocked_nodes(q)
    assert k.any() and not k.all()
    assert np.array_equal(V, U)
    assert not np.array_equal(V, W)


# ------------------------------------------------ 2. parity, European limit
CALLS = [
    ("call_up_in", dict(option_type="call", strike=220.0, barrier_type="up-and-in",
                        upper_barrier=250.0)),
    ("call_down_in", dict(option_type="call", strike=230.0, barrier_type="down-and-in",
                          lower_barrier=210.0)),
]


@pytest.mark.parametrize("n,m", [(400, 400), (128, 96)])
@pytest.mark.parametrize("name,kw", CALLS, ids=[n for n, _ in CALLS])
def test_in_out_parity_of_calls_that_are_never_exercised(name, kw, n, m):
    """Carry = discount, no dividends: early exercise never binds, so U of the
    American pricer is the European knock-in, and knock-in + knock-out =
    vanilla chain by chain when all three restart alike."""
    eng = oracle_engine()
    p = trade(eng, n=n, m=m, monitor_dates=WEEKDAYS, **kw)
    assert p.carry_rate_nacc == p.discount_rate_nacc
    U = np.array(p._solve_grid())
    q = trade(eng, n=n, m=m, monitor_dates=WEEKDAYS, **kw)
    U_eu, W_eu, steps = compose_ki(q, eng, w_it=False)
    assert len(steps) == 23 and q._job_events(m)[3] == [True] * 23
    KO = compose_eu_ko(q, eng)
    scale = max(1.0, float(np.max(np.abs(W_eu))))
    res = float(np.max(np.abs(U + KO - W_eu)))
    res_eu = float(np.max(np.abs(U_eu + KO - W_eu)))
    gap = float(np.max(np.abs(U - U_eu)))
    print(f"{name} {n}x{m}: max|U+KO-W| {res:.3e} (European W: {res_eu:.3e}), "
          f"max|U_am - U_eu| {gap:.3e}, max|W| {scale:.1f}")
    assert res <= 1e-11 * scale and res_eu <= 1e-11 * scale
    assert gap <= 1e-12 * max(1.0, float(np.max(np.abs(U_eu))))


@pytest.mark.parametrize("n,m", [(400, 400), (128, 96)])
@pytest.mark.parametrize("name,kw", PUTS[:2], ids=[n for n, _ in PUTS[:2]])
def test_in_out_parity_of_european_puts_under_the_reference_restart_rule(name, kw, n, m):
    """restart_on_monitoring=False: U, the knock-out chain and the vanilla
    chain all restart in the first segment only, and parity is exact again
    (with different theta schedules the residual is 1e-4 .. 4e-3)."""
    eng = oracle_engine()
    q = trade(eng, n=n, m=m, monitor_dates=WEEKDAYS, restart_on_monitoring=False, **kw)
    U_eu, W_eu, steps = compose_ki(q, eng, w_it=False)
    assert q._job_events(m)[3] == [True] + [False] * 22
    KO = compose_eu_ko(q, eng)
    scale = max(1.0, float(np.max(np.abs(W_eu))))
    res = float(np.max(np.abs(U_eu + KO - W_eu)))
    print(f"{name} {n}x{m}: max|U+KO-W| {res:.3e}, max|W| {scale:.1f}")
    assert res <= 1e-11 * scale


# ------------------------------------------------------------------ 3. bounds
@pytest.mark.parametrize("n,m,dates", [(128, 96, FIVE), (400, 400, WEEKDAYS)],
                         ids=["128x96_five", "400x400_weekdays"])
@pytest.mark.parametrize("name,kw", PUTS, ids=[n for n, _ in PUTS])
def test_bounds_of_the_american_knock_in_put(name, kw, n, m, dates):
    eng = oracle_engine()
    p = trade(eng, n=n, m=m, monitor_dates=dates, **kw)
    U = np.array(p._solve_grid())
    q = trade(eng, n=n, m=m, monitor_dates=dates, **kw)
    U_eu, _, _ = compose_ki(q, eng, w_it=False)
    _, W, _ = compose_ki(q, eng)
    diff = U - U_eu
    price_ki, price_cut = p.price_log(), q._interp_price(W)
    out = {k: v for k, v in kw.items() if k != "barrier_type"}
    price_ko = trade(eng, cls=AmericanBarrierFDMPricer, n=n, m=m, monitor_dates=dates,
                     barrier_type=OUT[kw["barrier_type"]], **out).price_log()
    van = trade(eng, cls=AmericanFDMPricer, n=n, m=m).price_log()
    print(f"{name} {n}x{m}: min(U_am - U_eu) {diff.min():.3e} max {diff.max():.3e}; "
          f"KI {price_ki:.6f} cut vanilla {price_cut:.6f} (margin {price_cut - price_ki:.3e}); "
          f"KI + KO - vanilla {price_ki + price_ko - van:.3e} "
          f"(cut: {price_ki + price_ko - price_cut:.3e})")
    assert diff.min() >= 0.0
    assert diff.max() > 0.0
    assert price_ki <= price_cut
    assert price_ki + price_ko >= van - 1e-3
    assert price_ki + price_ko >= price_cut - 1e-3


# ------------------------------------------------------------ 4. convergence
def test_knock_in_put_converges_in_time_and_stays_below_vanilla():
    """Down-and-in put K 220, H 200, 400 nodes, weekday monitoring (CPU
    oracle, NumPy grid: 1.072229 at 400 steps, 1.072333 at 6 400)."""
    kw = dict(barrier_type="down-and-in", lower_barrier=200.0, monitor_dates=WEEKDAYS)
    p400 = trade(oracle_engine(), m=400, **kw).price_log()
    p6400 = trade(oracle_engine(), m=6400, **kw).price_log()
    van = trade(oracle_engine(), cls=AmericanFDMPricer, m=400).price_log()
    print(f"p400 {p400:.6f} p6400 {p6400:.6f} vanilla400 {van:.6f}")
    assert abs(p400 - p6400) <= 5e-4
    assert p400 <= van


# ------------------------------------------- 5. unreachable barrier, rebate
def test_unreachable_barrier_is_the_discounted_rebate():
    kw = dict(n=128, m=96, barrier_type="down-and-in", lower_barrier=1e-3, monitor_dates=FIVE)
    p = trade(oracle_engine(), **kw)
    V = np.array(p._solve_grid())
    assert not knocked_nodes(p).any()
    assert np.all(V == 0.0)
    q = trade(oracle_engine(), rebate_amount=2.0, **kw)
    V = np.array(q._solve_grid())
    want = 2.0 * math.exp(-q.discount_rate_nacc * q.time_to_expiry)
    err = float(np.max(np.abs(V - want)))
    print(f"rebate 2.0: r {q.discount_rate_nacc:.6f}, max|V - R exp(-rT)| {err:.3e}")
    assert err <= 1e-6 * 2.0


# ------------------------------------------------------ 6. everything knocked
def test_everything_knocked_is_the_european_continuation_of_w():
    d = VAL + dt.timedelta(days=15)
    eng = oracle_engine()
    kw = dict(n=128, m=96, barrier_type="down-and-in", lower_barrier=1e6, monitor_dates=[d])
    p = trade(eng, **kw)
    V = np.array(p._solve_grid())
    assert knocked_nodes(p).all()
    events, pts, steps, restart = p._job_events(96)
    assert [[e[0] for e in evs] for evs in events] == [["ki"]] and restart == [True, True]
    Wd = eng.run([p._segment_solve(p._payoff_array(), pts[0], pts[1], steps[0], True)])[0]
    ref = eng.run([cn(p, Wd, pts[1], pts[2], steps[1], True, *p._boundaries())])[0]
    assert np.array_equal(V, ref)


def test_monitoring_at_maturity_only_starts_from_the_payoff_on_knocked_nodes():
    kw = dict(n=128, m=96, barrier_type="double-in", lower_barrier=200.0, upper_barrier=250.0,
              rebate_amount=3.0)
    p = trade(oracle_engine(), monitor_dates=[MAT], **kw)
    p._build_log_grid()
    pay, knocked = p._payoff_array(), knocked_nodes(p)
    assert knocked.any() and not knocked.all() and knocked[0] and knocked[-1]
    want = np.where(knocked, pay, 3.0)
    assert np.array_equal(p._initial_vector(), want)
    events, pts, steps, _ = p._job_events(96)
    assert events == [] and steps == [96]  # one segment: maturity is no cut
    eng = oracle_engine()
    p.engine = eng
    V = np.array(p._solve_grid())
    assert eng.solves == 1  # no monitoring time reads W: it is not marched
    ref = oracle_engine().run([cn(p, want, 0.0, p.time_to_expiry, 96, True, *p._boundaries())])[0]
    assert np.array_equal(V, ref)


# -------------------------------------------------------------- 7. event order
@pytest.mark.parametrize("opt", ["put", "call"])
def test_dividend_on_a_monitoring_date_knocks_in_first(opt):
    """Backward in time: the knock-in (monitoring sees the ex-dividend spot),
    then the jump of both chains, U's without the call's exercise floor."""
    d = VAL + dt.timedelta(days=10)
    kw = dict(option_type=opt, n=128, m=96, divs=[(d, 2.5)], barrier_type="double-in",
              lower_barrier=205.0, upper_barrier=250.0, rebate_amount=1.5,
              monitor_dates=[VAL + dt.timedelta(days=4), d, VAL + dt.timedelta(days=22)])
    eng = oracle_engine()
    p = trade(eng, **kw)
    p._build_log_grid()
    events, pts, steps, restart = p._job_events(96)
    assert [[e[0] for e in evs] for evs in events] == [["ki"], ["ki", "div"], ["ki"]]
    assert len(steps) == 4 and sum(steps) == 96 and restart == [True] * 4
    V = np.array(trade(eng, **kw)._solve_grid())
    ref, _, _ = compose_ki(trade(eng, **kw), eng)
    assert np.array_equal(V, ref)
    floored, _, _ = compose_ki(trade(eng, **kw), eng, floor_u=True)
    if opt == "call":
        assert not np.array_equal(floored, V)
    else:
        assert np.array_equal(floored, V)
    # and the other order is a different number
    q = trade(eng, **kw)
    inner = q._job_events

    def swapped(n_time):
        ev, *rest = inner(n_time)
        return ([e[::-1] for e in ev], *rest)
    q._job_events = swapped
    assert not np.array_equal(np.array(q._solve_grid()), V)


def test_restart_rule_of_the_u_chain():
    d = VAL + dt.timedelta(days=12)
    kw = dict(n=128, m=96, barrier_type="down-and-in", lower_barrier=200.0, monitor_dates=FIVE,
              divs=[(d, 2.5)])
    # segments end at: day 22, 15, 12 (dividend), 10, 4
    for opt, flag, want in (("put", True, [True, True, True, False, True, True]),
                            ("put", False, [True] + [False] * 5),
                            ("call", False, [True, False, False, True, False, False])):
        p = trade(oracle_engine(), option_type=opt, restart_on_monitoring=flag, **kw)
        p._build_log_grid()
        events, _, _, restart = p._job_events(96)
        assert [[e[0] for e in evs] for evs in events] == [["ki"], ["ki"], ["div"], ["ki"], ["ki"]]
        assert restart == want, (opt, flag)
        job = p._make_job(("k",), p.sigma, 96)
        assert job["w_restart"] == [s == 0 or opt == "call" for s in range(6)]
        assert job["w_last"] == 4


# ---------------------------------------------------- 8. identities and errors
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("barrier", [
    dict(barrier_type="none", lower_barrier=150.0, monitor_dates=WEEKDAYS),
    dict(barrier_type="down-and-in", lower_barrier=150.0, monitor_dates=WEEKDAYS,
         already_in=True),
], ids=["none", "already_in"])
def test_without_a_barrier_or_already_in_it_is_the_vanilla_pricer(case, barrier):
    b = AmericanKnockInFDMPricer(**golden_kw(case, oracle_engine()), **barrier)
    assert b._solve_grid() == case["V"]
    assert b.price_log2() == case["price_log2"]
    assert b.greeks_log2() == case["greeks_log2"]


def test_constructor_errors_and_the_option_that_cannot_knock_in():
    eng = oracle_engine()
    for bt in ("up-and-out", "down-and-out", "double-out"):
        with pytest.raises(ValueError, match="AmericanBarrierFDMPricer"):
            trade(eng, barrier_type=bt, lower_barrier=200.0, upper_barrier=250.0)
    with pytest.raises(ValueError, match="maturity"):
        trade(eng, barrier_type="down-and-in", lower_barrier=200.0, rebate_at_hit=True)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="down-and-in", upper_barrier=250.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="up-and-in", lower_barrier=200.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="double-in", lower_barrier=200.0)
    with pytest.raises(ValueError):
        trade(eng, barrier_type="sideways")
    for bt in ("up-and-in", "down-and-in", "double-in"):  # the knock-out class still refuses
        with pytest.raises(ValueError):
            trade(eng, cls=AmericanBarrierFDMPricer, barrier_type=bt, lower_barrier=200.0,
                  upper_barrier=250.0)
    for dates in ([], [VAL, VAL - dt.timedelta(days=3), MAT + dt.timedelta(days=1)]):
        p = trade(eng, barrier_type="down-and-in", lower_barrier=200.0, monitor_dates=dates,
                  rebate_amount=1.25)
        r, T = p.discount_rate_nacc, p.time_to_expiry
        want = 1.25 * math.exp(-r * T)
        assert p.price_log() == p.price_log2() == want
        assert p.greeks_log2() == {"price": want, "delta": 0.0, "gamma": 0.0, "vega": 0.0,
                                   "theta": r * want}
        prefetch_many([p])
    assert eng.launches == 0


def test_state_keys_of_the_kinds_do_not_collide():
    eng = oracle_engine()
    kw = dict(lower_barrier=200.0, monitor_dates=FIVE)
    a = trade(eng, barrier_type="down-and-in", **kw)
    b = trade(eng, barrier_type="down-and-in", already_in=True, **kw)
    c = trade(eng, cls=AmericanBarrierFDMPricer, barrier_type="down-and-out", **kw)
    keys = {p._state_key(0.26, 400) for p in (a, b, c)}
    assert len(keys) == 3


# ------------------------------------------------------------ 9. mixed batches
def test_mixed_prefetch_leaves_other_kinds_unchanged_and_shares_launches():
    div_cases = [c for c in CASES if c["inputs"]["divs"]]
    nodiv = [c for c in CASES if not c["inputs"]["divs"]]
    picks = nodiv[:1] + div_cases[:1]
    out = dict(barrier_type="down-and-out", lower_barrier=160.0, monitor_dates=FIVE)
    kin = dict(barrier_type="down-and-in", lower_barrier=160.0, monitor_dates=FIVE)
    alone = oracle_engine()
    va = [AmericanFDMPricer(**golden_kw(c, alone)) for c in CASES]
    oa = [AmericanBarrierFDMPricer(**golden_kw(c, alone), **out) for c in picks]
    prefetch_many(va + oa)
    eng = oracle_engine()
    vm = [AmericanFDMPricer(**golden_kw(c, eng)) for c in CASES]
    om = [AmericanBarrierFDMPricer(**golden_kw(c, eng), **out) for c in picks]
    km = [AmericanKnockInFDMPricer(**golden_kw(c, eng), **kin) for c in picks]
    prefetch_many(vm[:2] + km[:1] + om + km[1:] + vm[2:])
    used = eng.launches
    for a, m, c in zip(va, vm, CASES):
        assert m.price_log2() == a.price_log2() == c["price_log2"]
        assert m.greeks_log2() == a.greeks_log2() == c["greeks_log2"]
    for a, m in zip(oa, om):
        assert m.price_log2() == a.price_log2()
        assert m.greeks_log2() == a.greeks_log2()
    solo = oracle_engine()
    for c, k in zip(picks, km):
        q = AmericanKnockInFDMPricer(**golden_kw(c, solo), **kin)
        prefetch_many([q])
        assert k.price_log2() == q.price_log2()
        assert k.greeks_log2() == q.greeks_log2()
    assert eng.launches == used  # everything came from the one prefetch

    # two knock-in trades with the same dates march in the same launches
    two = oracle_engine()
    c = nodiv[0]
    ps = [AmericanKnockInFDMPricer(**golden_kw(c, two), **kin) for _ in range(2)]
    ps[1]._reset_trade(ps[1].spot, ps[1].strike * 1.01, ps[1].sigma)
    prefetch_many(ps)
    one = oracle_engine()
    prefetch_many([AmericanKnockInFDMPricer(**golden_kw(c, one), **kin)])
    assert two.launches == one.launches and two.solves == 2 * one.solves
