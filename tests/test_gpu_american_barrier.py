"""AmericanBarrierFDMPricer on the MI355X: the session path (marches, knock-out
events and dividend jumps chained on the device, payoff uploaded once)
against the host path on the CPU oracle.

Tolerances: those of the American GPU parity (tests/test_gpu_pricers.py):
  value vectors  max|V - V_ref| <= 1e-10 * max(1, max|V_ref|)
  price, delta   |x - ref| <= 1e-10 + 1e-9 |ref|
  gamma, theta, vega  |x - ref| <= 1e-8 * max(1, |ref|)
"""
import datetime as dt

import numpy as np
import pytest

from backends import oracle_engine
from finite_difference_amd import AmericanBarrierFDMPricer, market
from finite_difference_amd.american import AmericanFDMPricer, greeks_many
from finite_difference_amd.engine import Engine, group_solves
from finite_difference_amd.session import Session
from plan_factory import random_solve

pytestmark = pytest.mark.gpu

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
FIVE = [VAL + dt.timedelta(days=k) for k in (0, 4, 10, 15, 22, 31)]
CURVE = market.iso_curve(market.create_rate_df(0.073086))
DIV_DAY = VAL + dt.timedelta(days=10)

TRADES = [
    ("put_down_out", dict(option_type="put", barrier_type="down-and-out", lower_barrier=200.0)),
    ("put_up_out", dict(option_type="put", barrier_type="up-and-out", upper_barrier=250.0)),
    ("call_up_out", dict(option_type="call", barrier_type="up-and-out", upper_barrier=250.0)),
    ("put_double_out", dict(option_type="put", barrier_type="double-out", lower_barrier=200.0,
                            upper_barrier=250.0)),
    ("call_div_on_monitor_130", dict(option_type="call", barrier_type="double-out",
                                     lower_barrier=205.0, upper_barrier=250.0,
                                     rebate_amount=1.5, num_space_nodes=129,
                                     dividend_schedule=[(DIV_DAY, 2.5)])),
]


def make(engine, cls=AmericanBarrierFDMPricer, **kw):
    args = dict(spot=229.74, strike=220.0, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
                discount_curve=CURVE, forward_curve=CURVE, num_space_nodes=128,
                num_time_steps=96, rannacher_steps=2, engine=engine)
    if cls is AmericanBarrierFDMPricer:
        args["monitor_dates"] = FIVE
    args.update(kw)
    return cls(**args)


def close(name, x, ref):
    if name in ("price", "delta"):
        return abs(x - ref) <= 1e-10 + 1e-9 * abs(ref)
    return abs(x - ref) <= 1e-8 * max(1.0, abs(ref))


@pytest.mark.parametrize("name,kw", TRADES, ids=[n for n, _ in TRADES])
def test_session_path_matches_host_path_on_the_oracle(name, kw):
    ref = make(oracle_engine(), **kw)
    V_ref = np.array(ref._solve_grid())
    g_ref, p2_ref = ref.greeks_log2(), ref.price_log2()

    p = make(None, **kw)
    assert p._engine().on_device
    jobs, _ = p._device_jobs([(p.sigma, p.num_time_steps)])
    assert len(jobs[0]["steps"]) == 5 and len(jobs[0]["grid"]["s_nodes"]) == len(V_ref)
    with Session() as S:
        AmericanFDMPricer._march_jobs_device(jobs, p._engine(), S)
        V = S.fetch([jobs[0]["slot"]], len(V_ref))[0]
    err = float(np.max(np.abs(V - V_ref)))
    print(f"[{name}] vector max abs err {err:.3e} (max|V| {np.max(np.abs(V_ref)):.3f})")
    assert err <= 1e-10 * max(1.0, float(np.max(np.abs(V_ref))))

    g, p2 = p.greeks_log2(), p.price_log2()
    print(f"[{name}] abs err", {k: abs(g[k] - g_ref[k]) for k in g_ref}, abs(p2 - p2_ref))
    for k in g_ref:
        assert close(k, g[k], g_ref[k]), (name, k, g[k], g_ref[k])
    assert close("price", p2, p2_ref)


def test_march_ps_is_bitwise_march():
    """fdcn_session_march_ps (payoff in slots: read in place when they are
    consecutive rows of one upload, gathered on the device otherwise) gives
    fdcn_session_march's vectors bit for bit."""
    rng = np.random.default_rng(21)
    solves = ([random_solve(rng, 257, 48, 2, it=True) for _ in range(5)] +
              [random_solve(rng, 130, 30, 0, it=True) for _ in range(3)])
    with Session() as S:
        e = Engine()
        ref = e.march_slots(S, solves)
        want = {g.n_nodes: S.fetch(ref[g.index], g.n_nodes) for g in group_solves(solves)}
        for g in group_solves(solves):
            pay = S.upload(g.payoff)
            got = S.march(g, None, pay)                       # consecutive: in place
            assert np.array_equal(S.fetch(got, g.n_nodes), want[g.n_nodes])
            perm = np.arange(g.B)[::-1]
            back = S.upload(g.payoff[perm])                   # reversed rows: gathered
            got = S.march(g, None, back[perm])
            assert np.array_equal(S.fetch(got, g.n_nodes), want[g.n_nodes])
            vs = S.upload(g.v_init)                           # v_init and payoff from slots
            got = S.march(g, vs, pay)
            assert np.array_equal(S.fetch(got, g.n_nodes), want[g.n_nodes])


def _mixed(engine=None):
    van = [make(engine, cls=AmericanFDMPricer, option_type="put"),
           make(engine, cls=AmericanFDMPricer, option_type="call", strike=235.0),
           make(engine, cls=AmericanFDMPricer, option_type="put",
                dividend_schedule=[(DIV_DAY, 2.5)])]
    bar = [make(engine, **TRADES[0][1]), make(engine, **TRADES[2][1]),
           make(engine, **TRADES[4][1])]
    return van, bar


def _results(ps):
    return [(p.greeks_log2(), p.price_log2()) for p in ps]


def test_mixed_greeks_many_and_chunking():
    van0, _ = _mixed()
    greeks_many(van0)
    van, bar = _mixed()
    greeks_many([van[0], bar[0], van[1], bar[1], bar[2], van[2]])
    assert _results(van) == _results(van0)  # bitwise: barrier trades change nothing

    van2, bar2 = _mixed()
    ps = [van2[0], bar2[0], van2[1], bar2[1], bar2[2], van2[2]]
    sessions = []
    import finite_difference_amd.american as A
    real = A.Session

    class Counting(real):
        def __init__(self):
            super().__init__()
            sessions.append(self)
    A.Session = Counting
    try:
        # slot estimates (7 grids a trade, 8 bytes x nodes x (segments + jumps
        # + payoff)): 7 224 for a vanilla trade, 43 344 and 50 960 for the
        # barrier trades, 28 896 with the dividend -- the first four fit
        # (101 136), the fifth does not: two sessions
        greeks_many(ps, max_slot_bytes=120_000)
    finally:
        A.Session = real
    assert len(sessions) == 2
    assert _results(van2) == _results(van) and _results(bar2) == _results(bar)
