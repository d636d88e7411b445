"""AmericanKnockInFDMPricer on the MI355X: the session path (both chains'
marches, knock-in events and dividend jumps chained on the device, payoff
uploaded once) against the host path on the CPU oracle.

Tolerances: those of the American knock-out parity (test_gpu_american_barrier.py):
  value vectors  max|V - V_ref| <= 1e-10 * max(1, max|V_ref|)
  price, delta   |x - ref| <= 1e-10 + 1e-9 |ref|
  gamma, theta, vega  |x - ref| <= 1e-8 * max(1, |ref|)
"""
import datetime as dt

import numpy as np
import pytest

import finite_difference_amd.american as A
from backends import oracle_engine
from finite_difference_amd import AmericanBarrierFDMPricer, AmericanKnockInFDMPricer, market
from finite_difference_amd.american import AmericanFDMPricer, greeks_many
from finite_difference_amd.session import Session

pytestmark = pytest.mark.gpu

VAL, MAT = dt.date(2025, 7, 28), dt.date(2025, 8, 28)
FIVE = [VAL + dt.timedelta(days=k) for k in (0, 4, 10, 15, 22, 31)]
CURVE = market.iso_curve(market.create_rate_df(0.073086))
DIV_DAY = VAL + dt.timedelta(days=10)

TRADES = [
    ("put_down_in", dict(option_type="put", barrier_type="down-and-in", lower_barrier=200.0)),
    ("put_up_in", dict(option_type="put", barrier_type="up-and-in", upper_barrier=250.0)),
    ("call_up_in", dict(option_type="call", barrier_type="up-and-in", upper_barrier=250.0)),
    ("put_double_in", dict(option_type="put", barrier_type="double-in", lower_barrier=200.0,
                           upper_barrier=250.0)),
    ("call_div_on_monitor_130", dict(option_type="call", barrier_type="double-in",
                                     lower_barrier=205.0, upper_barrier=250.0,
                                     rebate_amount=1.5, num_space_nodes=129,
                                     dividend_schedule=[(DIV_DAY, 2.5)])),
]
OUT = dict(option_type="put", barrier_type="down-and-out", lower_barrier=200.0)


def make(engine, cls=AmericanKnockInFDMPricer, **kw):
    args = dict(spot=229.74, strike=220.0, valuation_date=VAL, maturity_date=MAT, sigma=0.26,
                discount_curve=CURVE, forward_curve=CURVE, num_space_nodes=128,
                num_time_steps=96, rannacher_steps=2, engine=engine)
    if cls is not AmericanFDMPricer:
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
    assert jobs[0]["w_last"] == 3
    with Session() as S:
        AmericanFDMPricer._march_jobs_device(jobs, p._engine(), S)
        assert jobs[0]["slot"] != jobs[0]["wslot"]
        V = S.fetch([jobs[0]["slot"]], len(V_ref))[0]
    err = float(np.max(np.abs(V - V_ref)))
    print(f"[{name}] vector max abs err {err:.3e} (max|V| {np.max(np.abs(V_ref)):.3f})")
    assert err <= 1e-10 * max(1.0, float(np.max(np.abs(V_ref))))

    g, p2 = p.greeks_log2(), p.price_log2()
    print(f"[{name}] abs err", {k: abs(g[k] - g_ref[k]) for k in g_ref}, abs(p2 - p2_ref))
    for k in g_ref:
        assert close(k, g[k], g_ref[k]), (name, k, g[k], g_ref[k])
    assert close("price", p2, p2_ref)


def _others(engine=None):
    """Vanilla and knock-out trades, the kinds a knock-in must not disturb."""
    return [make(engine, cls=AmericanFDMPricer, option_type="put"),
            make(engine, cls=AmericanBarrierFDMPricer, **OUT),
            make(engine, cls=AmericanFDMPricer, option_type="call", strike=235.0),
            make(engine, cls=AmericanFDMPricer, option_type="put",
                 dividend_schedule=[(DIV_DAY, 2.5)]),
            make(engine, cls=AmericanBarrierFDMPricer, option_type="call",
                 barrier_type="double-out", lower_barrier=205.0, upper_barrier=250.0,
                 rebate_amount=1.5, num_space_nodes=129, dividend_schedule=[(DIV_DAY, 2.5)])]


def _knockins(engine=None):
    return [make(engine, **TRADES[0][1]), make(engine, **TRADES[2][1]),
            make(engine, **TRADES[4][1])]


def _results(ps):
    return [(p.greeks_log2(), p.price_log2()) for p in ps]


def test_mixed_greeks_many_and_chunking():
    oth0 = _others()
    greeks_many(oth0)
    kin0 = _knockins()
    greeks_many(kin0)
    oth, kin = _others(), _knockins()
    greeks_many([oth[0], kin[0], oth[1], oth[2], kin[1], oth[3], kin[2], oth[4]])
    assert _results(oth) == _results(oth0)  # bitwise: knock-in trades change nothing
    assert _results(kin) == _results(kin0)

    oth2, kin2 = _others(), _knockins()
    ps = [oth2[0], kin2[0], oth2[1], oth2[2], kin2[1], oth2[3], kin2[2], oth2[4]]
    need = [sum(A._job_slot_bytes(j) for j in p._device_jobs(p._device_requests(0.01, False))[0])
            for p in ps]
    # both chains of a knock-in job count: U's five marches, W's four and the
    # payoff on 129 nodes, seven grids -- against the knock-out's five and one
    assert need[1] == 7 * 8 * 129 * (5 + 4 + 1) and need[2] == 7 * 8 * 129 * (5 + 1)
    sessions = []
    real = A.Session

    class Counting(real):
        def __init__(self):
            super().__init__()
            sessions.append(self)
    A.Session = Counting
    try:
        greeks_many(ps, max_slot_bytes=sum(need) - 1)  # all but the last trade fit
    finally:
        A.Session = real
    assert len(sessions) == 2
    assert _results(oth2) == _results(oth) and _results(kin2) == _results(kin)
