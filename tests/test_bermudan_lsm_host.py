"""The least-squares Monte Carlo as the cross-check of BermudanFDMPricer
(host engine): contract_from_pricer takes the pricer's own exercise dates,
and the FD Bermudan price lies within

    |FD - LSM| <= 0.01 FD + 5 s.e.

of the LSM price: the policy-bias and 5-standard-error part of
lsm_fixture.fd_gap_bound, without its grid-doubling term (which could only
loosen the bound).  On the strike-250 trades the same bound around the LSM
price excludes both FD neighbours, the European and the American knock-out:
the check tells Bermudan from either."""
import numpy as np
import pytest

from backends import oracle_engine
from finite_difference_amd import AmericanBarrierFDMPricer, capi, mc_american
from test_bermudan_host import WEEKDAYS, WEEKLY, trade

UP_OUT = [(220.0, 0.0), (220.0, 1.5), (250.0, 0.0), (250.0, 1.5)]


def barrier_kw(strike, rebate):
    return dict(strike=strike, barrier_type="up-and-out", upper_barrier=240.0,
                rebate_amount=rebate, rebate_at_hit=True, monitor_dates=WEEKLY)


def test_the_contract_carries_the_pricers_exercise_dates():
    p = trade(oracle_engine(), exercise_dates=WEEKLY, **barrier_kw(220.0, 1.5))
    c = mc_american.contract_from_pricer(p, n_exercise=7)  # n_exercise is ignored
    T = p.time_to_expiry
    want = sorted(T - tau for tau, _ in p._exercise_taus()) + [T]
    assert c.n_steps == 5 and np.allclose(c.times, want, rtol=0, atol=1e-15)
    assert list(c.step[:, capi.LSM_S_EXERCISE]) == [1.0, 1.0, 1.0, 1.0, 0.0]
    assert list(c.step[:, capi.LSM_S_MONITOR]) == [1.0, 1.0, 1.0, 1.0, 0.0]
    # without exercise dates: the European contract, whatever n_exercise says
    e = mc_american.contract_from_pricer(trade(oracle_engine()), n_exercise=64)
    assert e.n_steps == 1 and e.step[0, capi.LSM_S_EXERCISE] == 0.0
    # the American classes keep their n_exercise grid
    a = mc_american.contract_from_pricer(
        trade(oracle_engine(), cls=AmericanBarrierFDMPricer, **barrier_kw(220.0, 0.0)), 16)
    assert int(a.step[:, capi.LSM_S_EXERCISE].sum()) == 16


@pytest.mark.parametrize("strike,rebate", UP_OUT)
def test_fd_bermudan_agrees_with_the_lsm(strike, rebate):
    eng = oracle_engine()
    kw = barrier_kw(strike, rebate)
    p = trade(eng, exercise_dates=WEEKLY, **kw)
    fd = p.price_log()
    r = mc_american.price_american_mc(mc_american.contract_from_pricer(p), n_subruns=64,
                                      engine="host")
    bound = 0.01 * fd + 5.0 * r["stderr"]
    print(f"K {strike} R {rebate}: FD {fd:.6f} LSM {r['price']:.6f} +- {r['stderr']:.6f} "
          f"gap {abs(fd - r['price']):.6f} bound {bound:.6f}")
    assert abs(fd - r["price"]) <= bound
    if strike == 250.0:
        european = trade(eng, **kw).price_log()
        american = trade(eng, cls=AmericanBarrierFDMPricer, **kw).price_log()
        print(f"   European KO {european:.6f}  American KO {american:.6f}")
        assert abs(european - r["price"]) > bound and abs(american - r["price"]) > bound


def test_a_monitoring_date_that_is_no_exercise_date_is_refused():
    kw = barrier_kw(220.0, 0.0)
    kw["monitor_dates"] = WEEKDAYS
    with pytest.raises(ValueError, match="not an exercise date"):
        mc_american.contract_from_pricer(trade(oracle_engine(), exercise_dates=WEEKLY, **kw))
