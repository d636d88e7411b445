"""BermudanFDMPricer on the MI355X: the session path (Crank-Nicolson segments,
exercise events, plain knock-outs and dividend jumps chained on the device,
payoff uploaded once) against the host path on the CPU oracle.

Tolerances: those of test_gpu_american_barrier.py,
  value vectors  max|V - V_ref| <= 1e-10 * max(1, max|V_ref|)
and for the exercise boundary: equal to the host's, except that an edge may
move over nodes where the decision is within the vectors' tolerance,
|payoff - V_host| <= 1e-10 * max|V_host|.
The LSM check is that of test_bermudan_lsm_host.py, on the device engine."""
import numpy as np
import pytest

from backends import oracle_engine
from finite_difference_amd import (AmericanBarrierFDMPricer, AmericanKnockInFDMPricer,
                                   mc_american)
from finite_difference_amd.american import AmericanFDMPricer, greeks_many
from finite_difference_amd.session import Session
from test_bermudan_host import CHAIN_TRADES, WEEKLY, trade
from test_gpu_american_barrier import make as make_american

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host():
    """(V, exercise_boundary, host_events) of the three trades on the oracle,
    computed once for the module."""
    out = {}
    for n, m in ((128, 96), (400, 400)):
        for name, kw in CHAIN_TRADES:
            p = trade(oracle_engine(), n=n, m=m, **kw)
            V = np.array(p._solve_grid())
            out[(name, n)] = (V, p.exercise_boundary(), host_events(p))
    return out


def host_events(p):
    """Per exercise date, in calendar order, on the host path: the nodes that
    are in the exercise region whatever a vector error within tolerance does
    (`sure`), and the nodes that may be in it (`may`: those, and the
    not-knocked nodes with |payoff - V_host| <= 1e-10 * max|V_host|)."""
    jobs, _ = p._device_jobs([(p.sigma, p.num_time_steps)])
    seen = []
    real = type(p)._apply_job_event

    def spy(self, j, seg, event):
        if event[0] == "ex":
            pay, v = self._payoff_array(), np.asarray(j["v"], dtype=np.float64)
            k = np.arange(v.shape[0])
            free = ~((k <= event[1]) | (k >= event[2]))
            near = np.abs(pay - v) <= 1e-10 * float(np.max(np.abs(v)))
            seen.append((free & (pay > v) & ~near, free & ((pay > v) | near)))
        return real(self, j, seg, event)
    type(p)._apply_job_event = spy
    try:
        p._march_jobs(jobs, p._engine())
    finally:
        type(p)._apply_job_event = real
    return seen[::-1]


@pytest.mark.parametrize("n,m", [(128, 96), (400, 400)])
@pytest.mark.parametrize("name,kw", CHAIN_TRADES, ids=[t[0] for t in CHAIN_TRADES])
def test_session_path_matches_host_path_on_the_oracle(host, name, kw, n, m):
    V_ref, b_ref, masks = host[(name, n)]
    p = trade(None, n=n, m=m, **kw)
    assert p._engine().on_device
    jobs, _ = p._device_jobs([(p.sigma, p.num_time_steps)])
    with Session() as S:
        AmericanFDMPricer._march_jobs_device(jobs, p._engine(), S)
        V = S.fetch([jobs[0]["slot"]], len(V_ref))[0]
    err = float(np.max(np.abs(V - V_ref)))
    print(f"[{name} {n}x{m}] vector max abs err {err:.3e} (max|V| {np.max(np.abs(V_ref)):.3f})")
    assert err <= 1e-10 * max(1.0, float(np.max(np.abs(V_ref))))

    b = p.exercise_boundary()
    assert len(b) == len(b_ref) == 4
    for r, w, (sure, may) in zip(b, b_ref, masks):
        assert r[:2] == w[:2]
        if not np.any(may & ~sure):  # no decision within tolerance: the host's record
            assert r == w
            continue
        lo, hi, count = r[3:]
        assert int(sure.sum()) <= count <= int(may.sum())
        if count:
            first = np.nonzero(sure)[0]
            assert may[lo] and may[hi]
            assert first.size == 0 or (lo <= first[0] and hi >= first[-1])
        s = jobs[0]["grid"]["s_nodes"]
        put = p.option_type == "put"
        assert r[2] == (None if count == 0 else s[hi] if put else s[lo])


def _others(engine=None):
    return [make_american(engine, cls=AmericanFDMPricer, option_type="put"),
            make_american(engine, option_type="put", barrier_type="down-and-out",
                          lower_barrier=200.0),
            make_american(engine, cls=AmericanKnockInFDMPricer, option_type="put",
                          barrier_type="down-and-in", lower_barrier=200.0,
                          monitor_dates=WEEKLY),
            make_american(engine, cls=AmericanFDMPricer, option_type="call", strike=235.0)]


def _results(ps):
    return [(p.greeks_log2(), p.price_log2()) for p in ps]


def test_mixed_greeks_many_leaves_the_other_trades_bitwise():
    alone = _others()
    greeks_many(alone)
    mixed = _others()
    bs = [trade(None, n=128, m=96, **kw) for _, kw in CHAIN_TRADES]
    greeks_many([bs[0], mixed[0], mixed[1], bs[1], mixed[2], bs[2], mixed[3]])
    assert _results(mixed) == _results(alone)
    # and the Bermudan trades got their numbers: the host path's, within the
    # tolerances of the American GPU parity
    for b, (_, kw) in zip(bs, CHAIN_TRADES):
        ref = trade(oracle_engine(), n=128, m=96, **kw)
        g, g_ref = b.greeks_log2(), ref.greeks_log2()
        for k in g_ref:
            tol = (1e-10 + 1e-9 * abs(g_ref[k]) if k in ("price", "delta")
                   else 1e-8 * max(1.0, abs(g_ref[k])))
            assert abs(g[k] - g_ref[k]) <= tol, (k, g[k], g_ref[k])
        assert abs(b.price_log2() - ref.price_log2()) <= 1e-10 + 1e-9 * abs(ref.price_log2())


def test_fd_bermudan_agrees_with_the_lsm_on_the_device():
    kw = dict(strike=250.0, barrier_type="up-and-out", upper_barrier=240.0, rebate_amount=0.0,
              rebate_at_hit=True, monitor_dates=WEEKLY)
    p = trade(oracle_engine(), exercise_dates=WEEKLY, **kw)
    fd = p.price_log()
    r = mc_american.price_american_mc(mc_american.contract_from_pricer(p), n_subruns=64,
                                      engine="hip")
    bound = 0.01 * fd + 5.0 * r["stderr"]
    print(f"FD {fd:.6f} LSM {r['price']:.6f} +- {r['stderr']:.6f} bound {bound:.6f}")
    assert abs(fd - r["price"]) <= bound
    european = trade(oracle_engine(), **kw).price_log()
    american = trade(oracle_engine(), cls=AmericanBarrierFDMPricer, **kw).price_log()
    assert abs(european - r["price"]) > bound and abs(american - r["price"]) > bound
