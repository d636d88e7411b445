"""Shared pieces of the cash-dividend tests of the least-squares Monte Carlo
(test_mc_american_div_host.py, test_gpu_mc_american_div.py): the trades whose
FD price the LSM cross-checks, hand-built contracts with a dividend on any
step, the round-trip bound of the dividend map and a
stored-walk replay that never inverts the map."""
import math

import numpy as np

import lsm_fixture as lf
import test_bermudan_host as tb
from finite_difference_amd import AmericanBarrierFDMPricer, capi, mc_american
from finite_difference_amd.american import AmericanFDMPricer
from finite_difference_amd.bermudan import BermudanFDMPricer
from finite_difference_amd.mc_american import LsmContract, plan_american_contract

EPS = 2.0 ** -52
N = capi.LSM_SUBRUN
TINY_DIFF = 1e-300
KINDS = lf.KINDS


# ---------------------------------------------------------------------------
# the FD trades (spot 229.74, sigma 0.26, flat NACA 0.073086, one month)
# ---------------------------------------------------------------------------
DIV_MID = lf.WEEKDAYS[11]   # 2025-08-12, mid-life
DIV_WEEKLY = tb.DIV_DAY     # an exercise / monitoring date of the weekly trades


def _fd(cls, engine, n, **kw):
    return cls(spot=229.74, valuation_date=lf.VAL, maturity_date=lf.MAT, sigma=0.26,
               discount_curve=lf.CURVE, forward_curve=lf.CURVE, num_space_nodes=n,
               num_time_steps=n, rannacher_steps=2, engine=engine, **kw)


def american_call(engine, n, cls=AmericanFDMPricer, **kw):
    """Deep in the money, one large dividend mid-life: the textbook early
    exercise of a call, an instant before the dividend.  cls=BermudanFDMPricer
    without exercise dates is the same trade exercised at maturity only."""
    return _fd(cls, engine, n, strike=200.0, option_type="call",
               dividend_schedule=[(DIV_MID, 8.0)], **kw)


def bermudan_call(engine, n, dividend=True):
    kw = dict(dict(tb.CHAIN_TRADES)["call_div_on_exercise"])
    if not dividend:
        kw.pop("dividend_schedule")
    return tb.trade(engine, n=n, m=n, **kw)


def knock_out_put(engine, n, dividend=True):
    """Up-and-out put monitored weekly, a dividend on a monitoring date."""
    return _fd(AmericanBarrierFDMPricer, engine, n, strike=220.0, option_type="put",
               barrier_type="up-and-out", upper_barrier=245.0, monitor_dates=tb.WEEKLY,
               dividend_schedule=[(DIV_WEEKLY, 8.0)] if dividend else [])


FD_TRADES = {"american_call": american_call, "bermudan_call": bermudan_call,
             "knock_out_put": knock_out_put}
FD_N_EXERCISE = 16  # the American classes' exercise grid in these tests (<= 40 steps)


def fd_contract(name, pricer):
    return mc_american.contract_from_pricer(pricer, n_exercise=FD_N_EXERCISE,
                                            cash_dividends="path")


# ---------------------------------------------------------------------------
# hand-built contracts
# ---------------------------------------------------------------------------
def contract(kind, option_type, times, monitor, exercise, div, *, zero_length=(), strike=100.0,
             spot=100.0, rebate=0.0, at_hit=False, lower=88.0, upper=113.0):
    """plan_american_contract on the grid `times` with the MONITOR / EXERCISE
    flags written by row (lsm_fixture.plan_batch), then the dividend row `div`
    {row: cash} and the rows `zero_length` turned into steps without a move
    (DRIFT 0, DIFF 1e-300, DF_STEP 1).  CENTRE is rolled through the dividend
    map as the planner rolls it; a zero-length first step has ISCALE 1."""
    t = [float(v) for v in times]
    c = plan_american_contract(
        spot=spot, strike=strike, vol=0.3, option_type=option_type, discount_rate=0.05,
        carry_rate=0.03, time_to_expiry=t[-1], barrier_type=kind,
        lower_barrier=lower if ("down" in kind or "double" in kind) else None,
        upper_barrier=upper if ("up" in kind or "double" in kind) else None,
        monitor_times=[t[i] for i in monitor], rebate_amount=rebate, rebate_at_hit=at_hit,
        exercise_times=t)
    assert c.n_steps == len(t)
    S = c.step
    S[:, capi.LSM_S_EXERCISE] = 0.0
    S[list(exercise), capi.LSM_S_EXERCISE] = 1.0
    for i in zero_length:  # the step's own move goes; the later rows keep theirs
        S[i, [capi.LSM_S_DRIFT, capi.LSM_S_DIFF, capi.LSM_S_DF_STEP]] = 0.0, TINY_DIFF, 1.0
    row = np.zeros(len(t))
    for i, d in div.items():
        row[i] = d
    base, drift, var = math.log(spot), 0.0, 0.0  # the planner's own arithmetic
    for i in range(len(t)):
        drift += S[i, capi.LSM_S_DRIFT]
        var += S[i, capi.LSM_S_DIFF] * S[i, capi.LSM_S_DIFF]
        if row[i] != 0.0:
            base, drift = float(mc_american._div_forward(np.float64(base + drift), row[i])), 0.0
        S[i, capi.LSM_S_CENTRE] = base + drift
        S[i, capi.LSM_S_ISCALE] = 1.0 / math.sqrt(var) if var > 0.0 else 1.0
    c.div = row
    return c


# ---- the device / host parity batches --------------------------------------
T8 = [0.5 * k / 8 for k in range(1, 9)]
T3 = [0.1, 0.27, 0.5]
BIG_D = 45.0  # of spot 100: a fifth of the paths is below 2 D and takes the lower branch


def _kind_kw(kind, k):
    """Rebate at the hit for the knock-outs, at maturity for the knock-ins."""
    return dict(rebate=0.0 if kind == "none" else 1.0 + 0.1 * k, at_hit=kind.endswith("-out"))


def div_batches():
    """name -> (n_subruns, antithetic, seed, [contracts]).  Dividends on the
    first step, on an even and on an odd step (a Philox pair is steps 2 j + 1
    and 2 j + 2), on two consecutive steps, on the last step and on a
    zero-length step; every kind, puts and calls; one contract per batch of
    three or eight steps with a dividend of BIG_D."""
    out = {}
    mon8, ex8 = (1, 4, 5, 7), range(8)
    spec8 = [("none", "put", {0: 2.0}, ()), ("down-and-out", "call", {1: 1.5}, ()),
             ("up-and-out", "put", {2: 1.5}, ()), ("double-out", "call", {3: 1.0, 4: 1.0}, ()),
             ("down-and-in", "put", {7: 2.0}, ()), ("up-and-in", "call", {4: 2.0}, (4,)),
             ("double-in", "put", {5: 1.0}, ())]
    out["m8_div"] = (2, True, 111, [
        contract(k, ot, T8, mon8 if k != "none" else (), ex8, d, zero_length=z, **_kind_kw(k, i))
        for i, (k, ot, d, z) in enumerate(spec8)]
        + [contract("none", "put", T8, (), ex8, {2: BIG_D}, strike=60.0)])
    div3 = [{0: 2.0}, {1: 2.0}, {2: 2.0}, {0: 1.0, 1: 1.0}, {1: 1.0, 2: 1.0}, {1: 2.0}, {0: 1.5}]
    out["m3_div"] = (3, False, 112, [
        contract(k, "call" if i % 2 else "put", T3, (0, 2) if k != "none" else (), range(3),
                 div3[i], zero_length=(1,) if i == 5 else (), **_kind_kw(k, i))
        for i, k in enumerate(KINDS)]
        + [contract("none", "put", T3, (), range(3), {0: BIG_D}, strike=60.0)])
    out["m2_div"] = (1, True, 113, [
        contract(k, "put", [0.2, 0.5], (0,) if k != "none" else (), range(2),
                 {i % 2: 2.0}, **_kind_kw(k, i)) for i, k in enumerate(KINDS)])
    out["m1_div"] = (2, False, 114, [
        contract(k, "put" if i % 2 else "call", [0.5], (0,) if k != "none" else (), (0,),
                 {0: 2.0}, **_kind_kw(k, i)) for i, k in enumerate(KINDS)])
    return out


# Per contract the first stream id (pick_stream_ids) at which the host engine's
# smallest decision margin is at least 100 tau_c = lsm_fixture.MIN_MARGIN x
# strike / 100: no exercise decision can flip inside the continuation-value
# tolerance.  test_mc_american_div_host.py checks the condition on the CPU.
STREAM_IDS = {
    "m8_div": [0, 0, 0, 0, 0, 0, 1, 2],
    "m3_div": [0, 0, 0, 0, 0, 0, 0, 0],
    "m2_div": [0, 0, 0, 0, 0, 0, 0],
    "m1_div": [0, 0, 0, 0, 0, 0, 0],
}


def min_margin(c):
    return 100.0 * lf.TAU_C_REL * float(c.params[capi.LSM_P_STRIKE])


def pick_stream_ids(tries=64):
    """The generator of STREAM_IDS."""
    out = {}
    for name, (G, anti, seed, cs) in div_batches().items():
        out[name] = [next(sid for sid in range(tries)
                          if float(mc_american.host_subruns(c, range(G), anti, seed, sid)
                                   ["margin"].min()) >= min_margin(c)) for c in cs]
    return out


def with_initial_dividend(c, d):
    """Contract c (planned without dividends) behind a zero-length first step
    at valuation that pays d: the same trade started at spot - d."""
    x0 = float(np.log(c.params[capi.LSM_P_SPOT]))
    first = np.zeros((1, capi.LSM_NSTEP))
    first[0, [capi.LSM_S_DIFF, capi.LSM_S_DF_STEP, capi.LSM_S_DF_END, capi.LSM_S_ISCALE]] = (
        TINY_DIFF, 1.0, 1.0, 1.0)
    ex = float(mc_american._div_forward(np.float64(x0), d))
    first[0, capi.LSM_S_CENTRE] = ex
    step = np.vstack([first, c.step])
    step[1:, capi.LSM_S_CENTRE] += ex - x0
    return LsmContract(params=c.params.copy(), flags=c.flags.copy(), step=step,
                       times=np.concatenate([[0.0], c.times]), barrier_type=c.barrier_type,
                       div=np.concatenate([[d], np.zeros(c.n_steps)]))


# ---------------------------------------------------------------------------
# the dividend map
# ---------------------------------------------------------------------------
def round_trip_bound(x, d):
    """Bound on |g^-1(g(x)) - x| in float64: with t the
    ex-dividend spot and y = log t, 2 EPS (3 + D / t + |x| + |y|)."""
    s = np.exp(x)
    t = np.where(s >= 2.0 * d, s - d, 0.5 * s)
    return 2.0 * EPS * (3.0 + d / t + np.abs(x) + np.abs(np.log(t)))


# ---------------------------------------------------------------------------
# the stored-walk replay (kind "none" only)
# ---------------------------------------------------------------------------
def stored_walk(c, z):
    """(pre, post): the cum- and the ex-dividend log-spot of every step,
    [M][n], walked forward only."""
    S, D = c.step, c.div_row()
    x = np.full(z.shape[0], float(np.log(c.params[capi.LSM_P_SPOT])))
    pre, post = [], []
    for i in range(c.n_steps):
        x = x + (S[i, capi.LSM_S_DRIFT] + S[i, capi.LSM_S_DIFF] * z[:, i])
        pre.append(x)
        if D[i] != 0.0:
            x = mc_american._div_forward(x, D[i])
        post.append(x)
    return pre, post


def replay_subrun(c, g, antithetic, seed, sid):
    """One sub-run of a contract without a barrier, the algorithm of
    include/fdcn.h on stored walks: phase B reads x_m from the forward walk and
    never applies the inverse map.  -> values [N], min margin, the fit set's
    cum-dividend log-spots, coef [M, 4]."""
    assert int(c.flags[capi.LSM_F_KIND]) == 0
    S, M = c.step, c.n_steps
    strike, put = float(c.params[capi.LSM_P_STRIKE]), bool(c.flags[capi.LSM_F_PUT])
    per = mc_american.obs_per_subrun(antithetic)

    def payoff(x):
        s = np.exp(x)
        return np.maximum(strike - s, 0.0) if put else np.maximum(s - strike, 0.0)

    def regressor(x, i):
        return (x - S[i, capi.LSM_S_CENTRE]) * S[i, capi.LSM_S_ISCALE]

    z = mc_american._path_normals(M, seed, 2 * sid, g * per, antithetic)
    pre, post = stored_walk(c, z)
    coef, valid, margin = np.zeros((M, 4)), np.zeros(M, dtype=bool), math.inf
    cf = payoff(post[M - 1])
    for m in range(M, 0, -1):
        i = m - 1
        if m < M and S[i, capi.LSM_S_EXERCISE] != 0.0:
            phi, u = payoff(post[i]), regressor(post[i], i)
            part = phi > 0.0
            u2 = u * u
            u3 = u2 * u
            terms = [np.ones_like(u), u, u2, u3, u2 * u2, u3 * u2, u3 * u3, cf, u * cf, u2 * cf,
                     u3 * cf, np.ones_like(u)]
            sm = np.array([[np.sum(np.where(part, t, 0.0)) for t in terms]])
            cc, ok = mc_american._cholesky_cubic(sm)
            coef[i], valid[i] = cc[0], ok[0]
            if ok[0]:
                fit = mc_american._cubic(cc, u[None, :])[0]
                margin = min(margin, float(np.abs(phi - fit)[part].min()))
                cf = np.where(part & (phi > fit), phi, cf)
        cf = cf * S[i, capi.LSM_S_DF_STEP]
    z = mc_american._path_normals(M, seed, 2 * sid + 1, g * per, antithetic)
    _, post_p = stored_walk(c, z)
    val, done = np.zeros(N), np.zeros(N, dtype=bool)
    for m in range(1, M + 1):
        i = m - 1
        phi = payoff(post_p[i])
        if m == M:
            val = np.where(done, val, phi * S[i, capi.LSM_S_DF_END])
        elif valid[i]:
            fit = mc_american._cubic(coef[i][None, :], regressor(post_p[i], i)[None, :])[0]
            cand = ~done & (phi > 0.0)
            if cand.any():
                margin = min(margin, float(np.abs(phi - fit)[cand].min()))
            go = cand & (phi > fit)
            val = np.where(go, phi * S[i, capi.LSM_S_DF_END], val)
            done |= go
    return val, margin, pre, coef
