"""Cash dividends in the dual and the table-policy Monte Carlo bounds, without a
GPU: the opt-in, the NumPy host engines against a per-path walk written from
the contract text of include/fdcn.h (move, g, events), their identities and
invariants with dividends, the two-step dividend date of from_critical_spots,
the C entries' validation of `div`, and two Bermudan calls end to end against
the FD price."""
import math

import numpy as np
import pytest

import bounds_div_cases as bdc
import lsm_div_cases as ldc
import lsm_fixture as lf
from backends import oracle_engine
from conftest import load_golden
from finite_difference_amd import capi, mc_american
from finite_difference_amd.mc_american import ExercisePolicy, LsmContract

GOLDEN = load_golden("bounds_div_cases.json")
PATH = "path"
LN2 = 0.6931471805599453
NEW = ("fdcn_mc_lsm_dual_div_batch", "fdcn_mc_lsm_dual_div_batch_dev",
       "fdcn_mc_policy_div_batch", "fdcn_mc_policy_div_batch_dev",
       "fdcn_mc_policy_dual_div_batch", "fdcn_mc_policy_dual_div_batch_dev")


@pytest.fixture(scope="module")
def runs():
    """Per batch, computed once: the batch, the golden stream ids, the fitted
    policies and the three host references."""
    out = {}
    for name in bdc.PARITY:
        G, anti, seed, plans, pols, lsm_ids = bdc.batch(name)
        g = GOLDEN["batches"][name]
        coef = bdc.fitted(name)
        out[name] = dict(G=G, anti=anti, seed=seed, plans=plans, pols=pols, coef=coef,
                         table_ids=g["table_ids"], fit_ids=g["fit_ids"],
                         lower=bdc.host_lower(name, g["table_ids"]),
                         table_dual=bdc.host_table_dual(name, g["table_ids"]),
                         fit_dual=bdc.host_fitted_dual(name, coef, g["fit_ids"]))
    return out


# ---------------------------------------------------------------------------
# 1. the opt-in
# ---------------------------------------------------------------------------
def _small():
    """A three-step up-and-out put with a dividend on its second step, its table
    and the fits of one sub-run."""
    G, anti, seed, plans, pols, lsm_ids = bdc.batch("m3_div")
    c, pol = plans[2], pols[2]
    assert c.has_dividends and not anti
    coef = mc_american.host_subruns(c, range(1), anti, seed, 0)["coef"]
    return c, pol, coef, seed


def _calls():
    c, pol, coef, seed = _small()
    cfg = mc_american.LsmConfig(n_subruns=1, antithetic=False, seed=seed)
    dual = mc_american.DualConfig(1, 256)
    host = dict(engine="host")
    one = dict(n_subruns=1, antithetic=False, seed=seed, engine="host")
    plan_kw = dict(spot=100.0, strike=100.0, vol=0.3, option_type="call", discount_rate=0.05,
                   carry_rate=0.03, time_to_expiry=0.5, n_exercise=2, dividends=[(0.2, 2.0)])
    return {
        "mc_american_bounds_batch":
            lambda **kw: mc_american.mc_american_bounds_batch([c], cfg, dual, **host, **kw),
        "mc_american_bounds_batch (keywords)":
            lambda **kw: mc_american.mc_american_bounds_batch([plan_kw], cfg, dual, **host, **kw),
        "price_american_mc_bounds":
            lambda **kw: mc_american.price_american_mc_bounds(n_outer=1, n_inner=256, **one,
                                                              **plan_kw, **kw),
        "simulate_dual":
            lambda **kw: mc_american.simulate_dual([c], coef[None], 1, 256, False, seed=seed,
                                                   **host, **kw),
        "host_dual_subruns":
            lambda **kw: mc_american.host_dual_subruns(c, coef, range(1), 1, 256, False, seed, 0,
                                                       **kw),
        "simulate_policy":
            lambda **kw: mc_american.simulate_policy([c], [pol], 1, False, seed=seed, **host, **kw),
        "simulate_policy_dual":
            lambda **kw: mc_american.simulate_policy_dual([c], [pol], 1, 1, 256, False, seed=seed,
                                                          **host, **kw),
        "host_policy_subruns":
            lambda **kw: mc_american.host_policy_subruns(c, pol, range(1), False, seed, 0, **kw),
        "host_policy_dual_subruns":
            lambda **kw: mc_american.host_policy_dual_subruns(c, pol, range(1), 1, 256, False,
                                                              seed, 0, **kw),
        "mc_policy_batch":
            lambda **kw: mc_american.mc_policy_batch([c], [pol], cfg, **host, **kw),
        "price_policy_mc":
            lambda **kw: mc_american.price_policy_mc(c, pol, **one, **kw),
        "mc_policy_bounds_batch":
            lambda **kw: mc_american.mc_policy_bounds_batch([c], [pol], cfg, dual, **host, **kw),
        "price_policy_mc_bounds":
            lambda **kw: mc_american.price_policy_mc_bounds(c, pol, n_outer=1, n_inner=256, **one,
                                                            **kw),
    }


@pytest.mark.parametrize("name", list(_calls()))
def test_every_entry_point_takes_dividends_only_on_request(name):
    fn = _calls()[name]
    with pytest.raises(ValueError, match="dividends"):
        fn()
    with pytest.raises(ValueError, match="dividends"):
        fn(cash_dividends="refuse")
    with pytest.raises(ValueError, match="cash_dividends must be"):
        fn(cash_dividends="spline")
    assert fn(cash_dividends=PATH) is not None


def test_policy_from_pricer_takes_a_dividend_bermudan_only_on_request():
    p = bdc.trade("weekly_230", oracle_engine(), 100)
    with pytest.raises(ValueError, match="dividends"):
        mc_american.policy_from_pricer(p)
    with pytest.raises(ValueError, match="cash_dividends must be"):
        mc_american.policy_from_pricer(p, cash_dividends="spline")
    c = mc_american.contract_from_pricer(p, cash_dividends=PATH)
    with pytest.raises(ValueError, match="dividends"):
        mc_american.policy_from_pricer(p, c)
    pol = mc_american.policy_from_pricer(p, cash_dividends=PATH)
    assert c.has_dividends and pol.n_steps == c.n_steps
    # one step per date, the dividend's included: the exercise date that is the
    # dividend date has its record, in ex-dividend spots, on that single step
    i = int(np.nonzero(c.div_row())[0][0])
    assert c.step[i, capi.LSM_S_EXERCISE] != 0.0 and np.all(np.diff(c.times) > 1e-9)
    # a call's threshold, or "never": no dividend is left after this one
    assert (pol.x_lo[i], pol.x_hi[i]) == (math.inf, -math.inf) or \
        (math.isfinite(pol.x_lo[i]) and pol.x_hi[i] == math.inf)
    again = mc_american.policy_from_pricer(p, c, cash_dividends=PATH)
    assert np.array_equal(again.table(), pol.table())


def test_symbols_are_exported_and_the_abi_is_still_8():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(L, name), name
    assert L.fdcn_abi_version() == 8


# ---------------------------------------------------------------------------
# 2. the host engine against a per-path walk
# ---------------------------------------------------------------------------
def _walk(c, pol, z):
    """One path under the rule of include/fdcn.h (fdcn_mc_policy_div_batch),
    statement by statement: the move, the dividend map g, then the step's
    events on the ex-dividend spot.  -> (value, the step at which it stopped,
    whether the rule stopped it).  np.exp and np.log on a scalar are the array
    loops of one element, so the spot is the host engine's bit for bit."""
    P, F, S, D = c.params, c.flags, c.step, c.div_row()
    strike, lower, upper = (float(P[k]) for k in (capi.LSM_P_STRIKE, capi.LSM_P_LOWER,
                                                  capi.LSM_P_UPPER))
    put, kind = bool(F[capi.LSM_F_PUT]), int(F[capi.LSM_F_KIND])
    ko, ki = 1 <= kind <= 3, kind >= 4
    has_lo, has_hi = kind in (1, 3, 4, 6), kind in (2, 3, 5, 6)
    x = float(np.log(P[capi.LSM_P_SPOT]))
    eligible = not ki
    M = c.n_steps
    for m in range(1, M + 1):
        r = S[m - 1]
        x = x + (float(r[capi.LSM_S_DRIFT]) + float(r[capi.LSM_S_DIFF]) * float(z[m - 1]))
        d = float(D[m - 1])
        if d != 0.0:
            cum = float(np.exp(np.float64(x)))
            x = float(np.log(np.float64(cum - d))) if cum >= 2.0 * d else x - LN2
        s = float(np.exp(np.float64(x)))
        phi = max(strike - s, 0.0) if put else max(s - strike, 0.0)
        dfe, reb = float(r[capi.LSM_S_DF_END]), float(r[capi.LSM_S_REBATE])
        if kind != 0 and r[capi.LSM_S_MONITOR] != 0.0:
            if (has_lo and s <= lower) or (has_hi and s >= upper):
                if ko:
                    return max(phi, reb) * dfe, m, False
                eligible = True
        if m == M:
            return (phi if eligible else reb) * dfe, m, False
        if (r[capi.LSM_S_EXERCISE] != 0.0 and eligible and phi > 0.0
                and pol.x_lo[m - 1] <= x <= pol.x_hi[m - 1]):
            return phi * dfe, m, True
    raise AssertionError("maturity always stops")


@pytest.mark.parametrize("name", ["m3_div", "m8_div"])
def test_host_engine_is_the_per_path_walk(runs, name):
    r = runs[name]
    per = mc_american.obs_per_subrun(r["anti"])
    lower_branch = 0
    for b, (c, pol, sid, h) in enumerate(zip(r["plans"], r["pols"], r["table_ids"], r["lower"])):
        for g in range(r["G"]):
            Z = mc_american._path_normals(c.n_steps, r["seed"], 2 * sid + 1, g * per, r["anti"])
            by_rule = 0
            for p in range(capi.LSM_SUBRUN):
                v, m, ruled = _walk(c, pol, Z[p])
                assert v == h["values"][g, p] and m == h["stop_step"][g, p], (name, b, g, p)
                by_rule += ruled
            assert by_rule == h["exercised"][g], (name, b, g)
        if np.any(c.div_row() == ldc.BIG_D):
            # a fifth of the paths reaches the dividend below 2 D
            i = int(np.argmax(c.div_row()))
            Z = mc_american._path_normals(c.n_steps, r["seed"], 2 * sid + 1, 0, r["anti"])
            cum = ldc.stored_walk(c, Z)[0][i]
            lower_branch = float(np.mean(np.exp(cum) < 2.0 * ldc.BIG_D))
    assert 0.1 < lower_branch < 0.4, lower_branch


def test_the_fixture_holds_the_cases_the_device_test_needs(runs):
    """Every step count and kind; a dividend on the first, an odd, an even, the
    last and a zero-length step and on two in a row; in the duals a start step
    whose next step pays (inner t = 0), one that pays itself, an odd number of
    remaining steps, and an outer path knocked out on a dividend step."""
    assert {c.n_steps for r in runs.values() for c in r["plans"]} == {1, 2, 3, 8}
    assert {int(c.flags[capi.LSM_F_KIND]) for c in runs["m8_div"]["plans"]} == set(range(7))
    assert {bool(c.flags[capi.LSM_F_PUT]) for r in runs.values() for c in r["plans"]} == \
        {True, False}
    where = set()
    for r in runs.values():
        for c in r["plans"]:
            d = c.div_row() != 0.0
            where |= {"first"} if d[0] else set()
            where |= {"last"} if d[-1] else set()
            where |= {("even", "odd")[i % 2] for i in np.nonzero(d)[0]}
            where |= {"pair"} if np.any(d[:-1] & d[1:]) else set()
            where |= {"zero"} if np.any(d & (c.step[:, capi.LSM_S_DIFF] == ldc.TINY_DIFF)) \
                else set()
    assert where == {"first", "last", "even", "odd", "pair", "zero"}
    seen = set()
    for key in ("table_dual", "fit_dual"):
        for r in runs.values():
            for c, h in zip(r["plans"], r[key]):
                d, M = c.div_row() != 0.0, c.n_steps
                ko = 1 <= int(c.flags[capi.LSM_F_KIND]) <= 3
                mon = c.step[:, capi.LSM_S_MONITOR] != 0.0
                started = h["cont"].reshape(-1, M) != 0.0
                for i in np.nonzero(started.any(axis=0))[0]:
                    seen |= {(key, "next pays")} if i + 1 < M and d[i + 1] else set()
                    seen |= {(key, "pays itself")} if d[i] else set()
                    seen |= {(key, "odd rest")} if (M - 1 - i) % 2 else set()
                if ko and np.any(d & mon):
                    # a knocked-out outer path has no start after its breach; one
                    # whose last start is before a monitored dividend step i and
                    # whose walk ended there shows as all-zero cont from i on
                    # with starts before
                    i = int(np.nonzero(d & mon)[0][0])
                    ends = started[:, :i].any(axis=1) & ~started[:, i:].any(axis=1)
                    seen |= {(key, "knocked out on a dividend step")} if ends.any() else set()
    for key in ("table_dual", "fit_dual"):
        for what in ("next pays", "pays itself", "odd rest", "knocked out on a dividend step"):
            assert (key, what) in seen, (key, what)


def test_golden_stream_ids_reproduce_their_margins(runs):
    assert GOLDEN["tau_x"] == bdc.TAU_X and GOLDEN["min_margin_x_required"] == bdc.MIN_MARGIN_X
    for name, r in runs.items():
        g = GOLDEN["batches"][name]
        assert (g["n_outer"], g["n_inner"]) == bdc.PARITY[name]
        assert len(g["table_ids"]) == len(g["fit_ids"]) == len(r["plans"])  # nobody dropped
        for b, c in enumerate(r["plans"]):
            assert 16 * b <= g["table_ids"][b] < 16 * (b + 1)
            assert 16 * b <= g["fit_ids"][b] < 16 * (b + 1)
            ml, md = r["lower"][b]["margin"].min(), r["table_dual"][b]["margin"].min()
            mf = r["fit_dual"][b]["margin"].min()
            assert lf.finite(ml) == g["lower_margin"][b]
            assert lf.finite(md) == g["table_dual_margin"][b]
            assert lf.finite(mf) == g["fit_dual_margin"][b]
            assert min(ml, md) >= bdc.MIN_MARGIN_X and mf >= bdc.min_margin_c(c), (name, b)


# ---------------------------------------------------------------------------
# 3. equivalences, bit for bit
# ---------------------------------------------------------------------------
def _without_exercise(c):
    f = LsmContract(params=c.params, flags=c.flags, step=c.step.copy(), times=c.times,
                    barrier_type=c.barrier_type, div=c.div)
    f.step[:, capi.LSM_S_EXERCISE] = 0.0
    return f


def test_a_never_stop_table_is_the_lsm_price_set_without_exercise_flags(runs):
    for name, r in runs.items():
        for c, sid in zip(r["plans"], r["table_ids"]):
            never = mc_american.host_policy_subruns(c, ExercisePolicy.never(c.n_steps),
                                                    range(r["G"]), r["anti"], r["seed"], sid, PATH)
            lsm = mc_american.host_subruns(_without_exercise(c), range(r["G"]), r["anti"],
                                           r["seed"], sid)
            assert np.array_equal(never["values"], lsm["values"]), name
            assert np.all(never["exercised"] == 0.0) and np.all(np.isposinf(never["margin"]))


def test_an_all_zero_div_through_the_path_route_is_the_plain_route(runs):
    for name, r in runs.items():
        n_outer, n_inner = bdc.PARITY[name]
        sub, anti, seed = range(r["G"]), r["anti"], r["seed"]
        for b, (c, pol, sid) in enumerate(zip(r["plans"], r["pols"], r["table_ids"])):
            plain = LsmContract(params=c.params, flags=c.flags, step=c.step, times=c.times,
                                barrier_type=c.barrier_type)
            zero = LsmContract(params=c.params, flags=c.flags, step=c.step, times=c.times,
                               barrier_type=c.barrier_type, div=np.zeros(c.n_steps))
            assert not zero.has_dividends
            a = mc_american.host_policy_subruns(plain, pol, sub, anti, seed, sid)
            z = mc_american.host_policy_subruns(zero, pol, sub, anti, seed, sid, PATH)
            for k in ("values", "stop_step", "means", "margin", "exercised"):
                assert np.array_equal(a[k], z[k]), (name, b, k)
            duals = [
                (mc_american.host_policy_dual_subruns(plain, pol, sub, n_outer, n_inner, anti,
                                                      seed, sid),
                 mc_american.host_policy_dual_subruns(zero, pol, sub, n_outer, n_inner, anti,
                                                      seed, sid, PATH)),
                (mc_american.host_dual_subruns(plain, r["coef"][b], sub, n_outer, n_inner, anti,
                                               seed, sid),
                 mc_american.host_dual_subruns(zero, r["coef"][b], sub, n_outer, n_inner, anti,
                                               seed, sid, PATH))]
            for a, z in duals:
                for k in ("gaps", "cont", "margin", "inner_paths", "inner_steps"):
                    assert np.array_equal(a[k], z[k]), (name, b, k)


def test_the_table_dual_under_never_is_the_fitted_dual_under_zero_coef(runs):
    for name, r in runs.items():
        n_outer, n_inner = bdc.PARITY[name]
        for c, sid in zip(r["plans"], r["table_ids"]):
            a = mc_american.host_policy_dual_subruns(
                c, ExercisePolicy.never(c.n_steps), range(r["G"]), n_outer, n_inner, r["anti"],
                r["seed"], sid, PATH)
            z = mc_american.host_dual_subruns(
                c, np.zeros((r["G"], c.n_steps, capi.LSM_NCOEF)), range(r["G"]), n_outer, n_inner,
                r["anti"], r["seed"], sid, PATH)
            for k in ("gaps", "cont", "margin", "inner_paths", "inner_steps"):
                assert np.array_equal(a[k], z[k]), (name, k)


# ---------------------------------------------------------------------------
# 4. the dual's invariants, with dividends
# ---------------------------------------------------------------------------
def test_dual_invariants_hold_with_dividends(runs):
    for name, r in runs.items():
        for key in ("table_dual", "fit_dual"):
            for c, h in zip(r["plans"], r[key]):
                assert np.all(h["gaps"] >= 0.0) and np.all(np.isfinite(h["gaps"])), (name, key)
                assert np.all(h["cont"] >= 0.0)
                started = h["inner_paths"].sum() / bdc.PARITY[name][1]
                assert np.count_nonzero(h["cont"]) <= started
                if not np.any(c.step[:-1, capi.LSM_S_EXERCISE] != 0.0):
                    assert np.all(h["gaps"] == 0.0) and h["inner_paths"].sum() == 0.0
                    assert np.all(h["cont"] == 0.0)
    # a contract without an EXERCISE step before maturity exists in the fixture
    assert any(not np.any(c.step[:-1, capi.LSM_S_EXERCISE] != 0.0)
               for r in runs.values() for c in r["plans"])


def test_cont_is_zero_where_no_inner_simulation_started(runs):
    """Only an EXERCISE step before maturity can start one, and none starts
    after a knock-out."""
    for name, r in runs.items():
        for key in ("table_dual", "fit_dual"):
            for c, h in zip(r["plans"], r[key]):
                ex = c.step[:, capi.LSM_S_EXERCISE] != 0.0
                ex[-1] = False
                assert np.all(h["cont"][..., ~ex] == 0.0), (name, key)


def test_two_shards_of_sub_runs_merge_to_the_whole_run():
    name = "m8_div"
    G, anti, seed, plans, pols, _ = bdc.batch(name)
    g = GOLDEN["batches"][name]
    n_outer, n_inner = bdc.PARITY[name]
    cfg = mc_american.LsmConfig(n_subruns=G, antithetic=anti, seed=seed)
    dual = mc_american.DualConfig(n_outer, n_inner)
    pick = [1, 7]  # a knock-out call and the D = 45 put
    cs, ps, ids = [plans[k] for k in pick], [pols[k] for k in pick], [g["table_ids"][k] for k in pick]
    kw = dict(engine="host", stream_ids=ids, cash_dividends=PATH)
    whole = mc_american.mc_policy_bounds_batch(cs, ps, cfg, dual, **kw)
    parts = [mc_american.mc_policy_bounds_batch(cs, ps, cfg, dual, subrun_range=range(k, k + 1),
                                                **kw) for k in range(G)]
    fit_whole = mc_american.mc_american_bounds_batch(cs, cfg, dual, **kw)
    fit_parts = [mc_american.mc_american_bounds_batch(cs, cfg, dual, subrun_range=range(k, k + 1),
                                                      **kw) for k in range(G)]
    for b in range(len(cs)):
        m = mc_american.merge_policy_stats([p[b] for p in parts])
        assert m["price"] == pytest.approx(whole[b]["price"], rel=1e-14)
        assert m["stderr"] == pytest.approx(whole[b]["stderr"], rel=1e-9)
        assert m["exercised"] == whole[b]["exercised"]
        for w, ps_ in ((whole, parts), (fit_whole, fit_parts)):
            d = mc_american.merge_dual_stats([p[b] for p in ps_])
            assert d["gap"] == pytest.approx(w[b]["gap"], rel=1e-14)
            assert d["gap_stderr"] == pytest.approx(w[b]["gap_stderr"], rel=1e-9, abs=1e-18)
            assert sum(p[b]["inner_paths"] for p in ps_) == w[b]["inner_paths"]


# ---------------------------------------------------------------------------
# 5. the dividend is on the path
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m, j, d", [(3, 3, 4.0), (5, 2, 10.0), (8, 1, 6.0), (2, 1, 45.0)])
def test_the_value_of_a_stopped_call_is_the_ex_dividend_spot(m, j, d):
    """A call with strike 0.001 that a table stops at step m, a dividend d on
    step j <= m: log(value / DF_END_m + strike) is the host's own running x_m
    with the dividend, and differs from the x_m without it by log(1 - d / s_j),
    s_j the cum-dividend spot (x - ln 2 below 2 d), to rounding."""
    strike = 1e-3
    c = ldc.contract("none", "call", ldc.T8, (), range(8), {j - 1: d}, strike=strike)
    pol = ExercisePolicy.never(8)
    pol.x_lo[m - 1], pol.x_hi[m - 1] = -math.inf, math.inf
    anti, seed, sid = True, 5, 3
    h = mc_american.host_policy_subruns(c, pol, range(1), anti, seed, sid, PATH)
    assert np.all(h["stop_step"] == m)
    Z = mc_american._path_normals(8, seed, 2 * sid + 1, 0, anti)
    pre, post = ldc.stored_walk(c, Z)
    plain = np.full(Z.shape[0], float(np.log(c.params[capi.LSM_P_SPOT])))
    for i in range(m):
        plain = plain + (c.step[i, capi.LSM_S_DRIFT] + c.step[i, capi.LSM_S_DIFF] * Z[:, i])
    x_val = np.log(h["values"][0] / c.step[m - 1, capi.LSM_S_DF_END] + strike)
    assert np.max(np.abs(x_val - post[m - 1])) <= 1e-13
    s_j = np.exp(pre[j - 1])
    shift = np.where(s_j >= 2.0 * d, np.log1p(-np.minimum(d / s_j, 0.5)), -LN2)
    assert np.max(np.abs((x_val - plain) - shift)) <= 1e-12
    assert np.all(x_val < plain)
    if d == 45.0:
        assert 0.05 < np.mean(s_j < 2.0 * d) < 0.5


# ---------------------------------------------------------------------------
# 6. from_critical_spots on an American two-step dividend date
# ---------------------------------------------------------------------------
def _american(dividends, mode):
    return mc_american.plan_american_contract(
        spot=100.0, strike=95.0, vol=0.3, option_type="call", discount_rate=0.05,
        carry_rate=0.03, time_to_expiry=0.5, n_exercise=4, dividends=dividends,
        cash_dividends=mode)


def test_from_critical_spots_addresses_the_cum_and_the_ex_dividend_step():
    c = _american([(0.2, 3.0)], PATH)
    assert list(np.round(c.times, 12)) == [0.125, 0.2, 0.2, 0.25, 0.375, 0.5]
    assert c.div_row()[2] == 3.0 and c.div_row()[1] == 0.0
    spots = {0.125: (99.0, 101.0), 0.2: {"cum": (97.0, 98.0), "ex": None}, 0.25: None,
             0.375: (96.0, 97.0)}
    pol = ExercisePolicy.from_critical_spots(c, spots)
    mid = lambda a, b: 0.5 * (math.log(a) + math.log(b))  # noqa: E731
    assert pol.x_lo[0] == mid(99.0, 101.0) and pol.x_hi[0] == math.inf
    assert pol.x_lo[1] == mid(97.0, 98.0) and pol.x_hi[1] == math.inf   # cum-dividend
    assert pol.x_lo[2] == math.inf and pol.x_hi[2] == -math.inf         # ex-dividend: never
    assert pol.x_lo[3] == math.inf and pol.x_lo[4] == mid(96.0, 97.0)
    both = ExercisePolicy.from_critical_spots(
        c, {**spots, 0.2: {"cum": None, "ex": (94.0, 95.0)}})
    assert both.x_lo[1] == math.inf and both.x_lo[2] == mid(94.0, 95.0)
    # the policy runs
    r = mc_american.price_policy_mc_bounds(c, pol, n_subruns=2, n_outer=1, n_inner=512,
                                           engine="host", cash_dividends=PATH)
    assert r["gap"] >= 0.0 and r["exercised"] > 0


def test_from_critical_spots_refuses_a_plain_pair_on_a_two_step_date():
    c = _american([(0.2, 3.0)], PATH)
    spots = {0.125: None, 0.2: (97.0, 98.0), 0.25: None, 0.375: None}
    with pytest.raises(ValueError, match=r"0\.2.*cum"):
        ExercisePolicy.from_critical_spots(c, spots)
    with pytest.raises(ValueError, match=r"0\.2.*cum"):
        ExercisePolicy.from_critical_spots(c, {**spots, 0.2: None})
    with pytest.raises(ValueError, match="cum"):
        ExercisePolicy.from_critical_spots(c, {**spots, 0.2: {"cum": None}})
    with pytest.raises(ValueError, match="no entry"):
        ExercisePolicy.from_critical_spots(c, {0.125: None, 0.25: None, 0.375: None})
    with pytest.raises(ValueError, match="one step"):
        ExercisePolicy.from_critical_spots(
            c, {**spots, 0.2: {"cum": None, "ex": None}, 0.25: {"cum": None, "ex": None}})


def test_from_critical_spots_without_such_a_pair_gives_the_table_of_before():
    c = _american([], "refuse")
    spots = {0.125: (99.0, 101.0), 0.25: None, 0.375: (0.0, 97.0)}
    pol = ExercisePolicy.from_critical_spots(c, spots)
    want_lo = [0.5 * (math.log(99.0) + math.log(101.0)), math.inf, -math.inf, math.inf]
    assert list(pol.x_lo) == want_lo and list(pol.x_hi) == [math.inf, -math.inf, math.inf,
                                                            -math.inf]
    with pytest.raises(ValueError, match="no entry"):
        ExercisePolicy.from_critical_spots(c, {0.125: None, 0.25: None})
    with pytest.raises(ValueError, match="not one step"):
        ExercisePolicy.from_critical_spots(c, {**spots, 0.3: None})
    # a Bermudan dividend date is one step and takes a plain pair
    b = mc_american.plan_american_contract(
        spot=100.0, strike=95.0, vol=0.3, option_type="call", discount_rate=0.05,
        carry_rate=0.03, time_to_expiry=0.5, exercise_times=[0.2, 0.4], dividends=[(0.2, 3.0)],
        cash_dividends=PATH)
    pol = ExercisePolicy.from_critical_spots(b, {0.2: (97.0, 98.0), 0.4: None})
    assert pol.n_steps == 3 and pol.x_hi[0] == math.inf


# ---------------------------------------------------------------------------
# 7. the C entries validate div (before any device is touched)
# ---------------------------------------------------------------------------
def _raw(which, entry, div):
    """One of the six div entries straight through ctypes with one valid
    three-step contract and the dividend row `div` (None: NULL)."""
    try:
        L = capi.lib()
    except (OSError, capi.FdcnError) as e:  # pragma: no cover
        pytest.skip(f"libfdcn.so is not built: {e}")
    c, pol, coef, _ = _small()
    P, F, S = mc_american._stack([c], [0])
    T = pol.table()[None].copy()
    C = np.ascontiguousarray(coef[None])
    D = None if div is None else np.ascontiguousarray(div, dtype=np.float64)[None].copy()
    stats = np.empty((1, 8))
    dp = None if D is None else D.ctypes.data
    arrays = (P.ctypes.data, F.ctypes.data, S.ctypes.data, dp)
    dev = entry == "dev"
    if which == "lower":
        args = (1, 3, 1, 0) + arrays + (T.ctypes.data, 7, 0, stats.ctypes.data, None)
        fn = L.fdcn_mc_policy_div_batch_dev if dev else L.fdcn_mc_policy_div_batch
    else:
        rule = T if which == "table_dual" else C
        args = (1, 3, 1, 0, 1, 256) + arrays + (rule.ctypes.data, 7, 0, stats.ctypes.data, None,
                                                None)
        fn = {("table_dual", False): L.fdcn_mc_policy_dual_div_batch,
              ("table_dual", True): L.fdcn_mc_policy_dual_div_batch_dev,
              ("fit_dual", False): L.fdcn_mc_lsm_dual_div_batch,
              ("fit_dual", True): L.fdcn_mc_lsm_dual_div_batch_dev}[(which, dev)]
    rc = fn(*args, None, 0, None) if dev else fn(*args)
    return rc, L.fdcn_last_error().decode()


WHO = {"lower": "mc_policy_div_batch", "table_dual": "mc_policy_dual_div_batch",
       "fit_dual": "mc_lsm_dual_div_batch"}


@pytest.mark.parametrize("which", list(WHO))
def test_c_entries_validate_div(which):
    for entry in ("host", "dev"):
        rc, msg = _raw(which, entry, None)
        who = WHO[which] + ("_dev" if entry == "dev" else "")
        assert rc == -1 and msg == f"{who}: div is NULL", (rc, msg)
    for div, word in (([0.0, -1.0, 0.0], "the dividend of step 2 is negative"),
                      ([0.0, 0.0, math.nan], "the dividend of step 3 is not finite"),
                      ([math.inf, 0.0, 0.0], "the dividend of step 1 is not finite")):
        rc, msg = _raw(which, "host", div)
        assert rc == -1 and msg == f"{WHO[which]}: contract 0: {word}", (rc, msg)


# ---------------------------------------------------------------------------
# 8. end to end on the oracle engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def end_to_end():
    eng = oracle_engine()
    cfg = mc_american.LsmConfig(n_subruns=bdc.END_G, antithetic=True, seed=bdc.END_SEED)
    dual = mc_american.DualConfig(bdc.END_OUTER, bdc.END_INNER)
    out = {}
    for name in ("weekly_230", "cum_200"):
        fd, grid, c, pol = bdc.trade_case(name, eng)
        r = mc_american.mc_policy_bounds_batch([c], [pol], cfg, dual, engine="host",
                                               cash_dividends=PATH)[0]
        out[name] = (fd, grid, c, pol, r)
        print(f"{name}: FD(400) {fd:.6f} grid {grid:.2e}; lower {r['price']:.6f} +- "
              f"{r['stderr']:.6f}, gap {r['gap']:.6f} +- {r['gap_stderr']:.6f}, upper "
              f"{r['upper']:.6f}, width / FD {r['gap'] / fd:.3e}, exercised {r['exercised']}")
    return out


@pytest.mark.parametrize("name", ["weekly_230", "cum_200"])
def test_table_bounds_bracket_the_fd_price_of_a_dividend_bermudan(end_to_end, name):
    """policy_from_pricer and mc_policy_bounds_batch with cash_dividends="path"
    at FD 400 x 400, G = 256, n_outer = 2, n_inner = 512, antithetic, seed 42,
    z = 5, grid_error = |fd(400) - fd(200)| (section 13.4's), no percentage.

    Host engine: weekly_230 FD 6.387138 (grid 5.4e-3), lower 6.385454 +- 0.007588,
    gap 0.000123 +- 0.000083, upper 6.385578, width / FD 1.9e-5; cum_200 FD
    29.998390 (grid 6.3e-4), lower 29.997671 +- 0.000775, gap 0 exactly (every
    outer path stops at its first positive candidate, the day before the
    dividend, or never has one), upper 29.997671."""
    fd, grid, c, pol, r = end_to_end[name]
    assert c.has_dividends and r["exercised"] > 0
    assert mc_american.brackets(r, fd, grid_error=grid, z=5.0), (fd, grid, r)


def test_the_policy_exercises_ahead_of_the_dividend(end_to_end):
    """(b): the lower bound minus 5 s.e. exceeds the FD price of the same trade
    with maturity as its only exercise date."""
    fd, grid, c, pol, r = end_to_end["cum_200"]
    european = bdc.trade("cum_200_european", oracle_engine(), 400).price_log()
    print(f"cum_200: lower - 5 s.e. {r['price'] - 5.0 * r['stderr']:.6f}, exercised at "
          f"maturity only {european:.6f}, FD {fd:.6f}")
    assert r["price"] - 5.0 * r["stderr"] > european
    # the step before the dividend date carries a finite threshold
    i = int(np.nonzero(c.div_row())[0][0])
    assert c.step[i - 1, capi.LSM_S_EXERCISE] != 0.0 and math.isfinite(pol.x_lo[i - 1])


def test_fitted_bounds_of_trade_a_bracket_too(end_to_end):
    """(a) through mc_american_bounds_batch (fitted policy); its width beside
    the table policy's is recorded in DESIGN section 13.5."""
    fd, grid, c, pol, table = end_to_end["weekly_230"]
    cfg = mc_american.LsmConfig(n_subruns=bdc.END_G, antithetic=True, seed=bdc.END_SEED)
    r = mc_american.mc_american_bounds_batch(
        [c], cfg, mc_american.DualConfig(bdc.END_OUTER, bdc.END_INNER), engine="host",
        cash_dividends=PATH)[0]
    print(f"weekly_230 fitted: lower {r['price']:.6f} +- {r['stderr']:.6f}, gap {r['gap']:.6f} "
          f"+- {r['gap_stderr']:.6f}, width / FD {r['gap'] / fd:.3e} (table "
          f"{table['gap'] / fd:.3e})")
    assert mc_american.brackets(r, fd, grid_error=grid, z=5.0)
