"""The two Monte Carlo host engines (bgk_barrier.host_paths,
mc_barrier.host_payoffs) on steered paths: normals solved for so that spots
land in the smoothed bands, on the band edges, next to the exact-mode levels,
on the spot floor and on either side of a threshold across a dividend
(tests/steered_paths.py; fixtures by tests/golden/make_golden_steered.py).

1. census: the fixtures' rows reach every branch of monitor() / terminal() /
   advance() -- conditions on the inputs, recounted under the host arithmetic;
2. steering accuracy;
3. host engines against the reference's recorded per-path values, bit for bit;
4. host engines against the two path functionals restated in mpmath at 50
   digits from their documented forms (include/fdcn.h), on the fp64 inputs.
"""
import functools

import mpmath as mp
import numpy as np
import pytest

import bgk_fixture
import mc_fixture
import steered_paths as sp
from finite_difference_amd import bgk_barrier, capi, mc_barrier

CASES = sp.load_cases()
ARRAYS = sp.load_arrays()
TRADES = CASES["bgk"]["trades"]
SMOOTH = [t for t in TRADES if t["menu"] == "smooth"]
MC_CASES = CASES["mc"]["cases"]
LEVELS = CASES["levels"]
U = 2.0 ** -53
mp.mp.dps = 50


@functools.lru_cache(maxsize=None)
def _plan(name):
    t = next(t for t in TRADES if t["name"] == name)
    p = bgk_barrier.DiscreteBarrierBGKPricer(engine="host", **bgk_fixture.kwargs_for(t["inputs"]))
    return p._job().plan


def _z(trade, plan):
    Z = ARRAYS[trade["normals"]]
    return np.concatenate([Z, -Z], axis=0) if plan.antithetic else Z


@functools.lru_cache(maxsize=None)
def _contract(name):
    c = next(c for c in MC_CASES if c["name"] == name)
    return mc_barrier.plan_contract(**mc_fixture.kwargs_for(c["inputs"], mc_barrier))


def _bgk_rows(plan, menu):
    monitor = plan.step[:, capi.BGK_S_MONITOR]
    Hu, Hd, K = LEVELS["upper"], LEVELS["lower"], LEVELS["strike"]
    rows = []
    for put in (False, True):
        if menu == "smooth":
            rows += sp.bgk_menu(Hu, Hd, K, plan.params[capi.BGK_P_EPS_BARRIER],
                                plan.params[capi.BGK_P_EPS_PAYOFF], monitor, put)
        else:
            rows += sp.exact_menu([("up", Hu, 1.0), ("down", Hd, -1.0)], K, monitor, put)
    return rows


def _mc_rows(case, c):
    if case["menu"] != "exact":
        return sp.mc_extras_menu(c, case["menu"])
    sg = -1.0 if int(c.flags[capi.MC_F_KIND]) in (1, 3) else 1.0
    return sp.exact_menu([("thr", float(c.params[capi.MC_P_THRESHOLD]), sg)],
                         float(c.params[capi.MC_P_STRIKE]), c.step[:, capi.MC_S_MONITOR],
                         bool(c.flags[capi.MC_F_PUT]), mid=230.0)


# ---------------------------------------------------------------------------
# 1. census
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("trade", SMOOTH, ids=lambda t: t["name"])
def test_census_of_the_smoothed_trades(trade):
    """At least 4 monitored spots below, inside (the f = +-1 rows left out)
    and above each active band; at least 4 paths with alive = 1, 0 < alive < 1,
    alive = 0 from a breach sum in (1, 2), and a payoff argument below, inside
    and above its band; with a rebate at hit at least 2 paths in each case of
    `newly`."""
    plan = _plan(trade["name"])
    c = sp.bgk_census(plan, _z(trade, plan))
    assert c == trade["census"]
    sides = int(plan.flags[capi.BGK_F_SIDES])
    for bit, side in ((1, "up"), (2, "down")):
        assert (side in c) == bool(sides & bit)
        if side in c:
            assert min(c[side].values()) >= 4, (side, c[side])
    for k in ("alive_1", "alive_frac", "alive_0_clamped", "payoff_below", "payoff_inside",
              "payoff_above"):
        assert c[k] >= 4, (k, c[k])
    if plan.rebate_mode == 2:
        assert min(c["newly"].values()) >= 2, c["newly"]


def test_the_trades_cover_sides_rebates_and_types():
    seen = {(int(_plan(t["name"]).flags[capi.BGK_F_SIDES]), _plan(t["name"]).rebate_mode,
             int(_plan(t["name"]).flags[capi.BGK_F_PUT])) for t in SMOOTH}
    assert seen >= {(s, m, p) for s in (1, 2, 3) for m in (0, 1, 2) for p in (0, 1)}
    exact = [t for t in TRADES if t["menu"] == "exact"]
    assert {(int(_plan(t["name"]).flags[capi.BGK_F_SIDES]),
             int(_plan(t["name"]).flags[capi.BGK_F_PUT])) for t in exact} \
        == {(s, p) for s in (1, 2, 3) for p in (0, 1)}
    assert all(_plan(t["name"]).params[capi.BGK_P_EPS_BARRIER] == 0.0 for t in exact)
    anti = [_plan(t["name"]).antithetic for t in TRADES]
    assert 0 < sum(anti) < len(anti)


def test_census_of_the_single_barrier_cases():
    """At least 2 paths with the floor active, with the floor inactive on a
    dividend step, with a decision the jump order changes, and with a second
    breach after a return inside."""
    total = dict(floor_active=0, floor_inactive=0, order_changes=0, rebreach=0)
    for case in MC_CASES:
        census = sp.mc_census(_contract(case["name"]), ARRAYS[case["normals"]])
        assert census == case["census"], case["name"]
        for k in total:
            total[k] += census[k]
    assert min(total.values()) >= 2, total
    kinds = {(int(_contract(c["name"]).flags[capi.MC_F_KIND]),
              int(_contract(c["name"]).flags[capi.MC_F_DIV_FIRST]))
             for c in MC_CASES if c["menu"] == "straddle"}
    assert kinds == {(k, f) for k in (1, 2, 3, 4) for f in (0, 1)}
    floors = [c for c in MC_CASES if c["menu"] == "floor"]
    assert {int(_contract(c["name"]).flags[capi.MC_F_DIV_FIRST]) for c in floors} == {0, 1}
    for c in floors:
        census = c["census"]
        assert census["floor_active"] >= 2 and census["floor_inactive"] >= 2


def test_exact_decisions_sit_off_their_edges():
    for t in TRADES:
        plan = _plan(t["name"])
        assert sp.bgk_edge_gap(plan, _z(t, plan)) > sp.EDGE, t["name"]
    for case in MC_CASES:
        c = _contract(case["name"])
        Z = ARRAYS[case["normals"]]
        Zf = np.concatenate([Z, -Z]) if case["inputs"]["cfg"]["antithetic"] else Z
        assert sp.mc_edge_gap(c, Zf) > sp.EDGE, case["name"]


# ---------------------------------------------------------------------------
# 2. steering accuracy
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("menu", ["smooth", "exact"])
def test_steered_rows_land_on_their_targets(menu):
    """|landing - target| <= 1e-11 * target on every steered step, both for
    the fixture's normals and for rows steered afresh: 1e5 below the smallest
    band half-width."""
    trade = next(t for t in TRADES if t["menu"] == menu)
    plan = _plan(trade["name"])
    grid = (float(plan.params[capi.BGK_P_LOG_SPOT]), plan.step[:, capi.BGK_S_DRIFT],
            plan.step[:, capi.BGK_S_DIFF])
    rows = _bgk_rows(plan, menu)
    assert [f"{lb} [{tag}]" for tag, part in (("call", rows[:len(rows) // 2]),
                                              ("put", rows[len(rows) // 2:]))
            for lb, _ in part] == CASES["bgk"]["labels"][menu]
    for Z in (ARRAYS[trade["normals"]], sp.steer_rows(*grid, rows)):
        assert Z.shape == (len(rows), plan.n_steps)
        spots = sp.landing(*grid, Z)
        worst = max(abs(spots[r, k] - t) / t for r, k, t in sp.targets_of(rows))
        print(f"{menu}: worst landing error {worst:.2e} relative")
        assert worst <= 1e-11


@pytest.mark.parametrize("case", MC_CASES, ids=lambda c: c["name"])
def test_steered_single_barrier_rows_land_on_their_targets(case):
    c = _contract(case["name"])
    rows = _mc_rows(case, c)
    assert [lb for lb, _ in rows] == case["labels"]
    for Z in (ARRAYS[case["normals"]], sp.steer_mc_rows(c, rows)):
        pre = sp.mc_walk(c, Z)[0]
        worst = max(abs(pre[r, k] - t) / t for r, k, t in sp.targets_of(rows))
        assert worst <= 1e-11


# ---------------------------------------------------------------------------
# 3. host engines against the reference's recorded values
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("trade", TRADES, ids=lambda t: t["name"])
def test_host_paths_reproduce_the_reference(trade):
    plan = _plan(trade["name"])
    x, rebate, _ = bgk_barrier.host_paths(plan, _z(trade, plan))
    assert x.shape == (trade["n_sim"],)
    assert np.array_equal(x, ARRAYS["x_" + trade["name"]])
    if plan.rebate_mode == 2:
        assert np.array_equal(rebate, ARRAYS["rebate_" + trade["name"]])
    else:
        assert not rebate.any()


@pytest.mark.parametrize("case", MC_CASES, ids=lambda c: c["name"])
def test_host_payoffs_reproduce_the_reference(case):
    c = _contract(case["name"])
    assert np.array_equal(c.step, np.array(case["step"]))
    assert np.array_equal(c.params, np.array(case["params"]))
    Z = ARRAYS[case["normals"]]
    got = mc_barrier._host_observations(c, Z, case["inputs"]["cfg"]["antithetic"])
    assert np.array_equal(got, ARRAYS[case["payoffs"]])


# ---------------------------------------------------------------------------
# 4. host engines against mpmath restatements
# ---------------------------------------------------------------------------
_MP_SPOTS = {}


def _mp_spots(log_s0, drift, diff, Z):
    """exp(log_s0 + sum_j (drift_j + diff_j z_j)) at every step's end, exact
    on the fp64 inputs to 50 digits.  Rows are cached: the trades share two
    sets of normals."""
    out = []
    for row in Z:
        key = (log_s0, drift.tobytes(), diff.tobytes(), row.tobytes())
        if key not in _MP_SPOTS:
            c, spots = mp.mpf(0), []
            for k in range(len(row)):
                c += mp.mpf(float(drift[k])) + mp.mpf(float(diff[k])) * mp.mpf(float(row[k]))
                spots.append(mp.exp(mp.mpf(log_s0) + c))
            _MP_SPOTS[key] = spots
        out.append(_MP_SPOTS[key])
    return out


def mp_bgk_paths(params, flags, step, Z):
    """x, rebate_pv, alive and the per-monitor hit pattern of every row, from
    the path description of fdcn_mc_bgk_batch in include/fdcn.h."""
    log_s0, K, Hu, Hd, eb, ep, R = (mp.mpf(float(v)) for v in params)
    put, sides, mode = int(flags[0]), int(flags[1]), int(flags[2])
    half = mp.mpf(1) / 2
    spots = _mp_spots(float(params[0]), step[:, 0].copy(), step[:, 1].copy(), Z)
    xs, rebates, alives, patterns = [], [], [], []
    for s_row in spots:
        breached, rebate_pv, pattern = mp.mpf(0), mp.mpf(0), []
        for k in range(step.shape[0]):
            if step[k, 2] == 0.0 or sides == 0:
                continue
            s, df_k = s_row[k], mp.mpf(float(step[k, 3]))
            event = mp.mpf(0)
            if eb > 0:
                if sides & 1:
                    up = 0 if s < Hu - eb else (1 if s > Hu + eb else half + (s - Hu) / (2 * eb))
                    event = max(event, up)
                if sides & 2:
                    dn = 1 if s < Hd - eb else (0 if s > Hd + eb else half + (Hd - s) / (2 * eb))
                    event = max(event, dn)
                if mode == 2:
                    newly = max(mp.mpf(0), event - (1 if rebate_pv > 0 else 0))
                    rebate_pv += newly * R * df_k
            else:
                hit = bool((sides & 1) and s >= Hu) or bool((sides & 2) and s <= Hd)
                event = mp.mpf(1 if hit else 0)
                if mode == 2 and hit and breached == 0:
                    rebate_pv = R * df_k
            pattern.append(event == 1)
            breached += event
        alive = min(max(1 - breached, mp.mpf(0)), mp.mpf(1))
        d = K - s_row[-1] if put else s_row[-1] - K
        if ep > 0:
            intrinsic = 0 if d < -ep else (d if d > ep else
                                           (half * d * d + ep * d + half * ep * ep) / (2 * ep))
        else:
            intrinsic = max(d, mp.mpf(0))
        x = alive * intrinsic
        if mode == 1:
            x += R * (1 - alive)
        xs.append(x)
        rebates.append(rebate_pv)
        alives.append(alive)
        patterns.append(pattern)
    return xs, rebates, alives, patterns


def host_bounds(plan, Z):
    """Per-path bounds of |host - exact| for x and rebate_pv.

    The host forms y_k = fl(log_s0 + c_k) with c_k a running sum that takes
    three roundings a step (the product diff z, the sum drift + diff z, the
    accumulation), each at most 2^-53 relative to a result no larger than
    L = max(|y|, |c|, |increment|) over the path: |dy| <= (3 n_steps + 1) 2^-53 L.
    One exp follows, within 1 ulp = 2^-52 relative.  So a spot S differs from
    the exact one on the same fp64 inputs by at most

        e_S = 2^-53 * S_max * ((3 n_steps + 1) L + 2)

    with S_max the path's largest spot.  This replaces the unit 2^-51 * S of
    bgk_fixture.path_bounds, whose argument then carries over with its factor
    4 (which also covers the few 2^-53-relative roundings of the functional
    itself): inside a band of half-width e_b one monitor's breach amount moves
    by e_S / (2 e_b) and alive by at most n_mon times that; intrinsic has slope
    at most 1:

        |dx|         <= 4 e_S (1 + n_mon intrinsic / (2 e_b))
                        (+ 4 e_S n_mon R / (2 e_b) with a rebate at expiry,
                        the R (1 - alive) term)
        |drebate_pv| <= 4 e_S n_mon R / (2 e_b).

    For e_b = 0 no decision may differ (asserted apart): |dx| <= 4 e_S and
    rebate_pv = fl(R DF) is one rounding, 2^-53 R."""
    P, S = plan.params, plan.step
    log_s0 = float(P[capi.BGK_P_LOG_SPOT])
    dz = S[:, capi.BGK_S_DIFF][None, :] * Z
    inc = S[:, capi.BGK_S_DRIFT][None, :] + dz
    c = np.cumsum(inc, axis=1)
    y = log_s0 + c
    L = np.max(np.abs(np.concatenate([y, c, inc, dz], axis=1)), axis=1)
    spots = np.exp(y)
    e_s = U * spots.max(axis=1) * ((3 * plan.n_steps + 1) * L + 2.0)
    d = spots[:, -1] - P[capi.BGK_P_STRIKE]
    d = -d if plan.flags[capi.BGK_F_PUT] else d
    ep, eb = float(P[capi.BGK_P_EPS_PAYOFF]), float(P[capi.BGK_P_EPS_BARRIER])
    R = float(P[capi.BGK_P_REBATE])
    intrinsic = bgk_barrier.smooth_relu(d, eps=ep) if ep > 0.0 else np.maximum(d, 0.0)
    if eb == 0.0:
        return 4.0 * e_s, np.full(Z.shape[0], U * R)
    n_mon = int(np.count_nonzero(S[:, capi.BGK_S_MONITOR]))
    bound_r = 4.0 * e_s * n_mon * R / (2.0 * eb)
    bound_x = 4.0 * e_s * (1.0 + n_mon * intrinsic / (2.0 * eb))
    if plan.rebate_mode == 1:
        bound_x = bound_x + bound_r
    return bound_x, bound_r


@pytest.mark.parametrize("trade", TRADES, ids=lambda t: t["name"])
def test_host_paths_against_extended_precision(trade):
    plan = _plan(trade["name"])
    Z = _z(trade, plan)
    x, rebate, alive = bgk_barrier.host_paths(plan, Z)
    mx, mr, ma, patterns = mp_bgk_paths(plan.params, plan.flags, plan.step, Z)
    bound_x, bound_r = host_bounds(plan, Z)
    err_x = np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(x, mx)])
    err_r = np.array([float(abs(mp.mpf(float(a)) - b)) for a, b in zip(rebate, mr)])
    labels = CASES["bgk"]["labels"][trade["menu"]]
    labels = labels + ["mirror of " + lb for lb in labels] if plan.antithetic else labels
    for group in sorted({sp.group_of(lb) for lb in labels}):
        rows = [i for i, lb in enumerate(labels) if sp.group_of(lb) == group]
        print(f"{trade['name']} {group}: worst x error / bound "
              f"{np.max(err_x[rows] / bound_x[rows]):.2e}")
    assert np.all(err_x <= bound_x), np.max(err_x / bound_x)
    assert np.all(err_r <= bound_r), np.max(err_r - bound_r)
    if plan.params[capi.BGK_P_EPS_BARRIER] == 0.0:
        # exact mode: every decision is the extended-precision one
        spots = sp.landing(plan.params[0], plan.step[:, 0], plan.step[:, 1], Z)
        sides = int(plan.flags[capi.BGK_F_SIDES])
        mon = np.nonzero(plan.step[:, capi.BGK_S_MONITOR])[0]
        hit = np.zeros((Z.shape[0], len(mon)), bool)
        if sides & 1:
            hit |= spots[:, mon] >= plan.params[capi.BGK_P_UPPER]
        if sides & 2:
            hit |= spots[:, mon] <= plan.params[capi.BGK_P_LOWER]
        assert hit.tolist() == patterns
        assert alive.tolist() == [float(a) for a in ma]
        assert np.array_equal(rebate > 0.0, np.array([r > 0 for r in mr]))


def mp_mc_payoff(params, flags, step, z):
    """One path's discounted payoff and its per-step breach pattern, from the
    path description of fdcn_mc_barrier_batch in include/fdcn.h."""
    spot, strike, df_T, thr, rebate, floor = (mp.mpf(float(v)) for v in params)
    put, kind, at_hit, div_first = (int(flags[k]) for k in range(4))
    s, untouched, hit_df, pattern = spot, True, df_T, []
    for i in range(step.shape[0]):
        drift, diff, div, monitor, df_end = (mp.mpf(float(v)) for v in step[i])
        s = s * mp.exp(drift + diff * mp.mpf(float(z[i])))
        if div_first and div != 0:
            s = max(s - div, floor)
        if kind != 0 and monitor != 0:
            breached = s <= thr if kind in (1, 3) else s >= thr
            pattern.append(bool(breached))
            if breached and untouched:
                hit_df, untouched = df_end, False
        if not div_first and div != 0:
            s = max(s - div, floor)
    vanilla = max(strike - s, mp.mpf(0)) if put else max(s - strike, mp.mpf(0))
    pv = df_T * vanilla
    if kind == 0:
        return pv, pattern
    if kind <= 2:
        return (pv if untouched else rebate * (hit_df if at_hit else df_T)), pattern
    return (mp.mpf(0) if untouched else pv), pattern


@pytest.mark.parametrize("case", MC_CASES, ids=lambda c: c["name"])
def test_host_payoffs_against_extended_precision(case):
    """A step multiplies s by exp(fl(drift + fl(diff z))): the argument is off
    by at most 2 * 2^-53 * A with A = max(|diff z|, |argument|) <= 1/2 here
    (asserted), the exp by 2^-52 relative, the product by 2^-53: 4 * 2^-53
    relative a step.  A dividend's subtraction adds one rounding and max(.,
    floor) none, and neither enlarges an absolute error.  With the payoff's
    slope at most 1 and two roundings in df * vanilla (or one in R * DF):

        |dp| <= 4 * 2^-53 * (4 n_steps + n_div + 2) * max(S_max, |p|),

    the factor 4 as in bgk_fixture.path_bounds; an antithetic observation is
    the mean of two such paths.  Every breach decision is the
    extended-precision one."""
    c = _contract(case["name"])
    Z = ARRAYS[case["normals"]]
    anti = case["inputs"]["cfg"]["antithetic"]
    got = mc_barrier._host_observations(c, Z, anti)
    n_div = int(np.count_nonzero(c.step[:, capi.MC_S_DIV]))
    mon = c.step[:, capi.MC_S_MONITOR] != 0.0
    thr, kind = float(c.params[capi.MC_P_THRESHOLD]), int(c.flags[capi.MC_F_KIND])
    worst = 0.0
    for sign in ((1.0, -1.0) if anti else (1.0,)):
        arg = c.step[:, capi.MC_S_DRIFT][None, :] + c.step[:, capi.MC_S_DIFF][None, :] * (sign * Z)
        assert np.max(np.abs(arg)) <= 0.5
    for i in range(Z.shape[0]):
        want, s_max = mp.mpf(0), 0.0
        for sign in ((1.0, -1.0) if anti else (1.0,)):
            p, pattern = mp_mc_payoff(c.params, c.flags, c.step, sign * Z[i])
            pre, tested, _, _ = sp.mc_walk(c, sign * Z[i:i + 1])
            if kind != 0:
                t = tested[0, mon]
                assert (t <= thr if kind in (1, 3) else t >= thr).tolist() == pattern
            want += p
            s_max = max(s_max, float(pre.max()), float(abs(p)))
        want = want / 2 if anti else want
        bound = 4.0 * U * (4 * c.n_steps + n_div + 2) * s_max
        err = float(abs(mp.mpf(float(got[i])) - want))
        worst = max(worst, err / bound)
        assert err <= bound, (case["labels"][i], err, bound)
    print(f"{case['name']}: worst error / bound {worst:.2e}")
