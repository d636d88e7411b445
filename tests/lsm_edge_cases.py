"""The edge-case menu of the least-squares Monte Carlo tests
(test_lsm_edges_host.py, test_gpu_lsm_edges.py), the bounds of DESIGN.md
section 13.1, and the builder of the fixture (golden/make_golden_lsm_edges.py
-> golden/lsm_edges.json / .npz).

The kernel takes no normals from outside, so the paths are steered through the
contract: a strike or a barrier level placed between two neighbouring order
statistics of the reference's own paths puts exactly 64 (valid) or 63
(invalid) paths into one fit; step-table edits make the normal matrix singular
or badly conditioned; per-step rebates make a wrong hit date visible in the
value.  Everything steered is computed from lsm_reference.py (mpmath), never
from an engine.

build_case(name) -> Case: the contract(s) of one case, each with its stream
id, reference results, fit bounds and exclusions.  The tests read the stored
fixture; build_case is run by the generator, and by the host test for two
small cases (an exact regeneration check).
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import mpmath as mp
import numpy as np

import lsm_reference as lr
from finite_difference_amd import capi
from finite_difference_amd.mc_american import LsmContract, plan_american_contract

EPS = 2.0 ** -52
Z_TOL = 1e-13            # the device normals' bound (test_gpu_mc.py), absolute
MARGIN_FACTOR = 100.0    # every decision: |phi - fit| >= 100 fit_bound(u)
EXCLUSION_CAP = 0.01     # else at most 1 % of the case's decisions are left out
MIN_GAP = 1e-6           # relative gap of the order statistics a level sits between
MAX_STREAM = 256
N = lr.N_PATHS
T_HALF = 0.5
T8 = [T_HALF * k / 8 for k in range(1, 9)]


# ---------------------------------------------------------------------------
# contracts
# ---------------------------------------------------------------------------
def contract(kind="none", option_type="put", times=T8, monitor=(), exercise=None, *,
             strike=100.0, spot=100.0, lower=88.0, upper=113.0, rebate=0.0, at_hit=False,
             rate=0.05, carry=0.03, vol=0.3):
    """plan_american_contract on the grid `times`, then the MONITOR / EXERCISE
    flags written into the step table by row index (lsm_fixture.plan_batch)."""
    t = [float(v) for v in times]
    rows = range(len(t)) if exercise is None else exercise
    c = plan_american_contract(
        spot=spot, strike=strike, vol=vol, option_type=option_type, discount_rate=rate,
        carry_rate=carry, time_to_expiry=t[-1], barrier_type=kind,
        lower_barrier=lower if ("down" in kind or "double" in kind) else None,
        upper_barrier=upper if ("up" in kind or "double" in kind) else None,
        monitor_times=[t[i] for i in monitor], rebate_amount=rebate, rebate_at_hit=at_hit,
        exercise_times=t)
    assert c.n_steps == len(t)
    c.step[:, capi.LSM_S_EXERCISE] = 0.0
    c.step[list(rows), capi.LSM_S_EXERCISE] = 1.0
    return c


def clone(c, *, strike=None, lower=None, upper=None):
    out = LsmContract(params=c.params.copy(), flags=c.flags.copy(), step=c.step.copy(),
                      times=c.times.copy(), barrier_type=c.barrier_type)
    for k, v in ((capi.LSM_P_STRIKE, strike), (capi.LSM_P_LOWER, lower),
                 (capi.LSM_P_UPPER, upper)):
        if v is not None:
            out.params[k] = v
    return out


def float_walk(c, subrun, antithetic, seed, word, obs_first=0):
    """x [N, M] of one path set in float64 (x_0 + the running sum): where the
    tests evaluate two cubics at the same regressor, and what the builders
    order paths by.  Not an engine: no event, no fit."""
    per = N // 2 if antithetic else N
    z = lr.subrun_normals(c.n_steps, antithetic, seed, word, obs_first + subrun * per)
    w = c.step[:, capi.LSM_S_DRIFT][None, :] + c.step[:, capi.LSM_S_DIFF][None, :] * z
    return math.log(c.params[capi.LSM_P_SPOT]) + np.cumsum(w, axis=1)


def float_regressor(c, x, m):
    return (x[:, m - 1] - c.step[m - 1, capi.LSM_S_CENTRE]) * c.step[m - 1, capi.LSM_S_ISCALE]


# ---------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------
@dataclass
class FitBound:
    """fit_bound(u) = 2 (sum_k |u|^k dc[k] + |fit'(u)| (du_abs + 3 EPS |u|)
    + 4 EPS sum_k |c[k]| |u|^k), all from reference quantities."""
    c: List[float]
    dc: List[float]
    du_abs: float

    def __call__(self, u):
        a = np.abs(np.asarray(u, dtype=float))
        c, dc = self.c, self.dc
        slope = np.abs(c[1] + u * (2.0 * c[2] + u * 3.0 * c[3]))
        lin = dc[0] + a * (dc[1] + a * (dc[2] + a * dc[3]))
        size = abs(c[0]) + a * (abs(c[1]) + a * (abs(c[2]) + a * abs(c[3])))
        return 2.0 * (lin + slope * (self.du_abs + 3.0 * EPS * a) + 4.0 * EPS * size)


def walk_error(c, z, x, m):
    """Largest |engine x_m - reference x_m| over the paths of a set: log(spot)
    to an ulp, per step the device normal's Z_TOL through DIFF and the two
    roundings of DRIFT + DIFF z, and one rounding of x per add of the forward
    walk (M) and of the backward walk (M - m), each half an EPS of |x|."""
    M = c.n_steps
    S = c.step
    xmax = np.max(np.abs(x), axis=1)
    per_step = (S[:m, capi.LSM_S_DIFF][None, :] * (Z_TOL + 2.0 * EPS * np.abs(z[:, :m]))
                + 2.0 * EPS * np.abs(S[:m, capi.LSM_S_DRIFT])[None, :])
    dx = EPS * abs(math.log(c.params[capi.LSM_P_SPOT])) + per_step.sum(axis=1) + M * EPS * xmax
    return float(dx.max())


def fit_bound(c, ref, m, x64, z):
    """First-order bound on the float64 normal-equation fit's error for the
    valid fit of step m of reference result `ref`."""
    with mp.workdps(lr.DPS):
        M = c.n_steps
        us, ys = ref["fit_u"][m], ref["fit_cf"][m]
        cc = [abs(v) for v in ref["coef"][m - 1]]
        eps = mp.mpf(EPS)
        strike = mp.mpf(float(c.params[capi.LSM_P_STRIKE]))
        iscale = mp.mpf(float(c.step[m - 1, capi.LSM_S_ISCALE]))
        dx = mp.mpf(max(walk_error(c, z, x64, k) for k in range(m, M + 1)))
        df_min = mp.mpf(float(np.prod(c.step[:, capi.LSM_S_DF_STEP].clip(max=1.0))))
        au = [abs(u) for u in us]
        ay = [abs(y) for y in ys]
        du = [iscale * dx + 3 * eps * a for a in au]
        dy = [(y / df_min + strike) * dx + (M + 4) * eps * y for y in ay]
        pw = [[mp.mpf(1), a, a * a, a * a * a, a ** 4, a ** 5, a ** 6] for a in au]
        A = mp.matrix(4, 4)
        mom = [mp.fsum(u ** k for u in us) for k in range(7)]
        for i in range(4):
            for j in range(4):
                A[i, j] = mom[i + j]
        dA = [27 * eps * mp.fsum(r[k] for r in pw)
              + (mp.fsum(k * r[k - 1] * d for r, d in zip(pw, du)) if k else 0)
              for k in range(7)]
        db = [27 * eps * mp.fsum(r[i] * y for r, y in zip(pw, ay))
              + mp.fsum((i * r[i - 1] * y * d if i else 0) + r[i] * e
                        for r, y, d, e in zip(pw, ay, du, dy))
              for i in range(4)]
        rhs = [db[i] + mp.fsum((dA[i + j] + 14 * eps * mp.sqrt(A[i, i] * A[j, j])) * cc[j]
                               for j in range(4)) for i in range(4)]
        inv = mp.inverse(A)
        dc = [mp.fsum(abs(inv[k, i]) * rhs[i] for i in range(4)) for k in range(4)]
        return FitBound(c=[float(v) for v in ref["coef"][m - 1]], dc=[float(v) for v in dc],
                        du_abs=float(iscale * dx))


def stderr_bound(means):
    """Bound on |one-pass stderr - two-pass stderr| of G sub-run means (DESIGN.md
    13.1): s2 - s^2 / n carries an absolute error of at most (G + 3) EPS s2, so
    the computed variance of the mean is off by at most that over n (n - 1);
    through the square root, |sqrt(a) - sqrt(b)| <= sqrt(|a - b|)."""
    G = len(means)
    s2 = sum(float(v) ** 2 for v in means)
    return math.sqrt((G + 3) * EPS * s2 / (G * (G - 1)))


# ---------------------------------------------------------------------------
# one evaluated contract
# ---------------------------------------------------------------------------
@dataclass
class Item:
    """One contract of a case with everything the fixture stores about it."""
    contract: LsmContract
    stream_id: int
    refs: list                      # reference result per sub-run
    bounds: list                    # per sub-run {m: FitBound}
    excluded: list                  # per sub-run bool [N]: price paths left out
    n_decisions: int = 0
    n_low_margin: int = 0           # decisions (both sets) below 100 x their bound
    worst_margin_ratio: float = math.inf  # min |phi - fit| / fit_bound(u)
    note: str = ""


@dataclass
class Case:
    name: str
    n_steps: int
    antithetic: bool
    seed: int
    subruns: List[int]              # sub-run numbers of the run (obs_first = subruns[0])
    items: List[Item] = field(default_factory=list)
    family: str = ""


def evaluate(c, subruns, antithetic, seed, sid):
    """Reference, bounds and margins of contract c at stream id sid."""
    refs, bounds, excluded = [], [], []
    n_dec, n_low, worst = 0, 0, math.inf
    for g in subruns:
        r = lr.reference_subrun(c, g, antithetic, seed, sid)
        x_fit = float_walk(c, g, antithetic, seed, 2 * sid)
        x_price = float_walk(c, g, antithetic, seed, 2 * sid + 1)
        bb, ex = {}, np.zeros(N, dtype=bool)
        for m in r["fit_gap"]:
            bb[m] = fit_bound(c, r, m, x_fit, r["z_fit"])
            u = np.array([float(v) for v in r["fit_u"][m]])
            gap = np.abs(np.array([float(v) for v in r["fit_gap"][m]]))
            ratio = gap / bb[m](u)
            n_dec += len(u)
            n_low += int((ratio < MARGIN_FACTOR).sum())
            worst = min(worst, float(ratio.min()))
        for p, m, u, gap in r["price_decisions"]:
            ratio = abs(float(gap)) / float(bb[m](float(u)))
            n_dec += 1
            worst = min(worst, ratio)
            if ratio < MARGIN_FACTOR:
                n_low += 1
                ex[p] = True
        refs.append(r)
        bounds.append(bb)
        excluded.append(ex)
    return Item(contract=c, stream_id=sid, refs=refs, bounds=bounds, excluded=excluded,
                n_decisions=n_dec, n_low_margin=n_low, worst_margin_ratio=worst)


def search_stream(make, subruns, antithetic, seed, first=0, tries=8, accept=None):
    """The first stream id from `first` on (below MAX_STREAM) at which every
    contract that make(sid) returns (None: this id cannot be steered) has all
    its decisions at least MARGIN_FACTOR bounds from the fit, and `accept`
    holds; failing that within `tries` ids, the one with the fewest
    low-margin decisions, which must stay under EXCLUSION_CAP."""
    best = None
    for sid in range(first, min(MAX_STREAM, first + tries)):
        cs = make(sid)
        if cs is None:
            continue
        items = [evaluate(c, subruns, antithetic, seed, sid) for c in cs]
        if accept is not None and not accept(items):
            continue
        low = sum(i.n_low_margin for i in items)
        if best is None or low < best[0]:
            best = (low, items)
        if low == 0:
            break
    assert best is not None, "no stream id could be steered"
    for it in best[1]:
        assert it.n_low_margin <= EXCLUSION_CAP * max(1, it.n_decisions), \
            (it.n_low_margin, it.n_decisions)
    return best[1]


# ---------------------------------------------------------------------------
# steering through the contract
# ---------------------------------------------------------------------------
def _between(lo, hi):
    """The float64 midway between two neighbouring order statistics, or None
    where they are closer than MIN_GAP relative."""
    lo, hi = float(lo), float(hi)
    if not (hi - lo) >= MIN_GAP * abs(hi):
        return None
    return 0.5 * (lo + hi)


def _fit_spots(c, antithetic, seed, sid, m):
    """Reference s_1 .. s_m of the fit set, [N][m + 1] mpf."""
    with mp.workdps(lr.DPS):
        T = lr._Table(c)
        z = lr.subrun_normals(c.n_steps, antithetic, seed, 2 * sid, 0)
        return lr._PathSet(T, z).s


def strike_pair(c, antithetic, seed, sid, m):
    """(64-path contract, 63-path contract): the strike between order
    statistics of the fit-set spot at step m, counted from the in-the-money
    end."""
    s = sorted(float(row[m]) for row in _fit_spots(c, antithetic, seed, sid, m))
    if c.flags[capi.LSM_F_PUT]:
        k64, k63 = _between(s[63], s[64]), _between(s[62], s[63])
    else:
        k64, k63 = _between(s[-65], s[-64]), _between(s[-64], s[-63])
    if k64 is None or k63 is None:
        return None
    return [clone(c, strike=k64), clone(c, strike=k63)]


def knock_in_pair(c, antithetic, seed, sid, m):
    """Down-and-in put: eligibility (m >= h) thins the fit of step m.  The
    level sits between order statistics of the running minimum over the
    monitored steps up to m, so that exactly 64 / 63 eligible paths are in the
    money at step m."""
    S = _fit_spots(c, antithetic, seed, sid, m)
    strike = float(c.params[capi.LSM_P_STRIKE])
    mon = [j for j in range(1, m + 1) if c.step[j - 1, capi.LSM_S_MONITOR] != 0.0]
    rows = sorted((min(float(r[j]) for j in mon), float(r[m]) < strike) for r in S)
    itm = 0
    for a, (_, inm) in enumerate(rows):
        itm += inm
        if itm == lr.MIN_FIT:
            break
    # level >= running minimum knocks in: above row a takes the 64th, below it 63
    l64, l63 = _between(rows[a][0], rows[a + 1][0]), _between(rows[a - 1][0], rows[a][0])
    if l64 is None or l63 is None or not rows[a][1]:
        return None
    return [clone(c, lower=l64), clone(c, lower=l63)]


def knock_out_pair(c, antithetic, seed, sid, m):
    """Down-and-out put: eligibility (m < h) thins the fit of step m.  Of the
    paths in the money at step m, exactly 64 / 63 have their running minimum
    over the monitored steps up to m above the level."""
    S = _fit_spots(c, antithetic, seed, sid, m)
    strike = float(c.params[capi.LSM_P_STRIKE])
    mon = [j for j in range(1, m + 1) if c.step[j - 1, capi.LSM_S_MONITOR] != 0.0]
    low = sorted((min(float(r[j]) for j in mon) for r in S if float(r[m]) < strike),
                 reverse=True)
    l64, l63 = _between(low[64], low[63]), _between(low[63], low[62])
    if l64 is None or l63 is None:
        return None
    return [clone(c, lower=l64), clone(c, lower=l63)]


# ---------------------------------------------------------------------------
# the menu
# ---------------------------------------------------------------------------
EDGE_STEP = 2        # the exercise step whose fit is steered to 64 / 63 paths
PIVOT_STEP = 4       # the step whose CENTRE is shifted (8-step cases)
SHIFT_SINGULAR = 3.0e7   # (b): d_1 / a_11 = about K^-2 = 1e-15
SHIFTS_ILL = (16.0, 12.0, 8.0, 6.0, 4.0)  # (c): the largest under the exclusion cap
TINY_DIFF = 1e-300   # (a): absorbed by x in float64 (and at 50 digits)
SHARD_FIRST = 5      # the sharded launch starts at this sub-run


def shift_centre(c, m, k):
    """u -> u + k at step m: CENTRE_m moved by k standard deviations."""
    out = clone(c)
    out.step[m - 1, capi.LSM_S_CENTRE] -= k / out.step[m - 1, capi.LSM_S_ISCALE]
    return out


def _count_is(step, n):
    return lambda items: all(it.refs[0]["count"][step - 1] == k for it, k in zip(items, n))


def _minfit(name, option_type, antithetic, seed):
    base = contract("none", option_type)
    items = search_stream(lambda sid: strike_pair(base, antithetic, seed, sid, EDGE_STEP), [0],
                          antithetic, seed, accept=_count_is(EDGE_STEP, (64, 63)))
    return Case(name, 8, antithetic, seed, [0], items, "min_fit")


def _minfit_ki(name):
    base = contract("down-and-in", "put", monitor=range(8), rebate=0.4)
    items = search_stream(lambda sid: knock_in_pair(base, False, 23, sid, EDGE_STEP), [0], False,
                          23, accept=_count_is(EDGE_STEP, (64, 63)))
    return Case(name, 8, False, 23, [0], items, "min_fit")


def _minfit_ko(name):
    base = contract("down-and-out", "put", monitor=(0, 1), rebate=0.3, at_hit=True)
    items = search_stream(lambda sid: knock_out_pair(base, True, 24, sid, EDGE_STEP), [0], True,
                          24, accept=_count_is(EDGE_STEP, (64, 63)))
    return Case(name, 8, True, 24, [0], items, "min_fit")


def _pivot_equal(name):
    """(a) two steps, the first with a DIFF that x absorbs: every path has the
    same x_1 and u_1, d_1 is exactly 0.  Two steps, not eight: the engines
    walk back from maturity, and fl(fl(x_1 + w) - w) returns x_1 for certain
    over one step only (|x_2's rounding| <= half an ulp of x_1; a tie rounds to
    even, and x_1 has an even mantissa, asserted below)."""
    c = contract("none", "put", times=[0.2, 0.5])
    c.step[0, capi.LSM_S_DIFF] = TINY_DIFF
    x1 = math.log(c.params[capi.LSM_P_SPOT]) + c.step[0, capi.LSM_S_DRIFT]
    assert int(np.float64(x1).view(np.uint64)) % 2 == 0
    items = search_stream(lambda sid: [c], [0], False, 31)
    return Case(name, 2, False, 31, [0], items, "pivot")


def _pivot_singular(name):
    c = shift_centre(contract("none", "put"), PIVOT_STEP, SHIFT_SINGULAR)

    def singular(items):
        r = items[0].refs[0]["ratios"][PIVOT_STEP - 1]
        return min(v for v in r if v is not None) <= 1e-14
    items = search_stream(lambda sid: [c], [0], False, 32, accept=singular)
    return Case(name, 8, False, 32, [0], items, "pivot")


def _pivot_ill(name):
    for k in SHIFTS_ILL:
        c = shift_centre(contract("none", "put"), PIVOT_STEP, k)
        try:
            items = search_stream(lambda sid: [c], [0], False, 33, tries=4)
        except AssertionError:
            continue
        if min(items[0].refs[0]["ratios"][PIVOT_STEP - 1]) >= 1e-10:
            items[0].note = f"shift {k}"
            return Case(name, 8, False, 33, [0], items, "pivot")
    raise AssertionError("no shift keeps the ill-conditioned case under its cap")


def _single(name, c, antithetic, seed, family, subruns=(0,), first=0):
    items = search_stream(lambda sid: [c], list(subruns), antithetic, seed, first=first)
    return Case(name, c.n_steps, antithetic, seed, list(subruns), items, family)


def _shapes(name, M, antithetic, seed):
    t = [T_HALF * k / M for k in range(1, M + 1)]
    every = range(M)
    cs = [contract("double-out", "put", times=t, monitor=every, rebate=1.5, at_hit=True),
          contract("down-and-in", "put", times=t, monitor=every, rebate=0.4)]
    items = []
    for c in cs:
        items += search_stream(lambda sid: [c], [0], antithetic, seed)
    return Case(name, M, antithetic, seed, [0], items, "shapes")


def _finalize(name):
    """Sub-run means that agree to about 1e-9: a deep in-the-money put whose
    first step moves the spot by 1e-7 relative and is exercised there by every
    path (asserted on the reference).  Not antithetic: +z and -z would cancel
    the first order and leave means equal to 1e-16."""
    c = contract("none", "put", times=[0.2, 1.2], strike=200.0, rate=0.2, carry=0.0)
    c.step[0, capi.LSM_S_DIFF] = 1e-7
    c.step[0, capi.LSM_S_ISCALE] = 1e7
    case = _single(name, c, False, 41, "finalize", subruns=(0, 1, 2, 3))
    for r in case.items[0].refs:
        assert all(s == 1 for s in r["stops"])
    return case


MENU = {
    "minfit_put": lambda n: _minfit(n, "put", False, 12),
    "minfit_put_anti": lambda n: _minfit(n, "put", True, 12),
    "minfit_call": lambda n: _minfit(n, "call", False, 21),
    "minfit_call_anti": lambda n: _minfit(n, "call", True, 22),
    "minfit_knock_in": _minfit_ki,
    "minfit_knock_out": _minfit_ko,
    "pivot_equal_u": _pivot_equal,
    "pivot_singular": _pivot_singular,
    "pivot_ill": _pivot_ill,
    # every step monitored and an exercise date; knock-outs pay at the hit, so
    # REBATE_m differs per step and a wrong hit date shows in the value
    "events_double_out": lambda n: _single(
        n, contract("double-out", "put", monitor=range(8), rebate=1.5, at_hit=True), True, 51,
        "events"),
    "events_double_in": lambda n: _single(
        n, contract("double-in", "put", monitor=range(8), rebate=0.8), True, 52, "events"),
    # monitoring-only and exercise-only steps, interleaved
    "events_interleaved": lambda n: _single(
        n, contract("up-and-out", "put", monitor=(0, 2, 4, 6), exercise=(1, 3, 5, 7), rebate=2.0,
                    at_hit=True, upper=108.0), False, 53, "events"),
    "shape_1": lambda n: _shapes(n, 1, False, 61),
    "shape_2": lambda n: _shapes(n, 2, True, 62),
    "shape_5": lambda n: _shapes(n, 5, False, 63),
    "shape_7": lambda n: _shapes(n, 7, True, 64),
    "sharded": lambda n: _single(
        n, contract("up-and-out", "put", monitor=(1, 4, 5, 7), rebate=1.0, at_hit=True), True, 71,
        "sharded", subruns=range(SHARD_FIRST, SHARD_FIRST + 3)),
    "finalize": _finalize,
}
REGENERATED = ("pivot_equal_u", "shape_2")  # rebuilt by the host test, compared exactly


def build_case(name) -> Case:
    return MENU[name](name)


# ---------------------------------------------------------------------------
# the long launches (compared against host_subruns only; no fixture but ids)
# ---------------------------------------------------------------------------
def long_contracts(M):
    """n_steps = 511 / 512: exercise flags every 64th step, two monitored
    dates; none, down-and-out, up-and-in, double-out."""
    t = [T_HALF * k / M for k in range(1, M + 1)]
    ex = [i for i in range(M) if (i + 1) % 64 == 0]
    mon = (M // 3, M - 1)
    return [contract("none", "put", times=t, exercise=ex),
            contract("down-and-out", "put", times=t, monitor=mon, exercise=ex, rebate=1.0,
                     at_hit=True),
            contract("up-and-in", "call", times=t, monitor=mon, exercise=ex, rebate=0.5),
            contract("double-out", "call", times=t, monitor=mon, exercise=ex, rebate=0.7,
                     at_hit=True)]


LONG_SEED = 81


# ---------------------------------------------------------------------------
# fixture <-> Case
# ---------------------------------------------------------------------------
def case_to_fixture(case: Case, arrays: dict) -> dict:
    """JSON part of a case; the arrays go into `arrays` under name/item/..."""
    doc = dict(family=case.family, n_steps=case.n_steps, antithetic=case.antithetic,
               seed=case.seed, subruns=list(case.subruns), items=[])
    for k, it in enumerate(case.items):
        key = f"{case.name}/{k}"
        c = it.contract
        arrays[f"{key}/params"] = c.params
        arrays[f"{key}/flags"] = c.flags
        arrays[f"{key}/step"] = c.step
        arrays[f"{key}/times"] = c.times
        per_values = True  # every sub-run's values fit under the committed-file limit
        runs = []
        for g, (r, bb, ex) in enumerate(zip(it.refs, it.bounds, it.excluded)):
            gk = f"{key}/{g}"
            vals = np.array([float(v) for v in r["values"]])
            stops = np.array(r["stops"], dtype=np.uint8 if case.n_steps < 256 else np.uint16)
            arrays[f"{gk}/stops"] = stops
            arrays[f"{gk}/coef"] = np.array([[float(v) for v in row] for row in r["coef"]])
            if per_values:
                arrays[f"{gk}/values"] = vals
            if ex.any():
                arrays[f"{gk}/excluded"] = np.packbits(ex)
            fits = {}
            for m, b in bb.items():
                member = np.zeros(N, dtype=bool)
                member[r["fit_paths"][m]] = True
                arrays[f"{gk}/fit{m}"] = np.packbits(member)
                fits[str(m)] = dict(dc=b.dc, du_abs=b.du_abs)
            runs.append(dict(
                valid=[bool(v) for v in r["valid"]], fitted=[bool(v) for v in r["fitted"]],
                count=r["count"], ratios=r["ratios"], invalid=r["invalid"],
                min_margin=None if mp.isinf(r["min_margin"]) else float(r["min_margin"]),
                fit_mean=float(r["fit_mean"]), price_mean=float(r["price_mean"]),
                value_sum_kept=float(mp.fsum(v for v, e in zip(r["values"], ex) if not e)),
                fits=fits, census=r["census"]))
        doc["items"].append(dict(
            stream_id=it.stream_id, barrier_type=c.barrier_type, n_decisions=it.n_decisions,
            n_low_margin=it.n_low_margin, worst_margin_ratio=it.worst_margin_ratio, note=it.note,
            runs=runs))
    return doc


@dataclass
class StoredRun:
    doc: dict
    coef: np.ndarray
    stops: np.ndarray
    values: Optional[np.ndarray]
    excluded: np.ndarray
    members: dict   # m -> bool [N]
    bounds: dict    # m -> FitBound


@dataclass
class StoredItem:
    contract: LsmContract
    stream_id: int
    doc: dict
    runs: List[StoredRun]


def load_case(name, doc, arrays) -> List[StoredItem]:
    out = []
    for k, idoc in enumerate(doc["items"]):
        key = f"{name}/{k}"
        c = LsmContract(params=arrays[f"{key}/params"], flags=arrays[f"{key}/flags"],
                        step=arrays[f"{key}/step"], times=arrays[f"{key}/times"],
                        barrier_type=idoc["barrier_type"])
        runs = []
        for g, rdoc in enumerate(idoc["runs"]):
            gk = f"{key}/{g}"
            coef = arrays[f"{gk}/coef"]
            ex = (np.unpackbits(arrays[f"{gk}/excluded"]).astype(bool)
                  if f"{gk}/excluded" in arrays else np.zeros(N, dtype=bool))
            members = {int(m): np.unpackbits(arrays[f"{gk}/fit{m}"]).astype(bool)
                       for m in rdoc["fits"]}
            bounds = {int(m): FitBound(c=[float(v) for v in coef[int(m) - 1]], dc=f["dc"],
                                       du_abs=f["du_abs"]) for m, f in rdoc["fits"].items()}
            runs.append(StoredRun(doc=rdoc, coef=coef, stops=arrays[f"{gk}/stops"],
                                  values=arrays[f"{gk}/values"] if f"{gk}/values" in arrays
                                  else None, excluded=ex, members=members, bounds=bounds))
        out.append(StoredItem(contract=c, stream_id=idoc["stream_id"], doc=idoc, runs=runs))
    return out


# ---------------------------------------------------------------------------
# an engine's output against a stored item (both tests)
# ---------------------------------------------------------------------------
def value_bound(ref, spot):
    """The project's Monte Carlo bound (test_gpu_mc.py)."""
    return 1e-11 * np.abs(ref) + 1e-12 * spot


def check_engine(case_doc, item: StoredItem, coef, values, stats_invalid, min_margin,
                 fit_means=None):
    """coef [G, M, 5], values [G, N] of an engine for `item`, against the
    fixture under the bounds of DESIGN.md 13.1.  -> the worst error-to-bound
    ratios (fit, value, margin), for the record."""
    c = item.contract
    spot = float(c.params[capi.LSM_P_SPOT])
    worst = dict(fit=0.0, value=0.0, margin=0.0)
    invalid, ref_margin, big_bound = 0, math.inf, 0.0
    for g, (run, sub) in enumerate(zip(item.runs, case_doc["subruns"])):
        d = run.doc
        want = np.array([1.0 if (v and f) else 0.0 for v, f in zip(d["valid"], d["fitted"])])
        assert np.array_equal(coef[g, :, 4], want), (g, coef[g, :, 4], want)
        invalid += d["invalid"]
        x = float_walk(c, sub, case_doc["antithetic"], case_doc["seed"], 2 * item.stream_id)
        for m, b in run.bounds.items():
            u = float_regressor(c, x, m)[run.members[m]]
            got = coef[g, m - 1, 0] + u * (coef[g, m - 1, 1] + u * (coef[g, m - 1, 2]
                                                                   + u * coef[g, m - 1, 3]))
            ref = run.coef[m - 1, 0] + u * (run.coef[m - 1, 1] + u * (run.coef[m - 1, 2]
                                                                     + u * run.coef[m - 1, 3]))
            bound = b(u)
            ratio = float(np.max(np.abs(got - ref) / bound))
            worst["fit"] = max(worst["fit"], ratio)
            assert ratio <= 1.0, (g, m, ratio)
            big_bound = max(big_bound, float(bound.max()))
        for m in range(1, c.n_steps + 1):  # no coefficients where there is no valid fit
            if m not in run.bounds:
                assert not coef[g, m - 1, :4].any(), (g, m)
        keep = ~run.excluded
        if run.values is not None:
            err = np.abs(values[g] - run.values)[keep]
            vb = value_bound(run.values, spot)[keep]
            worst["value"] = max(worst["value"], float(np.max(err / vb)))
            assert np.all(err <= vb), (g, float(err.max()))
        # the stopping steps are in the values: a path stopped elsewhere is paid
        # another amount; with per-path values not stored, their sum carries it
        total = float(np.sum(values[g][keep]))
        assert abs(total - d["value_sum_kept"]) <= N * float(value_bound(
            d["value_sum_kept"] / N, spot)), (g, total)
        if fit_means is not None and item.doc["n_low_margin"] == 0:
            assert abs(fit_means[g] - d["fit_mean"]) <= value_bound(d["fit_mean"], spot), g
        if d["min_margin"] is not None:
            ref_margin = min(ref_margin, d["min_margin"])
    assert int(stats_invalid) == invalid, (stats_invalid, invalid)
    if math.isinf(ref_margin):
        assert math.isinf(min_margin)
    elif item.doc["n_low_margin"] == 0:
        # the smallest margin moves by at most the fit's error at that path
        # (and phi's, far smaller): 2 x the largest fit_bound
        worst["margin"] = abs(min_margin - ref_margin) / (2.0 * big_bound)
        assert abs(min_margin - ref_margin) <= 2.0 * big_bound, (min_margin, ref_margin)
    return worst
