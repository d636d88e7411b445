"""Monte Carlo bounds under a given exercise table, without a GPU: the C
entries' validation, policy_from_pricer on the Bermudan trades, the NumPy host
engines against a per-path walk written from the contract text of
include/fdcn.h, their identities, and the bounds end to end against the FD
price and, path for path, against the least-squares Monte Carlo."""
import math

import numpy as np
import pytest

import lsm_fixture as lf
import policy_fixture as pf
from backends import oracle_engine
from conftest import load_golden
from finite_difference_amd import AmericanBarrierFDMPricer, capi, mc_american
from finite_difference_amd.mc_american import ExercisePolicy
from test_bermudan_host import DIV_DAY, WEEKLY, trade

GOLDEN = load_golden("policy_cases.json")
T8 = [0.5 * k / 8 for k in range(1, 9)]
NEW = ("fdcn_mc_policy_batch", "fdcn_mc_policy_batch_dev", "fdcn_mc_policy_plan",
       "fdcn_mc_policy_dual_batch", "fdcn_mc_policy_dual_batch_dev", "fdcn_mc_policy_dual_plan")


# ---------------------------------------------------------------------------
# 1. the six C entries
# ---------------------------------------------------------------------------
def test_symbols_are_exported_and_the_abi_is_still_8():
    L = capi.lib()
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(L, name), name
    assert L.fdcn_abi_version() == 8
    assert (capi.POLICY_NCOL, capi.POLICY_NSTAT) == (2, 6)
    assert capi.mc_policy_plan(8, 3, True) == dict(
        obs_per_subrun=2048, ws_bytes_per_contract=3 * 4 * 8, values_per_contract=3 * 4096)
    assert capi.mc_policy_plan(8, 3, False)["obs_per_subrun"] == 4096
    assert capi.mc_policy_dual_plan(8, 2, True, 3, 512) == capi.mc_dual_plan(8, 2, True, 3, 512)


def _raw(which, entry="host", **kw):
    """fdcn_mc_policy_batch (which = "lower") or fdcn_mc_policy_dual_batch
    ("dual"), their _dev and _plan, straight through ctypes with one valid
    contract unless told otherwise: validation happens before any device is
    touched, so without a GPU a valid call ends in FDCN_ENODEV (-3)."""
    kind = kw.pop("kind", "up-and-out")
    c = lf.plan_batch([lf._contract(kind, "put", T8, (3,) if kind != "none" else (), range(8),
                                    rebate=1.0 if kind != "none" else 0.0)])[0]
    a = dict(B=1, n_steps=8, G=2, anti=1, n_outer=2, n_inner=512, first=0, policy=True,
             stats=True, policy_value=None, params=True, flags=True, step=True)
    a.update(kw)
    P, F, S = mc_american._stack([c], [0])
    for (arr, idx), value in a.get("poke", {}).items():
        {"P": P, "F": F, "S": S}[arr][idx] = value
    T = ExercisePolicy(np.full(8, -math.inf), np.full(8, math.log(95.0))).table()[None].copy()
    if a["policy_value"] is not None:
        T[0, 3, 1] = a["policy_value"]
    stats = np.empty((1, 8))
    L = capi.lib()
    ptr = lambda arr, on: arr.ctypes.data if on else None  # noqa: E731
    arrays = (ptr(P, a["params"]), ptr(F, a["flags"]), ptr(S, a["step"]), ptr(T, a["policy"]))
    if which == "lower":
        head = (a["B"], a["n_steps"], a["G"], a["anti"])
        if entry == "plan":
            rc = L.fdcn_mc_policy_plan(*head[1:], None, None, None)
        else:
            args = head + arrays + (7, a["first"], ptr(stats, a["stats"]), None)
            rc = (L.fdcn_mc_policy_batch(*args) if entry == "host"
                  else L.fdcn_mc_policy_batch_dev(*args, None, 0, None))
    else:
        head = (a["B"], a["n_steps"], a["G"], a["anti"], a["n_outer"], a["n_inner"])
        if entry == "plan":
            rc = L.fdcn_mc_policy_dual_plan(*head[1:], None, None, None)
        else:
            args = head + arrays + (7, a["first"], ptr(stats, a["stats"]), None, None)
            rc = (L.fdcn_mc_policy_dual_batch(*args) if entry == "host"
                  else L.fdcn_mc_policy_dual_batch_dev(*args, None, 0, None))
    return rc, L.fdcn_last_error().decode()


SIZES = [(dict(G=0), "G must"), (dict(B=0), "B must"), (dict(n_steps=0), "n_steps"),
         (dict(n_steps=513), "n_steps"), (dict(anti=2), "antithetic"),
         (dict(anti=-1), "antithetic"), (dict(B=2 ** 16, G=2 ** 16), "grid")]
POINTERS = [(dict(policy=False), "policy is NULL"), (dict(stats=False), "stats is NULL"),
            (dict(params=False), "params is NULL"), (dict(flags=False), "flags is NULL"),
            (dict(step=False), "step is NULL")]
LOWER_ONLY = [(dict(first=-2048), "obs_first"), (dict(first=100), "obs_first"),
              (dict(first=4096 + 2048, anti=0), "obs_first")]
DUAL_ONLY = [(dict(n_outer=0), "n_outer"), (dict(n_outer=1025), "n_outer"),
             (dict(n_inner=256), "n_inner"), (dict(n_inner=256 + 512), "n_inner"),
             (dict(n_inner=16384 + 512), "n_inner"), (dict(n_inner=384, anti=0), "n_inner"),
             (dict(first=-1), "subrun_first"), (dict(first=2 ** 31 - 1), "subrun_first")]


@pytest.mark.parametrize("which, kw, word",
                         [(w, kw, word) for w in ("lower", "dual") for kw, word in SIZES + POINTERS]
                         + [("lower", kw, word) for kw, word in LOWER_ONLY]
                         + [("dual", kw, word) for kw, word in DUAL_ONLY])
def test_c_entries_refuse_bad_sizes_and_pointers(which, kw, word):
    for entry in ("host", "dev"):
        rc, msg = _raw(which, entry, **kw)
        assert rc == -1 and word in msg, (entry, rc, msg)
    if not any(k in kw for k in ("B", "first", "policy", "stats", "params", "flags", "step")):
        rc, msg = _raw(which, "plan", **kw)
        assert rc == -1 and word in msg, (rc, msg)


# every defect of a contract fdcn_mc_lsm_batch's host entry lists
CONTENTS = [
    ({("F", (0, capi.LSM_F_PUT)): 2}, "put must be"),
    ({("F", (0, capi.LSM_F_KIND)): 7}, "kind must be"),
    ({("F", (0, capi.LSM_F_STREAM)): 2 ** 30}, "stream id"),
    ({("F", (0, capi.LSM_F_STREAM)): -1}, "stream id"),
    ({("P", (0, capi.LSM_P_SPOT)): 0.0}, "spot must be positive"),
    ({("P", (0, capi.LSM_P_SPOT)): math.inf}, "spot must be positive"),
    ({("P", (0, capi.LSM_P_STRIKE)): -1.0}, "strike must be positive"),
    ({("P", (0, capi.LSM_P_UPPER)): 0.0}, "upper level must be positive"),
    ({("F", (0, capi.LSM_F_KIND)): 1, ("P", (0, capi.LSM_P_LOWER)): 0.0},
     "lower level must be positive"),
    ({("F", (0, capi.LSM_F_KIND)): 3, ("P", (0, capi.LSM_P_LOWER)): 120.0},
     "below the upper level"),
    ({("S", (0, 2, capi.LSM_S_DIFF)): 0.0}, "DIFF must be positive"),
    ({("S", (0, 2, capi.LSM_S_ISCALE)): 0.0}, "ISCALE must be positive"),
    ({("S", (0, 5, capi.LSM_S_DRIFT)): math.nan}, "not finite"),
    ({("S", (0, 5, capi.LSM_S_DF_END)): math.inf}, "not finite"),
]


@pytest.mark.parametrize("which", ["lower", "dual"])
def test_host_entries_refuse_bad_contents_and_accept_a_valid_call(which):
    for poke, word in CONTENTS:
        rc, msg = _raw(which, poke=poke)
        assert rc == -1 and word in msg, (poke, rc, msg)
    rc, msg = _raw(which, policy_value=math.nan)
    assert rc == -1 and "policy entry is NaN" in msg, (rc, msg)
    for legal in (math.inf, -math.inf):
        rc, msg = _raw(which, policy_value=legal)
        assert rc in (0, -3), (rc, msg)
    rc, msg = _raw(which, poke={("S", (0, 3, capi.LSM_S_REBATE)): -1.0})
    if which == "dual":  # the dual needs every cashflow >= 0
        assert rc == -1 and "REBATE is negative" in msg, (rc, msg)
    else:
        assert rc in (0, -3), (rc, msg)
    for kind in ("none", "up-and-out", "double-in"):
        rc, msg = _raw(which, kind=kind)
        assert rc in (0, -3), (kind, rc, msg)


def test_python_layer_refuses_bad_input():
    c = lf.plan_batch([lf._contract("none", "put", T8, (), range(8))])[0]
    with pytest.raises(ValueError, match="NaN"):
        ExercisePolicy(np.full(8, math.nan), np.zeros(8))
    with pytest.raises(ValueError, match="n_steps"):
        ExercisePolicy(np.zeros((2, 4)), np.zeros((2, 4)))
    pol = ExercisePolicy.always(8)
    cfg = mc_american.LsmConfig(n_subruns=1)
    with pytest.raises(ValueError, match="7 steps"):
        mc_american.mc_policy_batch([c], [ExercisePolicy.always(7)], cfg, engine="host")
    with pytest.raises(ValueError, match="one policy per contract"):
        mc_american.mc_policy_batch([c], [pol, pol], cfg, engine="host")
    with pytest.raises(TypeError):
        mc_american.mc_policy_batch([dict(spot=1.0)], [pol], cfg, engine="host")
    with pytest.raises(ValueError, match="engine"):
        mc_american.mc_policy_batch([c], [pol], cfg, engine="numpy")
    with pytest.raises(ValueError, match="n_inner"):
        mc_american.mc_policy_bounds_batch([c], [pol], cfg, mc_american.DualConfig(n_inner=256),
                                           engine="host")
    div = mc_american.plan_american_contract(
        spot=100.0, strike=100.0, vol=0.3, option_type="put", discount_rate=0.05, carry_rate=0.03,
        time_to_expiry=0.5, exercise_times=T8, dividends=[(0.2, 1.0)], cash_dividends="path")
    with pytest.raises(ValueError, match="dividends"):
        mc_american.mc_policy_batch([div], [ExercisePolicy.always(div.n_steps)], cfg,
                                    engine="host")
    with pytest.raises(ValueError, match="has no entry"):
        ExercisePolicy.from_critical_spots(c, {T8[0]: (90.0, 91.0)})
    with pytest.raises(ValueError, match="not one step"):
        ExercisePolicy.from_critical_spots(c, {0.123: (90.0, 91.0)})


# ---------------------------------------------------------------------------
# 2. policy_from_pricer
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trades():
    return {name: pf.trade_case(name) for name in pf.trade_kw()}


@pytest.mark.parametrize("name", list(pf.trade_kw()))
def test_policy_from_pricer_on_the_three_trades(trades, name):
    p, fd, _, c, pol = trades[name]
    ex = c.step[:, capi.LSM_S_EXERCISE] != 0.0
    ex[-1] = False
    assert pol.n_steps == c.n_steps and ex.sum() == (22 if name == "put_weekdays" else 4)
    # finite entries exactly on the EXERCISE steps; a put has no lower end
    assert np.array_equal(np.isfinite(pol.x_hi), ex)
    assert np.all(pol.x_lo[ex] == -math.inf) and np.all(pol.x_lo[~ex] == math.inf)
    assert np.all(pol.x_hi[~ex] == -math.inf)
    recs = p.exercise_boundary()
    s = np.asarray(p.s_nodes)
    rows = np.nonzero(ex)[0]
    assert len(recs) == len(rows)
    for i, (_d, t, s_star, lo, hi, count) in zip(rows, recs):
        assert abs(c.times[i] - t) <= 1e-12 and count > 0 and s_star == s[hi]
        assert math.log(s[hi]) < pol.x_hi[i] < math.log(s[hi + 1])
        assert pol.x_hi[i] == 0.5 * (math.log(s[hi]) + math.log(s[hi + 1]))
        assert pol.x_hi[i] < math.log(float(c.params[capi.LSM_P_STRIKE]))
    # the same table through from_critical_spots; None is "never"
    spots = {t: (float(s[hi]), float(s[hi + 1])) for _d, t, _s, _lo, hi, _n in recs}
    again = ExercisePolicy.from_critical_spots(c, spots)
    assert np.array_equal(again.table(), pol.table())
    spots[recs[0][1]] = None
    never = ExercisePolicy.from_critical_spots(c, spots)
    assert never.x_lo[rows[0]] > never.x_hi[rows[0]]


def test_a_call_threshold_and_the_refusals():
    eng = oracle_engine()
    # a call with a carry below the discount rate has a boundary above the strike
    c = lf.plan_batch([lf._contract("none", "call", T8, (), range(8))])[0]
    pol = ExercisePolicy.from_critical_spots(c, {t: (119.0, 121.0) for t in T8[:-1]})
    assert np.all(pol.x_hi[:-1] == math.inf) and np.all(np.isfinite(pol.x_lo[:-1]))
    assert pol.x_lo[0] == 0.5 * (math.log(119.0) + math.log(121.0))
    assert pol.x_lo[-1] > pol.x_hi[-1]  # maturity: no row needed
    with pytest.raises(ValueError, match="only Bermudan exercise dates"):
        mc_american.policy_from_pricer(trade(eng, cls=AmericanBarrierFDMPricer))
    with pytest.raises(ValueError, match="dividends"):
        mc_american.policy_from_pricer(
            trade(eng, option_type="call", strike=230.0, exercise_dates=WEEKLY,
                  dividend_schedule=[(DIV_DAY, 2.5)]))


# ---------------------------------------------------------------------------
# 3. the host engine against a per-path walk
# ---------------------------------------------------------------------------
def _walk(c, pol, z):
    """One path under the rule of include/fdcn.h, statement by statement:
    (value, the step at which it stopped, whether the rule stopped it).  np.exp
    on a scalar is the array loop of one element, so the spot is the host
    engine's bit for bit."""
    P, F, S = c.params, c.flags, c.step
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


@pytest.fixture(scope="module")
def lower_runs():
    """Per parity batch, computed once: (G, antithetic, seed, plans, policies,
    stream ids, the host engine's result per contract)."""
    out = {}
    for name in pf.PARITY:
        ids = GOLDEN["batches"][name]["stream_ids"]
        out[name] = pf.batch(name) + (ids, pf.host_lower(name, ids))
    return out


@pytest.mark.parametrize("name", list(pf.PARITY))
def test_host_engine_is_the_per_path_walk(lower_runs, name):
    G, anti, seed, plans, pols, ids, host = lower_runs[name]
    per = mc_american.obs_per_subrun(anti)
    for b, (c, pol, sid, h) in enumerate(zip(plans, pols, ids, host)):
        for g in range(G):
            Z = mc_american._path_normals(c.n_steps, seed, 2 * sid + 1, g * per, anti)
            by_rule = 0
            for p in range(capi.LSM_SUBRUN):
                v, m, ruled = _walk(c, pol, Z[p])
                assert v == h["values"][g, p] and m == h["stop_step"][g, p], (name, b, g, p)
                by_rule += ruled
            assert by_rule == h["exercised"][g], (name, b, g)
            assert h["means"][g] == mc_american._block_sum(h["values"][g:g + 1])[0] / 4096.0


def test_the_fixture_tables_hold_every_kind_of_row(lower_runs):
    seen = set()
    for name, (G, anti, seed, plans, pols, ids, host) in lower_runs.items():
        for c, pol in zip(plans, pols):
            ex = c.step[:, capi.LSM_S_EXERCISE] != 0.0
            ex[-1] = False
            for i in range(c.n_steps):
                lo, hi = pol.x_lo[i], pol.x_hi[i]
                kind = ("never" if lo > hi else "always" if lo == -math.inf and hi == math.inf
                        else "put" if lo == -math.inf else "call" if hi == math.inf else "band")
                seen.add((kind, bool(ex[i]), math.isfinite(lo) or math.isfinite(hi)))
    for kind in ("never", "always", "put", "call", "band"):
        assert any(k == kind and on for k, on, _ in seen), kind
    assert ("never", True, True) in seen and ("never", True, False) in seen
    assert any(not on and finite for _, on, finite in seen)  # a finite row without the flag
    assert {c.n_steps for r in lower_runs.values() for c in r[3]} == {1, 2, 3, 8}


def test_golden_stream_ids_reproduce_their_margins(lower_runs):
    assert GOLDEN["tau_x"] == pf.TAU_X and GOLDEN["min_margin_required"] == pf.MIN_MARGIN_X
    for name, (G, anti, seed, plans, pols, ids, host) in lower_runs.items():
        g = GOLDEN["batches"][name]
        dual = pf.host_dual(name, ids)
        for b, (h, d) in enumerate(zip(host, dual)):
            assert 16 * b <= ids[b] < 16 * (b + 1)
            for got, want in ((h["margin"].min(), g["min_margin"][b]),
                              (d["margin"].min(), g["dual_min_margin"][b])):
                assert lf.finite(got) == want, (name, b)
                assert got >= pf.MIN_MARGIN_X


# ---------------------------------------------------------------------------
# 4. identities of the host engines
# ---------------------------------------------------------------------------
def test_a_never_stop_table_is_the_contract_without_exercise_flags(lower_runs):
    for name, (G, anti, seed, plans, pols, ids, host) in lower_runs.items():
        for c, sid in zip(plans, ids):
            never = mc_american.host_policy_subruns(c, ExercisePolicy.never(c.n_steps), range(G),
                                                    anti, seed, sid)
            flat = mc_american.LsmContract(params=c.params, flags=c.flags, step=c.step.copy(),
                                           times=c.times, barrier_type=c.barrier_type)
            flat.step[:, capi.LSM_S_EXERCISE] = 0.0
            lsm = mc_american.host_subruns(flat, range(G), anti, seed, sid)
            assert np.array_equal(never["values"], lsm["values"]), name
            assert never["exercised"].sum() == 0 and np.all(np.isinf(never["margin"]))
            # and under any table
            same = mc_american.host_policy_subruns(flat, ExercisePolicy.always(c.n_steps),
                                                   range(G), anti, seed, sid)
            assert np.array_equal(same["values"], lsm["values"])


def test_an_always_stop_table_stops_at_the_first_exercise_step():
    """Every eligible path in the money stops at its first EXERCISE step (3 or
    6 here; the barrier is monitored at steps 2 and 5)."""
    for kind in ("none", "down-and-out", "up-and-in"):
        c = lf.plan_batch([lf._contract(kind, "put", T8, (1, 4), (2, 5, 7), rebate=0.5)])[0]
        r = mc_american.host_policy_subruns(c, ExercisePolicy.always(8), range(1), True, 5, 1)
        Z = mc_american._path_normals(8, 5, 3, 0, True)
        x = np.full(capi.LSM_SUBRUN, float(np.log(100.0)))
        want = np.full(capi.LSM_SUBRUN, 8)
        alive = np.ones(capi.LSM_SUBRUN, dtype=bool)
        inn = np.zeros(capi.LSM_SUBRUN, dtype=bool)
        for m in range(1, 8):
            x = x + (c.step[m - 1, capi.LSM_S_DRIFT] + c.step[m - 1, capi.LSM_S_DIFF] * Z[:, m - 1])
            s = np.exp(x)
            if m in (2, 5) and kind == "down-and-out":
                want[alive & (s <= 88.0)] = m
                alive &= ~(s <= 88.0)
            if m in (2, 5) and kind == "up-and-in":
                inn |= s >= 113.0
            if m in (3, 6):
                k = alive & (inn if kind == "up-and-in" else True) & (s < 100.0)
                want[k] = m
                alive &= ~k
        assert np.array_equal(r["stop_step"][0], want), kind
        assert r["exercised"][0] == np.sum((want == 3) | (want == 6)) > 0, kind
        assert r["margin"][0] == math.inf


def test_the_dual_gap_is_non_negative_and_zero_without_exercise_steps(lower_runs):
    for name, (G, anti, seed, plans, pols, ids, host) in lower_runs.items():
        for b, d in enumerate(pf.host_dual(name, ids)):
            assert np.all(d["gaps"] >= 0.0) and np.all(np.isfinite(d["gaps"])), (name, b)
            assert np.all(d["cont"] >= 0.0)
            ex = plans[b].step[:-1, capi.LSM_S_EXERCISE]
            if not np.any(ex != 0.0):
                assert np.all(d["gaps"] == 0.0) and d["inner_paths"].sum() == 0.0, (name, b)
    # a never-stop table is the fitted dual with an all-zero coef, bit for bit
    G, anti, seed, plans, pols, ids, _ = lower_runs["m8_bermudan"]
    n_outer, n_inner = pf.PARITY["m8_bermudan"]
    for c, sid in zip(plans, ids):
        a = mc_american.host_policy_dual_subruns(c, ExercisePolicy.never(8), range(G), n_outer,
                                                 n_inner, anti, seed, sid)
        z = mc_american.host_dual_subruns(c, np.zeros((G, 8, capi.LSM_NCOEF)), range(G), n_outer,
                                          n_inner, anti, seed, sid)
        for k in ("gaps", "cont", "inner_paths", "inner_steps", "margin"):
            assert np.array_equal(a[k], z[k]), k


def test_shards_merge_to_the_whole_run():
    c = lf.plan_batch([lf._contract("up-and-out", "put", T8, (1, 4, 7), range(8), rebate=1.0,
                                    at_hit=True)])[0]
    pol = ExercisePolicy(np.full(8, -math.inf), np.full(8, math.log(93.0)))
    cfg, dual = mc_american.LsmConfig(n_subruns=5, seed=9), mc_american.DualConfig(2, 512)
    kw = dict(engine="host", stream_ids=[4])
    whole = mc_american.mc_policy_bounds_batch([c], [pol], cfg, dual, **kw)[0]
    parts = [mc_american.mc_policy_bounds_batch([c], [pol], cfg, dual, subrun_range=r, **kw)[0]
             for r in (range(0, 2), range(2, 5))]
    m = mc_american.merge_policy_stats(parts)
    assert m["n_subruns"] == 5 and m["exercised"] == whole["exercised"]
    assert m["min_margin"] == whole["min_margin"]
    assert m["price"] == pytest.approx(whole["price"], rel=1e-14)
    assert m["stderr"] == pytest.approx(whole["stderr"], rel=1e-9)
    d = mc_american.merge_dual_stats(parts)
    assert d["gap"] == pytest.approx(whole["gap"], rel=1e-13, abs=1e-18)
    assert d["gap_stderr"] == pytest.approx(whole["gap_stderr"], rel=1e-9, abs=1e-18)
    assert sum(p["inner_paths"] for p in parts) == whole["inner_paths"]
    # the whole run's sub-run means are the shards', bit for bit
    v = [mc_american.simulate_policy([c], [pol], n, True, engine="host", seed=9, stream_ids=[4],
                                     subrun_first=f, want_values=True)["values"]
         for f, n in ((0, 5), (0, 2), (2, 3))]
    assert np.array_equal(v[0], np.concatenate(v[1:], axis=1))


def test_a_fixed_price_is_answered_without_a_launch():
    c = lf.plan_batch([lf._contract("none", "put", T8, (), range(8))])[0]
    c.fixed_price = 1.25
    r = mc_american.mc_policy_bounds_batch([c], [None], mc_american.LsmConfig(n_subruns=3),
                                           engine="hip")[0]  # no device is asked for
    assert r["price"] == r["upper"] == 1.25 and r["gap"] == 0.0 and r["n_paths"] == 0
    assert r["exercised"] == 0 and math.isinf(r["min_margin"])
    assert mc_american.brackets(r, 1.25)


# ---------------------------------------------------------------------------
# 5. end to end on the host engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bounds(trades):
    cfg = mc_american.LsmConfig(n_subruns=pf.END_G, antithetic=True, seed=pf.END_SEED)
    dual = mc_american.DualConfig(pf.END_OUTER, pf.END_INNER)
    return {name: mc_american.mc_policy_bounds_batch([t[3]], [t[4]], cfg, dual, engine="host")[0]
            for name, t in trades.items()}


@pytest.mark.parametrize("name", list(pf.trade_kw()))
def test_the_fd_boundary_brackets_the_fd_price(trades, bounds, name):
    """brackets() at z = 5 with grid_error = |fd(400) - fd(200)| and no
    percentage allowance, at G = 256, n_outer = 2, n_inner = 512.  Measured
    (host engine; gap / FD): weekdays 2.69446 +- 0.00483, gap 0.00840 (0.31 %);
    weekly 2.67641 +- 0.00501, gap 0.00083 (0.03 %); up-and-out 19.10610 +-
    0.00264, gap 0.00617 (0.03 %) -- against 0.9 % for the fitted policy."""
    _, fd, grid, _, _ = trades[name]
    r = bounds[name]
    print(f"{name}: FD {fd:.5f} (grid {grid:.5f})  lower {r['price']:.5f} +- {r['stderr']:.5f}  "
          f"gap {r['gap']:.5f} +- {r['gap_stderr']:.5f}  upper {r['upper']:.5f} +- "
          f"{r['upper_stderr']:.5f}  width {100.0 * r['gap'] / fd:.3f} %  exercised "
          f"{r['exercised']}")
    assert r["gap"] >= 0.0 and r["upper"] == r["price"] + r["gap"]
    assert mc_american.brackets(r, fd, grid_error=grid, z=5.0)


def _paired(c, pol, G, seed):
    """Mean and standard error over the sub-runs of (policy value - LSM value)
    on the same price-set paths."""
    kw = dict(engine="host", seed=seed, want_values=True)
    a = mc_american.simulate_policy([c], [pol], G, True, **kw)["values"].reshape(G, -1)
    b = mc_american.simulate_lsm([c], G, True, **kw)["values"].reshape(G, -1)
    d = (a - b).mean(axis=1)
    return float(d.mean()), float(d.std(ddof=1) / math.sqrt(G))


@pytest.mark.parametrize("name", list(pf.trade_kw()))
def test_the_fd_policy_is_no_worse_than_the_fitted_one_path_for_path(trades, name):
    """Measured at G = 256: weekdays +7.3, weekly +7.1, up-and-out +8.2
    standard errors."""
    _, _, _, c, pol = trades[name]
    mean, se = _paired(c, pol, pf.END_G, pf.END_SEED)
    print(f"{name}: policy - LSM = {mean:.5f} +- {se:.5f} ({mean / se:+.2f} s.e.)")
    assert mean >= -3.0 * se
    if name == "up_out_250_weekly":
        assert mean > 3.0 * se


def test_an_up_and_in_under_the_vanilla_twins_policy(trades):
    """The fitted policy of an up-and-in degenerates (every fit is short of
    paths); the vanilla twin's FD boundary, applied from the hit on, is no
    worse."""
    p, _, _, c, _ = trades["put_weekdays"]
    T = p.time_to_expiry
    ki = mc_american.plan_american_contract(
        spot=float(c.params[capi.LSM_P_SPOT]), strike=float(c.params[capi.LSM_P_STRIKE]),
        vol=p.sigma, option_type="put", discount_rate=p.discount_rate_nacc,
        carry_rate=p.carry_rate_nacc, time_to_expiry=T, barrier_type="up-and-in",
        upper_barrier=245.0, monitor_times=list(c.times), exercise_times=list(c.times[:-1]))
    assert ki.n_steps == c.n_steps
    pol = mc_american.policy_from_pricer(p, ki)
    assert np.array_equal(pol.table(), trades["put_weekdays"][4].table())
    mean, se = _paired(ki, pol, 64, pf.END_SEED)
    print(f"up-and-in: policy - LSM = {mean:.5f} +- {se:.5f} ({mean / se:+.2f} s.e.)")
    assert mean >= -3.0 * se
