"""Cash dividends in the dual and the table-policy Monte Carlo kernels on the GPU
(the DIV instances of csrc/fdcn_mc_dual.hip and csrc/fdcn_mc_policy.hip) against
the NumPy host engines on the same Philox streams, the bitwise ties among the
entries, the device-pointer entries, batch independence and sharding, the
log-spot tolerance under dividends, and a dividend Bermudan end to end."""
import math

import numpy as np
import pytest

import bounds_div_cases as bdc
import lsm_div_cases as ldc
from conftest import load_golden
from finite_difference_amd import capi, mc_american
from finite_difference_amd.mc_american import ExercisePolicy, LsmContract

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("bounds_div_cases.json")
PATH = "path"


def _mc_bound(ref, spot):
    """The project's Monte Carlo bound on a value."""
    return 1e-11 * np.abs(ref) + 1e-12 * spot


@pytest.fixture(scope="module")
def runs():
    """Per batch, computed once: the batch, its stream ids, the host engines'
    references and the three device launches with their dumps."""
    out = {}
    for name, (n_outer, n_inner) in bdc.PARITY.items():
        G, anti, seed, plans, pols, _ = bdc.batch(name)
        g = GOLDEN["batches"][name]
        tids, fids = g["table_ids"], g["fit_ids"]
        coef = bdc.fitted(name)
        kw = dict(engine="hip", seed=seed, cash_dividends=PATH)
        dkw = dict(want_gap=True, want_cont=True, **kw)
        assert all(c.has_dividends for c in plans)
        out[name] = dict(
            G=G, anti=anti, seed=seed, plans=plans, pols=pols, coef=coef, tids=tids, fids=fids,
            host=bdc.host_lower(name, tids), host_table=bdc.host_table_dual(name, tids),
            host_fit=bdc.host_fitted_dual(name, coef, fids),
            dev=mc_american.simulate_policy(plans, pols, G, anti, want_values=True,
                                            stream_ids=tids, **kw),
            dev_table=mc_american.simulate_policy_dual(plans, pols, G, n_outer, n_inner, anti,
                                                       stream_ids=tids, **dkw),
            dev_fit=mc_american.simulate_dual(plans, coef, n_outer, n_inner, anti,
                                              stream_ids=fids, **dkw))
    return out


# ---------------------------------------------------------------------------
# 1. device against host on the fixture's stream ids
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bdc.PARITY))
def test_lower_bound_parity_with_the_host_engine(runs, name):
    """No decision flips (host margins >= 100 TAU_X): EXERCISED is equal and every
    value is within 1e-11 |ref| + 1e-12 spot.

    Measured on an MI355X, worst value error / bound: 2.3e-3 (m8_div)."""
    r = runs[name]
    worst = 0.0
    for b, (c, h) in enumerate(zip(r["plans"], r["host"])):
        spot = float(c.params[capi.LSM_P_SPOT])
        st = r["dev"]["stats"][b]
        hm, dm = float(h["margin"].min()), float(st[capi.POLICY_O_MIN_MARGIN])
        assert hm >= bdc.MIN_MARGIN_X, (name, b)
        assert st[capi.POLICY_O_EXERCISED] == h["exercised"].sum(), (name, b)
        if math.isinf(hm):
            assert math.isinf(dm) and dm > 0.0, (name, b)
        else:
            assert abs(dm - hm) <= bdc.TAU_X, (name, b, dm, hm)
        ref = h["values"].reshape(-1)
        err = np.abs(r["dev"]["values"][b] - ref)
        bound = _mc_bound(ref, spot)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        want = mc_american._finalize_policy(h["means"], hm, h["exercised"].sum())
        for k in (capi.POLICY_O_PRICE, capi.POLICY_O_SUM):
            tol = r["G"] * float(_mc_bound(want[capi.POLICY_O_PRICE], spot))
            assert abs(st[k] - want[k]) <= tol, (name, b, k)
    print(f"{name}: lower bound, worst value error / bound {worst:.3e}")


@pytest.mark.parametrize("rule", ["table", "fit"])
@pytest.mark.parametrize("name", list(bdc.PARITY))
def test_dual_parity_with_the_host_engine(runs, name, rule):
    """Fitted and table dual: equal inner-path and inner-step counts, inner means
    within 1e-11 |ref| + 1e-12 spot, D within (n_steps + 1) (1e-11 strike + 1e-12
    spot), D >= 0.

    Measured on an MI355X, worst ratio to the bound over the four batches: inner
    means 3.5e-4 (m8_div, both rules), D 4.3e-6 (m2_div, table)."""
    r = runs[name]
    dev, host = r["dev_" + rule], r["host_" + rule]
    worst_c = worst_d = 0.0
    assert np.all(dev["gap"] >= 0.0) and np.all(np.isfinite(dev["gap"])), name
    assert np.all(dev["cont"] >= 0.0), name
    for b, (c, h) in enumerate(zip(r["plans"], host)):
        spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
        tau = 1e-11 * strike + 1e-12 * spot
        st = dev["stats"][b]
        hm = float(h["margin"].min())
        assert hm >= (bdc.MIN_MARGIN_X if rule == "table" else bdc.min_margin_c(c)), (name, b)
        assert st[capi.DUAL_O_INNER_PATHS] == h["inner_paths"].sum(), (name, b)
        assert st[capi.DUAL_O_INNER_STEPS] == h["inner_steps"].sum(), (name, b)
        ref = h["cont"].reshape(-1, c.n_steps)
        assert np.array_equal(dev["cont"][b] != 0.0, ref != 0.0), (name, b)
        err = np.abs(dev["cont"][b] - ref)
        bound = _mc_bound(ref, spot)
        worst_c = max(worst_c, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        d_err = np.abs(dev["gap"][b] - h["gaps"].reshape(-1))
        worst_d = max(worst_d, float(d_err.max()) / ((c.n_steps + 1) * tau))
        assert np.all(d_err <= (c.n_steps + 1) * tau), (name, b, float(d_err.max()))
        if not np.any(c.step[:-1, capi.LSM_S_EXERCISE] != 0.0):
            assert np.all(dev["gap"][b] == 0.0) and st[capi.DUAL_O_INNER_PATHS] == 0.0
    print(f"{name} {rule}: worst ratio to the bound: inner means {worst_c:.3e}, D {worst_d:.3e}")


# ---------------------------------------------------------------------------
# 2. bitwise, on the device
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m8_div", "m3_div"])
def test_an_all_zero_div_through_each_div_entry_is_the_plain_entry(runs, name):
    r = runs[name]
    G, anti, seed = r["G"], r["anti"], r["seed"]
    n_outer, n_inner = bdc.PARITY[name]
    P, F, S = mc_american._stack(r["plans"], r["tids"])
    T = np.stack([pol.table() for pol in r["pols"]])
    Z = np.zeros((len(r["plans"]), r["plans"][0].n_steps))
    a = capi.mc_policy_batch(P, F, S, T, G, anti, seed=seed, want_values=True)
    z = capi.mc_policy_div_batch(P, F, S, Z, T, G, anti, seed=seed, want_values=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, z))
    kw = dict(seed=seed, want_gap=True, want_cont=True)
    a = capi.mc_policy_dual_batch(P, F, S, T, G, n_outer, n_inner, anti, **kw)
    z = capi.mc_policy_dual_div_batch(P, F, S, Z, T, G, n_outer, n_inner, anti, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, z))
    a = capi.mc_dual_batch(P, F, S, r["coef"], n_outer, n_inner, anti, **kw)
    z = capi.mc_dual_div_batch(P, F, S, Z, r["coef"], n_outer, n_inner, anti, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, z))
    assert np.any(a[2] > 0.0)  # inner simulations ran: the comparison is not of zeros


@pytest.mark.parametrize("name", list(bdc.PARITY))
def test_never_stop_tables_tie_the_three_div_kernels_bitwise(runs, name):
    """fdcn_mc_policy_div_batch under "never" is fdcn_mc_lsm_div_batch on the
    contract without EXERCISE flags; the table dual under "never" is the fitted
    dual under an all-zero coef."""
    r = runs[name]
    plans, G, anti = r["plans"], r["G"], r["anti"]
    n_outer, n_inner = bdc.PARITY[name]
    kw = dict(engine="hip", seed=r["seed"], stream_ids=r["tids"])
    never = [ExercisePolicy.never(c.n_steps) for c in plans]
    pol = mc_american.simulate_policy(plans, never, G, anti, want_values=True,
                                      cash_dividends=PATH, **kw)
    flat = []
    for c in plans:
        f = LsmContract(params=c.params, flags=c.flags, step=c.step.copy(), times=c.times,
                        barrier_type=c.barrier_type, div=c.div)
        f.step[:, capi.LSM_S_EXERCISE] = 0.0
        flat.append(f)
    lsm = mc_american.simulate_lsm(flat, G, anti, want_values=True, **kw)
    assert np.array_equal(pol["values"], lsm["values"])
    for a, b in ((capi.POLICY_O_PRICE, capi.LSM_O_PRICE), (capi.POLICY_O_STDERR, capi.LSM_O_STDERR),
                 (capi.POLICY_O_SUM, capi.LSM_O_SUM), (capi.POLICY_O_SUM2, capi.LSM_O_SUM2)):
        assert np.array_equal(pol["stats"][:, a], lsm["stats"][:, b]), (a, b)
    assert not np.array_equal(pol["values"], mc_american.simulate_policy(
        [LsmContract(params=c.params, flags=c.flags, step=c.step, times=c.times,
                     barrier_type=c.barrier_type) for c in plans], never, G, anti,
        want_values=True, **kw)["values"])  # the dividends are on the path
    dkw = dict(want_gap=True, want_cont=True, cash_dividends=PATH, **kw)
    tab = mc_american.simulate_policy_dual(plans, never, G, n_outer, n_inner, anti, **dkw)
    coef = np.zeros((len(plans), G, plans[0].n_steps, capi.LSM_NCOEF))
    fit = mc_american.simulate_dual(plans, coef, n_outer, n_inner, anti, **dkw)
    for k in ("stats", "gap", "cont"):
        assert np.array_equal(tab[k], fit[k]), k


def test_dev_entries_with_a_planned_workspace_match_the_host_entries(runs):
    import torch
    name = "m8_div"
    r = runs[name]
    plans, G, anti, seed = r["plans"], r["G"], r["anti"], r["seed"]
    n_outer, n_inner = bdc.PARITY[name]
    B, M = len(plans), 8
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    D = np.stack([c.div_row() for c in plans])
    T = np.stack([pol.table() for pol in r["pols"]])
    stream = torch.cuda.Stream(device=dev)
    # the lower bound
    P, F, S = mc_american._stack(plans, r["tids"])
    dP, dF, dS, dD, dT = (up(a) for a in (P, F, S, D, T))
    plan = capi.mc_policy_plan(M, G, anti)
    stats = torch.zeros((B, capi.POLICY_NSTAT), dtype=torch.float64, device=dev)
    val = torch.full((B, plan["values_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    ws_bytes = plan["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    head = (B, M, G, anti, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), dD.data_ptr(),
            dT.data_ptr(), seed, 0)
    with torch.cuda.stream(stream):
        capi.mc_policy_div_batch_dev(*head, stats.data_ptr(), val.data_ptr(), ws.data_ptr(),
                                     ws_bytes, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), r["dev"]["stats"])
    assert np.array_equal(val.cpu().numpy(), r["dev"]["values"])
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_policy_div_batch_dev(*head, stats.data_ptr(), None, ws.data_ptr(), ws_bytes - 1,
                                     stream.cuda_stream)
    with pytest.raises(capi.FdcnError, match="div is NULL"):
        capi.mc_policy_div_batch_dev(*head[:7], None, *head[8:], stats.data_ptr(), None, None, 0,
                                     stream.cuda_stream)
    # the two duals
    dplan = capi.mc_policy_dual_plan(M, G, anti, n_outer, n_inner)
    assert dplan == capi.mc_dual_plan(M, G, anti, n_outer, n_inner)
    dws_bytes = dplan["ws_bytes_per_contract"] * B
    Pf, Ff, Sf = mc_american._stack(plans, r["fids"])
    dFf, dC = up(Ff), up(r["coef"])
    for fn, flags, rule, want in (
            (capi.mc_policy_dual_div_batch_dev, dF, dT, r["dev_table"]),
            (capi.mc_dual_div_batch_dev, dFf, dC, r["dev_fit"])):
        dstats = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
        gap = torch.full((B, dplan["gap_per_contract"]), -1.0, dtype=torch.float64, device=dev)
        cont = torch.full((B, dplan["cont_per_contract"]), -1.0, dtype=torch.float64, device=dev)
        dws = torch.zeros(dws_bytes // 8, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        dhead = (B, M, G, anti, n_outer, n_inner, dP.data_ptr(), flags.data_ptr(), dS.data_ptr(),
                 dD.data_ptr(), rule.data_ptr(), seed, 0)
        with torch.cuda.stream(stream):
            fn(*dhead, dstats.data_ptr(), gap.data_ptr(), cont.data_ptr(), dws.data_ptr(),
               dws_bytes, stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(dstats.cpu().numpy(), want["stats"])
        assert np.array_equal(gap.cpu().numpy(), want["gap"])
        assert np.array_equal(cont.cpu().numpy().reshape(want["cont"].shape), want["cont"])
        with pytest.raises(capi.FdcnError, match="workspace"):
            fn(*dhead, dstats.data_ptr(), None, None, dws.data_ptr(), dws_bytes - 1,
               stream.cuda_stream)


def test_bitwise_batch_independence_rerun_and_sharding(runs):
    name = "m8_div"
    r = runs[name]
    plans, pols, coef, G, anti = r["plans"], r["pols"], r["coef"], r["G"], r["anti"]
    n_outer, n_inner = bdc.PARITY[name]
    kw = dict(engine="hip", seed=r["seed"], cash_dividends=PATH)
    pick = [0, 7, 2, 8, 1, 3, 5]  # contract 3 at position 5 of B = 7

    def lower(sel, g=G, **more):
        return mc_american.simulate_policy([plans[k] for k in sel], [pols[k] for k in sel], g,
                                           anti, stream_ids=[r["tids"][k] for k in sel],
                                           want_values=True, **{**kw, **more})

    def table(sel, g=G, **more):
        return mc_american.simulate_policy_dual(
            [plans[k] for k in sel], [pols[k] for k in sel], g, n_outer, n_inner, anti,
            stream_ids=[r["tids"][k] for k in sel], want_gap=True, want_cont=True,
            **{**kw, **more})

    def fit(sel, g=G, **more):
        first = more.get("subrun_first", 0)
        return mc_american.simulate_dual(
            [plans[k] for k in sel], coef[sel][:, first:first + g], n_outer, n_inner, anti,
            stream_ids=[r["fids"][k] for k in sel], want_gap=True, want_cont=True,
            **{**kw, **more})

    everyone = list(range(len(plans)))
    for fn, whole, keys, dump in ((lower, r["dev"], ("stats", "values"), "values"),
                                  (table, r["dev_table"], ("stats", "gap", "cont"), "gap"),
                                  (fit, r["dev_fit"], ("stats", "gap", "cont"), "gap")):
        many, one, again = fn(pick), fn([3]), fn([3])
        for k in keys:
            assert np.array_equal(one[k][0], many[k][5]), (fn.__name__, k)
            assert np.array_equal(one[k][0], whole[k][3]), (fn.__name__, k)
            assert np.array_equal(one[k], again[k]), (fn.__name__, k)
        # sub-runs [0, 1) and [1, 2), each launched alone, are the whole run's
        parts = [fn(everyone, g=1, subrun_first=g) for g in range(G)]
        assert np.array_equal(np.concatenate([p[dump] for p in parts], axis=1), whole[dump]), \
            fn.__name__


# ---------------------------------------------------------------------------
# 3. the log-spot tolerance under dividends
# ---------------------------------------------------------------------------
def test_log_spot_of_device_and_host_agrees_within_tau_x_under_dividends():
    """Section 13.4's measurement with a dividend on every step before the stop:
    contract m of eight calls with strike 0.001 stops every path at step m and
    pays 2.0 on each of the steps 1 .. m - 1 and on step m itself, so the
    device's x_m is log(value / DF_END_m + strike) after m passes through g; the
    host's x_m is its own walk.  Expected from the forward rounding bound of
    section 13.2: about eps (3/2 + D / t + |y|), 2e-15 per dividend, on top of
    the 2.7e-15 measured without dividends.

    Measured on an MI355X: 4.441e-15, below 1e-14, so
    TAU_X stays 1e-12 for the dividend fixture.  Asserted <= 1e-13, a tenth of
    TAU_X."""
    strike = 1e-3
    plans, pols = [], []
    for m in range(1, 9):
        plans.append(ldc.contract("none", "call", ldc.T8, (), range(8),
                                  {i: 2.0 for i in range(m)}, strike=strike))
        pol = ExercisePolicy.never(8)
        pol.x_lo[m - 1], pol.x_hi[m - 1] = -math.inf, math.inf
        pols.append(pol)
    worst = 0.0
    for anti in (True, False):
        G, seed = 2, 21
        dev = mc_american.simulate_policy(plans, pols, G, anti, engine="hip", seed=seed,
                                          want_values=True, cash_dividends=PATH)
        per = mc_american.obs_per_subrun(anti)
        for b, c in enumerate(plans):
            m = b + 1
            x = np.empty((G, capi.LSM_SUBRUN))
            for g in range(G):
                Z = mc_american._path_normals(8, seed, 2 * b + 1, g * per, anti)
                x[g] = ldc.stored_walk(c, Z)[1][m - 1]
            x_dev = np.log(dev["values"][b].reshape(G, -1) / c.step[m - 1, capi.LSM_S_DF_END]
                           + strike)
            worst = max(worst, float(np.max(np.abs(x_dev - x))))
            assert dev["stats"][b, capi.POLICY_O_EXERCISED] == (G * capi.LSM_SUBRUN if m < 8 else 0)
    print(f"worst |x_dev - x_host| over 8 steps with up to 8 dividends, both pairings: "
          f"{worst:.3e} (TAU_X {bdc.TAU_X:.0e})")
    assert worst <= bdc.TAU_X / 10.0


# ---------------------------------------------------------------------------
# 4. a dividend Bermudan end to end
# ---------------------------------------------------------------------------
def test_bounds_of_the_dividend_bermudan_end_to_end():
    """Trade (a) of the host test (the weekly call K 230 with D = 2.5 on an
    exercise date) on the device at the same sizes and streams: the host
    engine's lower bound and gap within the per-value bounds, and the device FD
    price inside the bracket with grid_error = |fd(400) - fd(200)|, z = 5."""
    fd, grid, c, pol = bdc.trade_case("weekly_230", None)  # engine None: the device's
    kw = dict(n_subruns=bdc.END_G, seed=bdc.END_SEED, n_outer=bdc.END_OUTER,
              n_inner=bdc.END_INNER, cash_dividends=PATH)
    host = mc_american.price_policy_mc_bounds(c, pol, engine="host", **kw)
    assert min(host["min_margin"], host["dual_min_margin"]) >= bdc.MIN_MARGIN_X
    dev = mc_american.price_policy_mc_bounds(c, pol, engine="hip", **kw)
    spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
    print(f"device lower {dev['price']:.6f} +- {dev['stderr']:.6f}, gap {dev['gap']:.6f} +- "
          f"{dev['gap_stderr']:.6f}, upper {dev['upper']:.6f}; host lower {host['price']:.6f}, "
          f"gap {host['gap']:.6f}; FD {fd:.6f} (grid {grid:.2e})")
    assert c.has_dividends
    assert dev["exercised"] == host["exercised"] and dev["inner_paths"] == host["inner_paths"]
    assert abs(dev["price"] - host["price"]) <= float(_mc_bound(host["price"], spot))
    assert abs(dev["gap"] - host["gap"]) <= (c.n_steps + 1) * (1e-11 * strike + 1e-12 * spot)
    assert dev["upper"] == dev["price"] + dev["gap"] and dev["gap"] >= 0.0
    assert mc_american.brackets(dev, fd, grid_error=grid, z=5.0)
