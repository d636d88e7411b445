"""The table-policy Monte Carlo on the GPU (csrc/fdcn_mc_policy.hip) against the
NumPy host engines on the same Philox streams, the bitwise ties to the
least-squares kernel and its dual under a table that never stops, the
device-pointer entry, batch independence, sharding, and the bounds as a user
runs them."""
import math

import numpy as np
import pytest

import lsm_fixture as lf
import policy_fixture as pf
from conftest import load_golden
from finite_difference_amd import capi, mc_american
from finite_difference_amd.mc_american import ExercisePolicy

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("policy_cases.json")
T8 = [0.5 * k / 8 for k in range(1, 9)]


def _mc_bound(ref, spot):
    """The project's Monte Carlo bound on a value."""
    return 1e-11 * np.abs(ref) + 1e-12 * spot


@pytest.fixture(scope="module")
def runs():
    """Per parity batch, computed once: the batch, its stream ids, the host
    engines' references and the two device launches with their dumps."""
    out = {}
    for name, (n_outer, n_inner) in pf.PARITY.items():
        G, anti, seed, plans, pols = pf.batch(name)
        ids = GOLDEN["batches"][name]["stream_ids"]
        kw = dict(engine="hip", seed=seed, stream_ids=ids)
        out[name] = dict(
            G=G, anti=anti, seed=seed, plans=plans, pols=pols, ids=ids,
            host=pf.host_lower(name, ids), host_dual=pf.host_dual(name, ids),
            dev=mc_american.simulate_policy(plans, pols, G, anti, want_values=True, **kw),
            dev_dual=mc_american.simulate_policy_dual(plans, pols, G, n_outer, n_inner, anti,
                                                      want_gap=True, want_cont=True, **kw))
    return out


# ---------------------------------------------------------------------------
# 6. device against host, lower bound
# ---------------------------------------------------------------------------
def test_log_spot_of_device_and_host_agrees_within_tau_x():
    """The worst |x_dev - x_host| at a decision step, which the fixture's
    MIN_MARGIN_X = 100 TAU_X rests on.  Contract m of eight calls with strike
    0.001 stops every path at step m (an "always" row there, "never"
    elsewhere), so the device's x_m is log(value / DF_END_m + strike), its own
    exp and two roundings included; the host's x_m is the sum itself.

    Measured on an MI355X: 2.665e-15 (three ulp of x = 4.6).  TAU_X = 1e-12 is
    100 times that, rounded up to a power of ten."""
    strike = 1e-3
    plans = lf.plan_batch([lf._contract("none", "call", T8, (), range(8), strike=strike)
                           for _ in range(8)])
    pols = []
    for m in range(1, 9):
        pol = ExercisePolicy.never(8)
        pol.x_lo[m - 1], pol.x_hi[m - 1] = -math.inf, math.inf
        pols.append(pol)
    worst = 0.0
    for anti in (True, False):
        G, seed = 2, 21
        dev = mc_american.simulate_policy(plans, pols, G, anti, engine="hip", seed=seed,
                                          want_values=True)
        per = mc_american.obs_per_subrun(anti)
        for b, c in enumerate(plans):
            m = b + 1
            x = np.full((G, capi.LSM_SUBRUN), float(np.log(c.params[capi.LSM_P_SPOT])))
            for g in range(G):
                Z = mc_american._path_normals(8, seed, 2 * b + 1, g * per, anti)
                for i in range(m):
                    drift, diff = c.step[i, capi.LSM_S_DRIFT], c.step[i, capi.LSM_S_DIFF]
                    x[g] = x[g] + (drift + diff * Z[:, i])
            x_dev = np.log(dev["values"][b].reshape(G, -1) / c.step[m - 1, capi.LSM_S_DF_END]
                           + strike)
            worst = max(worst, float(np.max(np.abs(x_dev - x))))
            assert dev["stats"][b, capi.POLICY_O_EXERCISED] == (G * capi.LSM_SUBRUN if m < 8 else 0)
    print(f"worst |x_dev - x_host| over 8 steps, both pairings: {worst:.3e} "
          f"(TAU_X {pf.TAU_X:.0e})")
    assert worst <= pf.TAU_X / 100.0


@pytest.mark.parametrize("name", list(pf.PARITY))
def test_path_parity_with_the_host_engine(runs, name):
    """Every contract's host margin is at least MIN_MARGIN_X = 100 TAU_X, so no
    decision flips: EXERCISED is equal, every value agrees within the Monte
    Carlo bound 1e-11 |ref| + 1e-12 spot, and the smallest margins, each a
    difference of x and a table entry, agree within TAU_X.

    Measured on an MI355X, worst over the five batches: values 1.7e-3 of their
    bound (m2_kinds), margins 8.9e-16 apart (m3_kinds; equal elsewhere)."""
    r = runs[name]
    worst_v = worst_m = 0.0
    for b, (c, h) in enumerate(zip(r["plans"], r["host"])):
        spot = float(c.params[capi.LSM_P_SPOT])
        st = r["dev"]["stats"][b]
        hm = float(h["margin"].min())
        assert hm >= pf.MIN_MARGIN_X, (name, b)
        assert st[capi.POLICY_O_EXERCISED] == h["exercised"].sum(), (name, b)
        dm = float(st[capi.POLICY_O_MIN_MARGIN])
        if math.isinf(hm):
            assert math.isinf(dm) and dm > 0.0, (name, b)
        else:
            worst_m = max(worst_m, abs(dm - hm))
            assert abs(dm - hm) <= pf.TAU_X, (name, b, dm, hm)
        ref = h["values"].reshape(-1)
        err = np.abs(r["dev"]["values"][b] - ref)
        bound = _mc_bound(ref, spot)
        worst_v = max(worst_v, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        want = mc_american._finalize_policy(h["means"], hm, h["exercised"].sum())
        for k in (capi.POLICY_O_PRICE, capi.POLICY_O_SUM):
            tol = r["G"] * float(_mc_bound(want[capi.POLICY_O_PRICE], spot))
            assert abs(st[k] - want[k]) <= tol, (name, b, k)
    print(f"{name}: worst value error / bound {worst_v:.3e}, worst margin difference "
          f"{worst_m:.3e}")


def test_dev_entry_with_a_planned_workspace_matches_the_host_entry(runs):
    import torch
    r = runs["m8_all_kinds"]
    plans, G, anti, seed = r["plans"], r["G"], r["anti"], r["seed"]
    B, M = len(plans), 8
    P, F, S = mc_american._stack(plans, r["ids"])
    T = np.stack([pol.table() for pol in r["pols"]])
    dev = torch.device("cuda:0")
    dP, dF, dS, dT = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, F, S, T))
    plan = capi.mc_policy_plan(M, G, anti)
    assert plan["values_per_contract"] == G * capi.LSM_SUBRUN
    stats = torch.zeros((B, capi.POLICY_NSTAT), dtype=torch.float64, device=dev)
    val = torch.full((B, plan["values_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    ws_bytes = plan["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    head = (B, M, G, anti, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), dT.data_ptr(), seed, 0)
    with torch.cuda.stream(stream):
        capi.mc_policy_batch_dev(*head, stats.data_ptr(), val.data_ptr(), ws.data_ptr(), ws_bytes,
                                 stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), r["dev"]["stats"])
    assert np.array_equal(val.cpu().numpy(), r["dev"]["values"])
    # library-owned scratch (NULL workspace) gives the same numbers
    stats2 = torch.zeros_like(stats)
    capi.mc_policy_batch_dev(*head, stats2.data_ptr(), None, None, 0, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats2.cpu().numpy(), r["dev"]["stats"])
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_policy_batch_dev(*head, stats.data_ptr(), None, ws.data_ptr(), ws_bytes - 1,
                                 stream.cuda_stream)
    # and the dual's
    n_outer, n_inner = pf.PARITY["m8_all_kinds"]
    dplan = capi.mc_policy_dual_plan(M, G, anti, n_outer, n_inner)
    dstats = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
    gap = torch.full((B, dplan["gap_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    cont = torch.full((B, dplan["cont_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    dws_bytes = dplan["ws_bytes_per_contract"] * B
    dws = torch.zeros(dws_bytes // 8, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    dhead = (B, M, G, anti, n_outer, n_inner) + head[4:]
    with torch.cuda.stream(stream):
        capi.mc_policy_dual_batch_dev(*dhead, dstats.data_ptr(), gap.data_ptr(), cont.data_ptr(),
                                      dws.data_ptr(), dws_bytes, stream.cuda_stream)
    stream.synchronize()
    want = r["dev_dual"]
    assert np.array_equal(dstats.cpu().numpy(), want["stats"])
    assert np.array_equal(gap.cpu().numpy(), want["gap"])
    assert np.array_equal(cont.cpu().numpy().reshape(want["cont"].shape), want["cont"])
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_policy_dual_batch_dev(*dhead, dstats.data_ptr(), None, None, dws.data_ptr(),
                                      dws_bytes - 1, stream.cuda_stream)


# ---------------------------------------------------------------------------
# 7. bitwise ties to the existing kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pf.PARITY))
def test_a_never_stop_table_is_the_lsm_kernel_without_exercise_flags_bitwise(runs, name):
    r = runs[name]
    plans, G, anti = r["plans"], r["G"], r["anti"]
    kw = dict(engine="hip", seed=r["seed"], stream_ids=r["ids"], want_values=True)
    never = [ExercisePolicy.never(c.n_steps) for c in plans]
    pol = mc_american.simulate_policy(plans, never, G, anti, **kw)
    flat = []
    for c in plans:
        f = mc_american.LsmContract(params=c.params, flags=c.flags, step=c.step.copy(),
                                    times=c.times, barrier_type=c.barrier_type)
        f.step[:, capi.LSM_S_EXERCISE] = 0.0
        flat.append(f)
    lsm = mc_american.simulate_lsm(flat, G, anti, **kw)
    assert np.array_equal(pol["values"], lsm["values"])
    for a, b in ((capi.POLICY_O_PRICE, capi.LSM_O_PRICE), (capi.POLICY_O_STDERR, capi.LSM_O_STDERR),
                 (capi.POLICY_O_SUM, capi.LSM_O_SUM), (capi.POLICY_O_SUM2, capi.LSM_O_SUM2)):
        assert np.array_equal(pol["stats"][:, a], lsm["stats"][:, b]), (a, b)
    assert np.all(pol["stats"][:, capi.POLICY_O_EXERCISED] == 0.0)
    assert np.all(np.isposinf(pol["stats"][:, capi.POLICY_O_MIN_MARGIN]))
    # a shard: the second sub-run alone, through obs_first
    if G > 1:
        kw1 = dict(kw, subrun_first=1)
        one = mc_american.simulate_policy(plans, never, 1, anti, **kw1)
        n = capi.LSM_SUBRUN
        assert np.array_equal(one["values"], lsm["values"][:, n:2 * n])


@pytest.mark.parametrize("name", list(pf.PARITY))
def test_a_never_stop_table_is_the_fitted_dual_with_zero_coef_bitwise(runs, name):
    r = runs[name]
    plans, G, anti = r["plans"], r["G"], r["anti"]
    n_outer, n_inner = pf.PARITY[name]
    kw = dict(engine="hip", seed=r["seed"], stream_ids=r["ids"], want_gap=True, want_cont=True)
    never = [ExercisePolicy.never(c.n_steps) for c in plans]
    pol = mc_american.simulate_policy_dual(plans, never, G, n_outer, n_inner, anti, **kw)
    coef = np.zeros((len(plans), G, plans[0].n_steps, capi.LSM_NCOEF))
    fit = mc_american.simulate_dual(plans, coef, n_outer, n_inner, anti, **kw)
    for k in ("stats", "gap", "cont"):
        assert np.array_equal(pol[k], fit[k]), k
    assert pol["stats"].shape[1] == 7


# ---------------------------------------------------------------------------
# 8. device against host, dual
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(pf.PARITY))
def test_dual_parity_with_the_host_engine(runs, name):
    """The bounds of test_gpu_mc_dual.py for the fitted dual: equal inner-path
    and inner-step counts, inner means within 1e-11 |ref| + 1e-12 spot, D
    within (n_steps + 1) tau with tau = 1e-11 strike + 1e-12 spot; D >= 0.  The
    smallest margins, distances in x here, agree within TAU_X.

    Measured on an MI355X, worst ratio to the bound over the five batches:
    inner means 6.3e-4, D 9.9e-6 (both m8_all_kinds)."""
    r = runs[name]
    dev = r["dev_dual"]
    worst_c = worst_d = 0.0
    assert np.all(dev["gap"] >= 0.0) and np.all(np.isfinite(dev["gap"])), name
    assert np.all(dev["cont"] >= 0.0), name
    for b, (c, h) in enumerate(zip(r["plans"], r["host_dual"])):
        spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
        tau = 1e-11 * strike + 1e-12 * spot
        st = dev["stats"][b]
        assert st[capi.DUAL_O_INNER_PATHS] == h["inner_paths"].sum(), (name, b)
        assert st[capi.DUAL_O_INNER_STEPS] == h["inner_steps"].sum(), (name, b)
        hm, dm = float(h["margin"].min()), float(st[capi.DUAL_O_MIN_MARGIN])
        assert hm >= pf.MIN_MARGIN_X, (name, b)
        if math.isinf(hm):
            assert math.isinf(dm) and dm > 0.0, (name, b)
        else:
            assert abs(dm - hm) <= pf.TAU_X, (name, b, dm, hm)
        ref = h["cont"].reshape(-1, c.n_steps)
        assert np.array_equal(dev["cont"][b] != 0.0, ref != 0.0), (name, b)
        err = np.abs(dev["cont"][b] - ref)
        bound = _mc_bound(ref, spot)
        worst_c = max(worst_c, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        d_err = np.abs(dev["gap"][b] - h["gaps"].reshape(-1))
        worst_d = max(worst_d, float(d_err.max()) / ((c.n_steps + 1) * tau))
        assert np.all(d_err <= (c.n_steps + 1) * tau), (name, b, float(d_err.max()))
        want = mc_american._finalize_dual(h["gaps"], hm, h["inner_paths"].sum(),
                                          h["inner_steps"].sum())
        for k in (capi.DUAL_O_GAP, capi.DUAL_O_SUM):
            assert abs(st[k] - want[k]) <= (c.n_steps + 1) * tau * max(1, h["gaps"].shape[0])
        if not np.any(c.step[:-1, capi.LSM_S_EXERCISE] != 0.0):
            assert np.all(dev["gap"][b] == 0.0) and st[capi.DUAL_O_INNER_PATHS] == 0.0
    print(f"{name}: worst ratio to the bound: inner means {worst_c:.3e}, D {worst_d:.3e}")


# ---------------------------------------------------------------------------
# 9. invariance
# ---------------------------------------------------------------------------
def test_bitwise_batch_independence_rerun_and_sharding(runs):
    r = runs["m8_all_kinds"]
    plans, pols, ids, G, anti = r["plans"], r["pols"], r["ids"], r["G"], r["anti"]
    n_outer, n_inner = pf.PARITY["m8_all_kinds"]
    kw = dict(engine="hip", seed=r["seed"])
    pick = [0, 7, 2, 9, 12, 3, 5]  # contract 3 at position 5 of B = 7

    def lower(sel, **more):
        return mc_american.simulate_policy([plans[k] for k in sel], [pols[k] for k in sel], G,
                                           anti, stream_ids=[ids[k] for k in sel],
                                           want_values=True, **{**kw, **more})

    def dual(sel, g=G, **more):
        return mc_american.simulate_policy_dual(
            [plans[k] for k in sel], [pols[k] for k in sel], g, n_outer, n_inner, anti,
            stream_ids=[ids[k] for k in sel], want_gap=True, want_cont=True, **{**kw, **more})

    for fn, whole, keys in ((lower, r["dev"], ("stats", "values")),
                            (dual, r["dev_dual"], ("stats", "gap", "cont"))):
        many, one, again = fn(pick), fn([3]), fn([3])
        for k in keys:
            assert np.array_equal(one[k][0], many[k][5]), k
            assert np.array_equal(one[k][0], whole[k][3]), k
            assert np.array_equal(one[k], again[k]), k
    # sub-runs [0, 1) and [1, 2) are the whole run's
    everyone = list(range(len(plans)))
    parts = [mc_american.simulate_policy(plans, pols, 1, anti, stream_ids=ids, subrun_first=g,
                                         want_values=True, **kw) for g in range(G)]
    assert np.array_equal(np.concatenate([p["values"] for p in parts], axis=1),
                          r["dev"]["values"])
    dparts = [dual(everyone, g=1, subrun_first=g) for g in range(G)]
    assert np.array_equal(np.concatenate([p["gap"] for p in dparts], axis=1),
                          r["dev_dual"]["gap"])
    for b in everyone:
        w = r["dev"]["stats"][b]
        m = mc_american.merge_policy_stats(
            [(1, p["stats"][b, capi.POLICY_O_SUM], p["stats"][b, capi.POLICY_O_SUM2])
             for p in parts])
        assert m["sum_mean"] == pytest.approx(w[capi.POLICY_O_SUM], rel=1e-14, abs=0.0)
        assert m["sum_mean2"] == pytest.approx(w[capi.POLICY_O_SUM2], rel=1e-14, abs=0.0)
        assert sum(p["stats"][b, capi.POLICY_O_EXERCISED] for p in parts) == \
            w[capi.POLICY_O_EXERCISED]
        w = r["dev_dual"]["stats"][b]
        m = mc_american.merge_dual_stats(
            [(1, p["stats"][b, capi.DUAL_O_SUM], p["stats"][b, capi.DUAL_O_SUM2]) for p in dparts])
        assert m["sum_gap"] == pytest.approx(w[capi.DUAL_O_SUM], rel=1e-14, abs=0.0)
        assert m["sum_gap2"] == pytest.approx(w[capi.DUAL_O_SUM2], rel=1e-14, abs=0.0)
    # another stream id is another run
    other = mc_american.simulate_policy([plans[3]], [pols[3]], G, anti, stream_ids=[ids[3] + 1],
                                        want_values=True, **kw)
    assert not np.array_equal(other["values"][0], r["dev"]["values"][3])


# ---------------------------------------------------------------------------
# 10. the facade
# ---------------------------------------------------------------------------
def test_bounds_of_the_weekly_bermudan_end_to_end():
    """price_policy_mc_bounds on the device at the sizes of the host test (G =
    256, n_outer = 2, n_inner = 512): the host engine's numbers within the
    parity bounds, and the FD price inside the bracket with grid_error =
    |fd(400) - fd(200)|, z = 5 and no percentage allowance."""
    _, fd, grid, c, pol = pf.trade_case("put_weekly")
    kw = dict(n_subruns=pf.END_G, seed=pf.END_SEED, n_outer=pf.END_OUTER, n_inner=pf.END_INNER)
    host = mc_american.price_policy_mc_bounds(c, pol, engine="host", **kw)
    assert min(host["min_margin"], host["dual_min_margin"]) >= pf.MIN_MARGIN_X
    dev = mc_american.price_policy_mc_bounds(c, pol, engine="hip", **kw)
    spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
    print(f"device lower {dev['price']:.6f} +- {dev['stderr']:.6f}, gap {dev['gap']:.6f} +- "
          f"{dev['gap_stderr']:.6f}, upper {dev['upper']:.6f}; host lower {host['price']:.6f}, "
          f"gap {host['gap']:.6f}; FD {fd:.6f}")
    assert dev["exercised"] == host["exercised"] and dev["inner_paths"] == host["inner_paths"]
    assert abs(dev["price"] - host["price"]) <= float(_mc_bound(host["price"], spot))
    assert abs(dev["gap"] - host["gap"]) <= (c.n_steps + 1) * (1e-11 * strike + 1e-12 * spot)
    assert dev["upper"] == dev["price"] + dev["gap"] and dev["gap"] >= 0.0
    assert mc_american.brackets(dev, fd, grid_error=grid, z=5.0)
