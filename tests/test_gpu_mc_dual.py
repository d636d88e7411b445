"""The dual upper bound on the GPU (csrc/fdcn_mc_dual.hip) against the NumPy
host engine on the same Philox streams and under the same policies -- the
coefficient rows come from the host engine's least-squares fits
(dual_fixture.policies), so a policy difference cannot enter --, the properties
that hold exactly, bitwise determinism / batch independence / the
device-pointer entry, sharding, and the bounds as a user runs them."""
import math

import numpy as np
import pytest

import dual_fixture as df
import lsm_fixture as lf
from conftest import load_golden
from finite_difference_amd import capi, mc_american

pytestmark = pytest.mark.gpu

GOLDEN = load_golden("lsm_dual_cases.json")
LSM_GOLDEN = load_golden("lsm_cases.json")
BATCHES = lf.batches()
T8 = [0.5 * k / 8 for k in range(1, 9)]


@pytest.fixture(scope="module")
def runs():
    """Per parity batch, computed once: plans, policies, stream ids, the host
    reference per contract and the device launch with both dumps."""
    out = {}
    for name, (n_outer, n_inner) in df.PARITY.items():
        G, anti, seed, _ = BATCHES[name]
        plans, coef = df.policies(name)
        ids = GOLDEN["batches"][name]["stream_ids"]
        host = df.host_dual(name, plans, coef, ids)
        dev = mc_american.simulate_dual(plans, coef, n_outer, n_inner, anti, engine="hip",
                                        seed=seed, stream_ids=ids, want_gap=True, want_cont=True)
        out[name] = (plans, coef, ids, host, dev)
    return out


@pytest.mark.parametrize("name", list(df.PARITY))
def test_path_parity_with_the_host_engine(runs, name):
    """Device against host per outer path.  Every contract's host-engine
    margin, outer and inner decisions alike, is at least lsm_fixture.MIN_MARGIN,
    so no stopping decision flips: the inner-path and inner-step counts are
    equal, and the smallest margins -- each a difference of an exp and a cubic,
    so equal up to the two engines' exp -- agree within the per-term bound
    tau = 1e-11 strike + 1e-12 spot.  The inner means agree within 1e-11 |ref|
    + 1e-12 spot, the project's Monte Carlo bound, and D within (n_steps + 1)
    tau: r and the candidates add at most n_steps such terms, and D itself may
    be 0.

    Measured on an MI355X, worst ratio to the bound over the five batches:
    inner means 6.3e-4 (m8_all_kinds), D 5.4e-7 (m8_all_kinds; most D of the
    batches are exactly 0 on both engines), margins 1.3e-5."""
    n_outer, n_inner = df.PARITY[name]
    plans, coef, ids, host, dev = runs[name]
    worst_c = worst_d = worst_m = 0.0
    for b, (c, h) in enumerate(zip(plans, host)):
        spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
        tau = 1e-11 * strike + 1e-12 * spot
        st = dev["stats"][b]
        assert st[capi.DUAL_O_INNER_PATHS] == h["inner_paths"].sum(), (name, b)
        assert st[capi.DUAL_O_INNER_STEPS] == h["inner_steps"].sum(), (name, b)
        hm, dm = float(h["margin"].min()), float(st[capi.DUAL_O_MIN_MARGIN])
        assert hm >= lf.MIN_MARGIN, (name, b)
        if math.isinf(hm):
            assert math.isinf(dm) and dm > 0.0, (name, b)
        else:
            worst_m = max(worst_m, abs(dm - hm) / tau)
            assert abs(dm - hm) <= tau, (name, b, dm, hm)
        ref = h["cont"].reshape(-1, c.n_steps)
        assert np.array_equal(dev["cont"][b] != 0.0, ref != 0.0), (name, b)
        err = np.abs(dev["cont"][b] - ref)
        bound = 1e-11 * np.abs(ref) + 1e-12 * spot
        worst_c = max(worst_c, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        d_ref = h["gaps"].reshape(-1)
        d_err = np.abs(dev["gap"][b] - d_ref)
        worst_d = max(worst_d, float(d_err.max()) / ((c.n_steps + 1) * tau))
        assert np.all(d_err <= (c.n_steps + 1) * tau), (name, b, float(d_err.max()))
        want = mc_american._finalize_dual(h["gaps"], hm, h["inner_paths"].sum(),
                                          h["inner_steps"].sum())
        for k in (capi.DUAL_O_GAP, capi.DUAL_O_SUM):
            assert abs(st[k] - want[k]) <= (c.n_steps + 1) * tau * max(1, h["gaps"].shape[0])
    print(f"{name}: worst ratio to the bound: inner means {worst_c:.3e}, D {worst_d:.3e}, "
          f"margins {worst_m:.3e}")


def test_gaps_are_non_negative_and_the_zero_cases_are_exact(runs):
    for name, (plans, coef, ids, host, dev) in runs.items():
        assert np.all(dev["gap"] >= 0.0) and np.all(np.isfinite(dev["gap"])), name
        assert np.all(dev["cont"] >= 0.0), name
    # no EXERCISE step before maturity: the European of m8_bermudan, all of m1_kinds
    for name, b in [("m8_bermudan", 4)] + [("m1_kinds", b) for b in range(7)]:
        gap, cont, st = (runs[name][4][k][b] for k in ("gap", "cont", "stats"))
        assert np.all(gap == 0.0) and np.all(cont == 0.0)
        assert st[capi.DUAL_O_GAP] == 0.0 and st[capi.DUAL_O_INNER_PATHS] == 0.0
        assert st[capi.DUAL_O_INNER_STEPS] == 0.0 and math.isinf(st[capi.DUAL_O_MIN_MARGIN])
    # a knock-in whose barrier is never reached; a knock-out breached on step 1
    # (every path is above 1e-6) under the hold-to-maturity policy
    far = lf.plan_batch([lf._contract("up-and-in", "put", T8, range(8), range(8), rebate=1.0)])[0]
    far.params[capi.LSM_P_UPPER] = 1e6
    out = lf.plan_batch([lf._contract("up-and-out", "put", T8, (0,), range(8), rebate=1.0,
                                      strike=150.0)])[0]
    out.params[capi.LSM_P_UPPER] = 1e-6
    coef = np.zeros((2, 2, 8, capi.LSM_NCOEF))
    coef[0] = mc_american.host_subruns(far, range(2), True, 3, 1)["coef"]
    r = mc_american.simulate_dual([far, out], coef, 3, 512, True, engine="hip", seed=3,
                                  stream_ids=[1, 2], want_gap=True, want_cont=True)
    assert np.all(r["gap"] == 0.0) and np.all(r["cont"] == 0.0)
    assert np.all(r["stats"][:, capi.DUAL_O_INNER_PATHS] == 0.0)
    # and the opposite: holding a put deep in the money to maturity has a gap
    deep = lf.plan_batch([lf._contract("none", "put", T8, (), range(8), strike=150.0)])[0]
    r = mc_american.simulate_dual([deep], coef[1:], 3, 1024, True, engine="hip", seed=5,
                                  want_gap=True)
    assert np.all(r["gap"] > 0.0)
    assert r["stats"][0, capi.DUAL_O_INNER_PATHS] == 2 * 3 * 7 * 1024
    assert r["stats"][0, capi.DUAL_O_INNER_STEPS] == 2 * 3 * 1024 * sum(range(1, 8))
    # every D is positive here, so the bound on D of the parity test is put to
    # work: (n_steps + 1) (1e-11 strike + 1e-12 spot)
    h = mc_american.host_dual_subruns(deep, coef[1], range(2), 3, 1024, True, 5, 0)
    err = np.abs(r["gap"][0] - h["gaps"].reshape(-1))
    bound = 9 * (1e-11 * 150.0 + 1e-12 * 100.0)
    print(f"deep put: D {r['gap'][0].min():.4f} .. {r['gap'][0].max():.4f}, worst error "
          f"{err.max():.3e} = {err.max() / bound:.3e} of its bound")
    assert np.all(err <= bound)


def test_dev_entry_with_a_planned_workspace_matches_the_host_entry(runs):
    import torch
    name = "m8_bermudan"
    plans, coef, ids, _, want = runs[name]
    G, anti, seed, _ = BATCHES[name]
    n_outer, n_inner = df.PARITY[name]
    B, M = len(plans), 8
    P, F, S = mc_american._stack(plans, ids)
    dev = torch.device("cuda:0")
    dP, dF, dS, dC = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (P, F, S, coef))
    plan = capi.mc_dual_plan(M, G, anti, n_outer, n_inner)
    assert plan["gap_per_contract"] == G * n_outer
    assert plan["cont_per_contract"] == G * n_outer * M
    stats = torch.zeros((B, capi.DUAL_NSTAT), dtype=torch.float64, device=dev)
    gap = torch.full((B, plan["gap_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    cont = torch.full((B, plan["cont_per_contract"]), -1.0, dtype=torch.float64, device=dev)
    ws_bytes = plan["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    head = (B, M, G, anti, n_outer, n_inner, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
            dC.data_ptr(), seed, 0)
    with torch.cuda.stream(stream):
        capi.mc_dual_batch_dev(*head, stats.data_ptr(), gap.data_ptr(), cont.data_ptr(),
                               ws.data_ptr(), ws_bytes, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), want["stats"])
    assert np.array_equal(gap.cpu().numpy(), want["gap"])
    assert np.array_equal(cont.cpu().numpy().reshape(want["cont"].shape), want["cont"])
    # library-owned scratch (NULL workspace) gives the same numbers
    stats2 = torch.zeros_like(stats)
    capi.mc_dual_batch_dev(*head, stats2.data_ptr(), None, None, None, 0, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats2.cpu().numpy(), want["stats"])
    # one byte short: refused on the host, nothing launched
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_dual_batch_dev(*head, stats.data_ptr(), None, None, ws.data_ptr(), ws_bytes - 1,
                               stream.cuda_stream)


def test_bitwise_batch_independence_and_sharding(runs):
    name = "m8_all_kinds"
    plans, coef, ids, _, whole = runs[name]
    G, anti, seed, _ = BATCHES[name]
    n_outer, n_inner = df.PARITY[name]
    kw = dict(engine="hip", seed=seed, want_gap=True, want_cont=True)
    pick = [0, 7, 2, 9, 12, 3, 5]  # contract 3 at position 5 of B = 7
    many = mc_american.simulate_dual([plans[k] for k in pick], coef[pick], n_outer, n_inner, anti,
                                     stream_ids=[ids[k] for k in pick], **kw)
    one = mc_american.simulate_dual([plans[3]], coef[3:4], n_outer, n_inner, anti,
                                    stream_ids=[ids[3]], **kw)
    for k in ("stats", "gap", "cont"):
        assert np.array_equal(one[k][0], many[k][5]), k
        assert np.array_equal(one[k][0], whole[k][3]), k
    # sub-runs [0, 1) and [1, 2) are the whole run's: the same D, and (sum, sum of
    # squares) of the sub-run gaps merge to the whole run's
    parts = [mc_american.simulate_dual(plans, coef[:, g:g + 1], n_outer, n_inner, anti,
                                       stream_ids=ids, subrun_first=g, **kw) for g in range(G)]
    assert np.array_equal(np.concatenate([p["gap"] for p in parts], axis=1), whole["gap"])
    for b in range(len(plans)):
        m = mc_american.merge_dual_stats(
            [(1, p["stats"][b, capi.DUAL_O_SUM], p["stats"][b, capi.DUAL_O_SUM2]) for p in parts])
        w = whole["stats"][b]
        assert m["sum_gap"] == pytest.approx(w[capi.DUAL_O_SUM], rel=1e-14, abs=0.0)
        assert m["sum_gap2"] == pytest.approx(w[capi.DUAL_O_SUM2], rel=1e-14, abs=0.0)
        assert m["gap_stderr"] == pytest.approx(w[capi.DUAL_O_STDERR], rel=1e-9, abs=1e-18)
    other = mc_american.simulate_dual([plans[3]], coef[3:4], n_outer, n_inner, anti,
                                      stream_ids=[ids[3] + 1], **kw)
    assert not np.array_equal(other["cont"][0], one["cont"][0])


@pytest.mark.parametrize("name", list(lf.TRADES))
def test_bounds_of_the_fixture_trades_end_to_end(name):
    """mc_american_bounds_batch on the device at the golden run's G = 32,
    n_outer = 4, n_inner = 1024, seed and stream id.  The policies are the
    device's own fits here, so the gap agrees with the host engine's golden gap
    statistically, within 5 sqrt(2) gap_stderr; and the bracket of the FD
    price holds as in test_mc_dual_host.py: the fixture's G = 1024 lower bound,
    this gap, grid_error = |fd_3200 - fd_1600|, z = 5."""
    fix, g = LSM_GOLDEN["trades"][name], GOLDEN["trades"][name]
    cfg = mc_american.LsmConfig(n_subruns=g["n_subruns"], antithetic=True, seed=g["seed"])
    r = mc_american.mc_american_bounds_batch(
        [df.trade_contract(name)], cfg, mc_american.DualConfig(g["n_outer"], g["n_inner"]),
        engine="hip", stream_ids=[g["stream_id"]])[0]
    print(f"{name}: device lower {r['price']:.5f} +- {r['stderr']:.5f}, gap {r['gap']:.5f} +- "
          f"{r['gap_stderr']:.5f}, upper {r['upper']:.5f}; golden gap {g['gap']:.5f} +- "
          f"{g['gap_stderr']:.5f}; fd_3200 {fix['fd_3200']:.5f}")
    assert r["gap"] >= 0.0 and r["steps"] == fix["n_steps"]
    assert abs(r["gap"] - g["gap"]) <= 5.0 * math.sqrt(2.0) * g["gap_stderr"]
    assert r["upper"] == r["price"] + r["gap"]
    res, grid = df.trade_bracket(fix, r["gap"], r["gap_stderr"])
    assert mc_american.brackets(res, fix["fd_3200"], grid_error=grid, z=5.0)
    assert mc_american.brackets(r, fix["fd_3200"], grid_error=grid, z=5.0)
