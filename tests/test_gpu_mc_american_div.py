"""Cash dividends on the path of the least-squares Monte Carlo, on the GPU
(lsm_kernel<ANTI, true>, fdcn_mc_lsm_div_batch): an all-zero dividend row is
the plain entry bit for bit, path-for-path parity with the NumPy host engine
on the smallest shapes, sub-run sharding, the device-pointer entry, and the FD
pricers with a dividend against the device LSM as a user runs it.  Every launch
has valid arguments or is rejected on the host before the device is touched."""
import numpy as np
import pytest

import lsm_div_cases as dc
import lsm_fixture as lf
from finite_difference_amd import capi, mc_american

pytestmark = pytest.mark.gpu

BATCHES = dc.div_batches()


@pytest.fixture(scope="module")
def runs():
    """Per batch, computed once: the host reference (with the fit regressors)
    and the device launch with both dumps."""
    out = {}
    for name, (G, anti, seed, cs) in BATCHES.items():
        ids = dc.STREAM_IDS[name]
        host = lf.host_reference(cs, G, anti, seed, ids)
        dev = mc_american.simulate_lsm(cs, G, anti, engine="hip", seed=seed, stream_ids=ids,
                                       want_values=True, want_coef=True)
        out[name] = (cs, ids, host, dev)
    return out


# ---------------------------------------------------------------------------
# 1. an all-zero dividend row
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True])
def test_all_zero_div_is_the_plain_entry_bitwise(anti):
    """B = 2, G = 2, three steps: the DIV instance with D_m = 0 everywhere
    against the plain instance."""
    cs = [dc.contract(k, ot, dc.T3, (0, 2), range(3), {}, rebate=0.5)
          for k, ot in (("up-and-out", "put"), ("down-and-in", "call"))]
    P, F, S = mc_american._stack(cs, [4, 9])
    kw = dict(seed=21, want_values=True, want_coef=True)
    plain = capi.mc_lsm_batch(P, F, S, 2, anti, **kw)
    zero = capi.mc_lsm_batch(P, F, S, 2, anti, div=np.zeros((2, 3)), **kw)
    for a, b in zip(plain, zero):
        assert np.array_equal(a, b)
    assert plain[0][:, capi.LSM_O_PRICE].min() > 0.0


# ---------------------------------------------------------------------------
# 2. parity with the host engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BATCHES))
def test_path_parity_with_the_host_engine(runs, name):
    """test_gpu_mc_american.py's parity test with dividends on the path, under
    its tolerances: fitted continuation values on the host's regressors within
    tau_c = 1e-9 x strike, every host-engine decision margin at least
    100 tau_c, path values and prices within 1e-11 |ref| + 1e-12 spot, equal
    validity flags and invalid-step counts.  The dividend map's round trip
    moves x by about 1e-15 per dividend, three orders
    inside the value bound, which therefore carries no extra term.  Measured
    on an MI355X: worst continuation-value difference 5.0e-12 x strike (m3_div),
    worst path value error 1.8e-3 of its bound."""
    G, anti, seed, _ = BATCHES[name]
    cs, ids, host, dev = runs[name]
    n = capi.LSM_SUBRUN
    worst_c, worst_v = 0.0, 0.0
    for b, (c, h) in enumerate(zip(cs, host)):
        spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
        tau_c = lf.TAU_C_REL * strike
        assert float(h["margin"].min()) >= 100.0 * tau_c, (name, b)
        dcoef = dev["coef"][b]
        assert np.array_equal(dcoef[..., 4], h["coef"][..., 4]), (name, b)
        assert int(dev["stats"][b, capi.LSM_O_INVALID]) == int(h["invalid"].sum()), (name, b)
        u = h["fit_u"]
        gap = np.abs(lf.cubic(dcoef, u) - lf.cubic(h["coef"], u))
        if np.isfinite(gap).any():
            w = float(np.nanmax(gap))
            worst_c = max(worst_c, w / strike)
            assert w <= tau_c, (name, b, w)
        ref = h["values"].reshape(-1)
        err = np.abs(dev["values"][b] - ref)
        bound = 1e-11 * np.abs(ref) + 1e-12 * spot
        worst_v = max(worst_v, float(np.max(err / bound)))
        assert np.all(err <= bound), (name, b, float(err.max()))
        means = h["values"].sum(axis=1) / n
        st = mc_american._finalize(means, h["fit_mean"], h["invalid"].sum(), h["margin"].min())
        for k in (capi.LSM_O_PRICE, capi.LSM_O_FIT_VALUE):
            assert abs(dev["stats"][b, k] - st[k]) <= 1e-11 * abs(st[k]) + 1e-12 * spot, (name, b)
        hm, dm = float(h["margin"].min()), float(dev["stats"][b, capi.LSM_O_MIN_MARGIN])
        assert (np.isinf(hm) and np.isinf(dm)) or abs(dm - hm) <= 2.0 * tau_c, (name, b)
    print(f"{name}: worst continuation-value difference {worst_c:.3e} x strike, worst path "
          f"value error {worst_v:.3e} of its bound")


def test_the_dividend_is_on_the_device_path(runs):
    """The same contracts without their dividend rows give other values: the
    parity above is not that of two engines that both ignore `div`."""
    cs, ids, _, dev = runs["m3_div"]
    G, anti, seed, _ = BATCHES["m3_div"]
    bare = [mc_american.LsmContract(params=c.params, flags=c.flags, step=c.step, times=c.times,
                                    barrier_type=c.barrier_type) for c in cs]
    plain = mc_american.simulate_lsm(bare, G, anti, engine="hip", seed=seed, stream_ids=ids,
                                     want_values=True)
    for b in range(len(cs)):
        assert not np.array_equal(plain["values"][b], dev["values"][b]), b


# ---------------------------------------------------------------------------
# 3. sharding
# ---------------------------------------------------------------------------
def test_shard_from_obs_first_is_the_whole_runs_bitwise(runs):
    c = runs["m8_div"][0][3]   # double-out call, dividends on two consecutive steps
    kw = dict(engine="hip", seed=77, stream_ids=[12], want_values=True, want_coef=True)
    whole = mc_american.simulate_lsm([c], 8, True, **kw)
    head = mc_american.simulate_lsm([c], 5, True, subrun_first=0, **kw)
    tail = mc_american.simulate_lsm([c], 3, True, subrun_first=5, **kw)
    n = capi.LSM_SUBRUN
    assert np.array_equal(tail["values"][0], whole["values"][0, 5 * n:])
    assert np.array_equal(tail["coef"][0], whole["coef"][0, 5:])
    assert np.array_equal(head["values"][0], whole["values"][0, :5 * n])
    merged = mc_american.merge_lsm_stats(
        [(g, r["stats"][0, capi.LSM_O_SUM], r["stats"][0, capi.LSM_O_SUM2])
         for g, r in ((5, head), (3, tail))])
    w = whole["stats"][0]
    assert abs(merged["price"] - w[capi.LSM_O_PRICE]) <= 1e-14 * abs(w[capi.LSM_O_PRICE])
    assert merged["stderr"] == pytest.approx(w[capi.LSM_O_STDERR], rel=1e-9)


# ---------------------------------------------------------------------------
# 4. device-pointer entry
# ---------------------------------------------------------------------------
def test_dev_entry_matches_the_host_entry(runs):
    import torch
    cs, ids, _, want = runs["m3_div"]
    G, anti, seed, _ = BATCHES["m3_div"]
    B, M = len(cs), 3
    P, F, S = mc_american._stack(cs, ids)
    D = np.stack([c.div_row() for c in cs])
    dev = torch.device("cuda:0")
    dP, dF, dS, dD = (torch.from_numpy(a).to(dev) for a in (P, F, S, D))
    plan = capi.mc_lsm_plan(M, G, anti)
    stats = torch.zeros((B, capi.LSM_NSTAT), dtype=torch.float64, device=dev)
    val = torch.zeros((B, plan["values_per_contract"]), dtype=torch.float64, device=dev)
    coef = torch.zeros((B, plan["coef_per_contract"]), dtype=torch.float64, device=dev)
    ws_bytes = plan["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    with torch.cuda.stream(stream):
        capi.mc_lsm_div_batch_dev(B, M, G, anti, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
                                  dD.data_ptr(), seed, 0, stats.data_ptr(), val.data_ptr(),
                                  coef.data_ptr(), ws.data_ptr(), ws_bytes, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), want["stats"])
    assert np.array_equal(val.cpu().numpy(), want["values"])
    assert np.array_equal(coef.cpu().numpy().reshape(want["coef"].shape), want["coef"])
    # one byte short: refused on the host, nothing launched
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_lsm_div_batch_dev(B, M, G, anti, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
                                  dD.data_ptr(), seed, 0, stats.data_ptr(), None, None,
                                  ws.data_ptr(), ws_bytes - 1, stream.cuda_stream)


# ---------------------------------------------------------------------------
# 5. the cross-check as a user runs it
# ---------------------------------------------------------------------------
def test_fd_pricers_with_a_dividend_against_the_monte_carlo():
    """|FD_800 - LSM| <= 1 % FD_800 + 5 stderr + 2 |FD_800 - FD_400|, the
    pricers on the GPU, the LSM at G = 128 through mc_american_batch in one
    batch with a contract that pays no dividend."""
    names = list(dc.FD_TRADES)
    pricers = [dc.FD_TRADES[k](None, 400) for k in names]
    fd_400 = [float(p.price_log()) for p in pricers]
    fd_800 = [float(dc.FD_TRADES[k](None, 800).price_log()) for k in names]
    plain = dict(spot=229.74, strike=220.0, vol=0.26, option_type="put", discount_rate=0.07,
                 carry_rate=0.07, time_to_expiry=31 / 365.0, n_exercise=16)
    contracts = [dc.fd_contract(k, p) for k, p in zip(names, pricers)] + [plain]
    cfg = mc_american.LsmConfig(n_subruns=128, seed=2025)
    res = mc_american.mc_american_batch(contracts, cfg, engine="hip", cash_dividends="path")
    for k, coarse, fine, r in zip(names, fd_400, fd_800, res):
        bound = lf.fd_gap_bound(fine, coarse, r["stderr"])
        print(f"{k}: FD 400 / 800 {coarse:.5f} / {fine:.5f}, LSM {r['price']:.5f} +- "
              f"{r['stderr']:.5f} ({r['steps']} steps), gap {abs(fine - r['price']):.5f} of "
              f"{bound:.5f}")
        assert abs(fine - r["price"]) <= bound
    # the contract without a dividend is priced as it is alone, by the plain entry
    alone = mc_american.mc_american_batch([plain], cfg, engine="hip", stream_ids=[3])[0]
    assert alone == res[3]
