"""Monte Carlo discrete-barrier pricer on the GPU (csrc/fdcn_mc.hip): payoff
parity with the reference on its own normals, the generator against the
documented mapping, its moments, statistical parity on the device stream,
bitwise determinism / batch independence / range splitting, the tails, and the
device-pointer entry.  Every launch has valid arguments or is rejected on the
host before the device is touched."""
import math

import numpy as np
import pytest

import mc_fixture as fx
from finite_difference_amd import analytic, capi, mc_barrier
from finite_difference_amd.mc_barrier import MCConfig, price_discrete_barrier_mc

pytestmark = pytest.mark.gpu

CASES = fx.load_cases()
ARRAYS = fx.load_arrays()


def _plan(case):
    return mc_barrier.plan_contract(**fx.kwargs_for(case["inputs"], mc_barrier))


@pytest.fixture(scope="module")
def chunk():
    return capi.mc_plan(1)["obs_per_block"]


@pytest.fixture(scope="module")
def eight_step_plans():
    return [_plan(c) for c in CASES["small"] if c["result"]["steps"] == 8]


# ---------------------------------------------------------------------------
# payoff parity, normals supplied
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["small"], ids=lambda c: c["name"])
def test_payoff_parity_on_the_references_normals(case):
    """|gpu - ref| <= 1e-11 |ref| + 1e-12 spot per observation and for the
    price: one device exp per step is within 1 ulp, with the multiply the
    relative error of s is at most 3 n_steps 2^-53 ~ 2.7e-15 at 8 steps, about
    1e-12 absolute at s <= 400; the bound keeps the project's 1e-11 relative
    and puts the absolute term two orders above that.  stderr to 1e-9."""
    plan = _plan(case)
    z = ARRAYS[case["normals"]]
    anti = case["inputs"]["cfg"]["antithetic"]
    sums, pay = mc_barrier.simulate([plan], z.shape[0], anti, engine="hip", z=z,
                                    want_payoffs=True)
    ref = ARRAYS[case["payoffs"]]
    spot = case["inputs"]["spot"]
    err = np.abs(pay[0] - ref)
    bound = 1e-11 * np.abs(ref) + 1e-12 * spot
    print(f"{case['name']}: worst payoff error {err.max():.3e} (bound there "
          f"{bound[np.argmax(err)]:.3e})")
    assert np.all(err <= bound)
    # and through the façade, as a user calls it
    out = price_discrete_barrier_mc(engine="hip", rng="numpy",
                                    **fx.kwargs_for(case["inputs"], mc_barrier))
    res = case["result"]
    print(f"  price error {abs(out['price'] - res['price']):.3e}")
    assert abs(out["price"] - res["price"]) <= 1e-11 * abs(res["price"]) + 1e-12 * spot
    assert abs(out["stderr"] - res["stderr"]) <= 1e-9 * abs(res["stderr"])
    assert abs(sums[0, 0] / z.shape[0] - res["price"]) <= 1e-11 * abs(res["price"]) + 1e-12 * spot
    assert sorted(out) == sorted(res)


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
Z_TOL = 1e-13  # log within 1 ulp, cos(2 pi u) argument rounding in NumPy <= 7e-16,
#                radius <= 8.6: at most 1e-14, times ten


@pytest.mark.parametrize("n_steps", [1, 2, 3, 8])
def test_generator_parity(n_steps, chunk):
    worst = 0.0
    for n_obs in (1, 255, 256, 257, chunk + 1):
        got = capi.mc_normals(n_obs, n_steps, seed=7, stream_id=0)
        want = fx.expected_normals(n_obs, n_steps, 7, 0)
        assert got.shape == want.shape
        worst = max(worst, float(np.max(np.abs(got - want))))
    print(f"n_steps {n_steps}: worst |dz| {worst:.3e}")
    assert worst <= Z_TOL


def test_generator_carries_into_the_high_counter_word():
    first = 2 ** 32 - 100
    got = capi.mc_normals(200, 3, seed=7, stream_id=2, obs_first=first)
    want = fx.expected_normals(200, 3, 7, 2, first)
    assert np.max(np.abs(got - want)) <= Z_TOL
    # the rows past the carry are not those of a wrapped 32-bit counter
    wrapped = fx.expected_normals(100, 3, 7, 2, 0)
    assert np.min(np.abs(got[100:] - wrapped)) > 0.0


def test_seeds_and_streams_give_different_streams():
    base = capi.mc_normals(257, 2, seed=7, stream_id=0)
    for seed, stream in ((8, 0), (7, 1), (7 + 2 ** 32, 0)):
        other = capi.mc_normals(257, 2, seed=seed, stream_id=stream)
        assert np.max(np.abs(other - fx.expected_normals(257, 2, seed, stream))) <= Z_TOL
        assert not np.any(other == base)


def test_generator_moments():
    """2^20 normals; every tolerance is 5 standard deviations of the sample
    moment: mean 1/sqrt n, variance sqrt(2/n), kurtosis sqrt(96/n), lag-1
    correlation between steps 1/sqrt n."""
    z = capi.mc_normals(2 ** 17, 8, seed=12345, stream_id=3)
    n = z.size
    assert n == 2 ** 20
    mean = float(z.mean())
    var = float(z.var())
    kurt = float(np.mean((z - mean) ** 4)) / var ** 2
    a, b = z[:, :-1].ravel(), z[:, 1:].ravel()
    lag = float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))
    print(f"mean {mean:.3e} var-1 {var - 1:.3e} kurt-3 {kurt - 3:.3e} lag1 {lag:.3e}")
    assert abs(mean) <= 5.0 / math.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert abs(kurt - 3.0) <= 5.0 * math.sqrt(96.0 / n)
    assert abs(lag) <= 5.0 / math.sqrt(n)


# ---------------------------------------------------------------------------
# statistical parity, device generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["large"], ids=lambda c: c["name"])
def test_statistical_parity_with_the_device_generator(case):
    """|price - ref| <= 5 s_ref sqrt(N_ref / N + 1): the reference's stderr
    scaled to this run's N, plus the reference's own error; both from the
    fixture."""
    N = 2 ** 21
    kw = fx.kwargs_for(case["inputs"], mc_barrier)
    kw["cfg"] = MCConfig(n_paths=2 * N, seed=7, antithetic=True)
    out = price_discrete_barrier_mc(engine="hip", rng="philox", **kw)
    ref = case["result"]
    bound = 5.0 * ref["stderr"] * math.sqrt(ref["n_observations"] / N + 1.0)
    print(f"{case['name']}: price {out['price']:.6f} ref {ref['price']:.6f} "
          f"diff {out['price'] - ref['price']:.3e} bound {bound:.3e} stderr {out['stderr']:.3e}")
    assert out["n_observations"] == N
    assert abs(out["price"] - ref["price"]) <= bound
    inp = case["inputs"]
    if inp["barrier"]["type"] == "none" and not inp["dividends"]:
        r = math.log(1.0 + inp["rate"])  # flat NACA: DF = (1 + naca)^-tau
        T = 31 / 365.0
        bs = float(analytic.black_scholes("p" if inp["option_type"] == "put" else "c",
                                          inp["spot"], inp["strike"], r, r, inp["vol"], T))
        print(f"  closed form {bs:.6f} diff {out['price'] - bs:.3e}")
        assert abs(out["price"] - bs) <= bound


# ---------------------------------------------------------------------------
# determinism and independence (bitwise)
# ---------------------------------------------------------------------------
def test_result_is_independent_of_the_batch(eight_step_plans, chunk):
    kinds = {int(p.flags[capi.MC_F_KIND]) for p in eight_step_plans}
    assert kinds == {0, 1, 2, 4}
    three = _plan(next(c for c in CASES["small"] if c["name"] == "di_call_3"))
    # a down-and-in on the eight-step grid: the fifth kind of the mix
    di = mc_barrier.McContract(**{**eight_step_plans[2].__dict__})
    di.params, di.flags = three.params.copy(), three.flags.copy()
    pool = eight_step_plans + [di]
    batch = [pool[k % len(pool)] for k in range(37)]
    assert {int(p.flags[capi.MC_F_KIND]) for p in batch} == {0, 1, 2, 3, 4}
    n_obs = chunk + 904
    kw = dict(engine="hip", rng="philox", seed=99, want_payoffs=True)
    alone = mc_barrier.simulate([batch[17]], n_obs, True, stream_ids=[17], **kw)
    mixed = mc_barrier.simulate(batch, n_obs, True, **kw)
    again = mc_barrier.simulate(batch, n_obs, True, **kw)
    assert np.array_equal(alone[1][0], mixed[1][17]) and np.array_equal(alone[0][0], mixed[0][17])
    assert np.array_equal(mixed[0], again[0]) and np.array_equal(mixed[1], again[1])
    # another stream id is another sample
    assert not np.array_equal(mixed[1][17], mixed[1][17 + len(pool)])


def test_ranges_continue_one_stream(eight_step_plans, chunk):
    plan = eight_step_plans[2]
    n, k = chunk + 1904, 1500
    assert k % chunk != 0
    kw = dict(engine="hip", rng="philox", seed=5, stream_ids=[4], want_payoffs=True)
    whole = mc_barrier.simulate([plan], n, True, **kw)
    head = mc_barrier.simulate([plan], k, True, **kw)
    tail = mc_barrier.simulate([plan], n - k, True, obs_first=k, **kw)
    assert np.array_equal(whole[1][0], np.concatenate([head[1][0], tail[1][0]]))
    merged = mc_barrier.merge_mc_stats([(k, *head[0][0]), (n - k, *tail[0][0])])
    price = whole[0][0, 0] / n
    assert abs(merged["price"] - price) <= 1e-14 * abs(price)


# ---------------------------------------------------------------------------
# tails, against the host engine on the same normals
# ---------------------------------------------------------------------------
def _pair(kw, cfg):
    return (price_discrete_barrier_mc(engine="hip", rng="numpy", cfg=cfg, **kw),
            price_discrete_barrier_mc(engine="host", rng="numpy", cfg=cfg, **kw))


def _same(gpu, host, spot):
    assert gpu["n_observations"] == host["n_observations"]
    assert abs(gpu["price"] - host["price"]) <= 1e-11 * abs(host["price"]) + 1e-12 * spot
    assert abs(gpu["stderr"] - host["stderr"]) <= 1e-9 * abs(host["stderr"])


def test_tails(chunk):
    inputs = CASES["small"][2]["inputs"]  # up-and-out call, eight steps
    kw = {k: v for k, v in fx.kwargs_for(inputs, mc_barrier).items() if k != "cfg"}
    spot = inputs["spot"]
    gpu, host = _pair(kw, MCConfig(n_paths=1, seed=11, antithetic=False))
    _same(gpu, host, spot)
    assert gpu["n_observations"] == 1 and gpu["stderr"] == 0.0
    gpu, host = _pair(kw, MCConfig(n_paths=chunk + 1, seed=11, antithetic=False,
                                   chunk_size=chunk + 1))
    _same(gpu, host, spot)
    assert gpu["n_observations"] == chunk + 1
    gpu, host = _pair(kw, MCConfig(n_paths=3, seed=11, antithetic=True))
    _same(gpu, host, spot)
    assert gpu["n_observations"] == 1 and gpu["stderr"] == 0.0


# ---------------------------------------------------------------------------
# device-pointer entry
# ---------------------------------------------------------------------------
def test_dev_entry_matches_the_host_entry(eight_step_plans, chunk):
    import torch
    B, n_obs = len(eight_step_plans), chunk + 77
    P, F, S = mc_barrier._stack(eight_step_plans, list(range(B)))
    want, want_pay = capi.mc_barrier_batch(P, F, S, n_obs, True, seed=21, want_payoffs=True)
    dev = torch.device("cuda:0")
    dP, dF, dS = (torch.from_numpy(a).to(dev) for a in (P, F, S))
    stats = torch.zeros((B, capi.MC_NSTAT), dtype=torch.float64, device=dev)
    pay = torch.zeros((B, n_obs), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_plan(n_obs)["ws_bytes_per_contract"] * B
    ws = torch.zeros(ws_bytes // 8, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    with torch.cuda.stream(stream):
        capi.mc_barrier_batch_dev(B, 8, n_obs, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
                                  None, 21, 0, stats.data_ptr(), pay.data_ptr(), ws.data_ptr(),
                                  ws_bytes, stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), want)
    assert np.array_equal(pay.cpu().numpy(), want_pay)
    # library-owned scratch (NULL workspace) gives the same numbers
    stats2 = torch.zeros_like(stats)
    capi.mc_barrier_batch_dev(B, 8, n_obs, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(),
                              None, 21, 0, stats2.data_ptr(), None, None, 0,
                              stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(stats2.cpu().numpy(), want)
    # one byte short: refused on the host, nothing launched
    with pytest.raises(capi.FdcnError, match="workspace"):
        capi.mc_barrier_batch_dev(B, 8, n_obs, True, dP.data_ptr(), dF.data_ptr(),
                                  dS.data_ptr(), None, 21, 0, stats.data_ptr(), None,
                                  ws.data_ptr(), ws_bytes - 1, stream.cuda_stream)
