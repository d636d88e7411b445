"""Quasi-Monte Carlo paths on the GPU (csrc/fdcn_mc_qmc.hip): the generator
against qmc.py (the NumPy restatement of include/fdcn.h), payoff parity of the
hip engine with the host engine on the same points, bitwise determinism /
batch independence / sharding along both axes, statistics against the Philox
kernel and the closed form, and the device-pointer entry.  Every launch has
valid arguments or is rejected on the host before the device is touched."""
import math

import numpy as np
import pytest

import mc_fixture as fx
import qmc_cases as qc
from finite_difference_amd import analytic, capi, mc_barrier, qmc
from finite_difference_amd.mc_barrier import MCConfig, price_discrete_barrier_mc

pytestmark = pytest.mark.gpu

CASES = fx.load_cases()
Z_TOL = 1e-13  # the project's bound for its normals (test_gpu_mc.py): the tails'
#                log and sqrt are within an ulp each, |y| <= 6.4


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
def _expected(n_obs, D, R, scramble, seed, stream, obs_first, rep_first):
    words = np.empty((R, n_obs, D.shape[0]), dtype=np.uint32)
    y = np.empty((R, n_obs, D.shape[0]))
    for k in range(R):
        words[k], y[k] = qmc.normals(n_obs, D, seed=seed, stream_id=stream,
                                     replicate=rep_first + k, scramble=scramble,
                                     obs_first=obs_first)
    return words, y


@pytest.mark.parametrize("n_dims", [1, 2, 3, 8, 64])
def test_generator_parity(n_dims):
    D = qmc.direction_numbers(n_dims)
    chunk = capi.mc_qmc_plan(n_dims, 1)["obs_per_block"]
    worst = 0.0
    for n_obs in (1, 255, 256, 257, chunk + 1):
        for R, rep_first, scramble in ((1, 0, False), (1, 3, True), (2, 0, True), (5, 3, True)):
            words, y = capi.qmc_normals(n_obs, D, R=R, scramble=scramble, seed=7, stream_id=2,
                                        rep_first=rep_first)
            want_w, want_y = _expected(n_obs, D, R, scramble, 7, 2, 0, rep_first)
            assert np.array_equal(words, want_w)
            worst = max(worst, float(np.max(np.abs(y - want_y))))
    print(f"n_dims {n_dims}: worst |dy| {worst:.3e}")
    assert worst <= Z_TOL


def test_generator_reaches_all_32_columns():
    """A synthetic table of random 32-bit words around observation 2^31: the
    top Gray-code bit and the two columns torch's 30-bit table leaves empty."""
    D = np.random.default_rng(32).integers(0, 2 ** 32, size=(5, 32), dtype=np.uint64)
    D = D.astype(np.uint32)
    first = 2 ** 31 - 100
    words, y = capi.qmc_normals(200, D, R=2, seed=11, stream_id=1, obs_first=first, rep_first=1)
    want_w, want_y = _expected(200, D, 2, True, 11, 1, first, 1)
    assert np.array_equal(words, want_w)
    assert np.max(np.abs(y - want_y)) <= Z_TOL
    plain, _ = capi.qmc_normals(200, D, R=1, scramble=False, obs_first=first)
    assert np.array_equal(plain[0], qmc.sobol_words(200, D, first))
    assert np.any(plain[0][100:] != qmc.sobol_words(100, D, 0))  # bit 31 of g is read


def test_generator_accepts_the_last_observation():
    D = qmc.direction_numbers(3)
    first = 2 ** 32 - 64
    words, _ = capi.qmc_normals(64, D, R=1, scramble=False, obs_first=first)
    assert np.array_equal(words[0], qmc.sobol_words(64, D, first))
    with pytest.raises(capi.FdcnError, match="obs_first"):
        capi.qmc_normals(65, D, R=1, scramble=False, obs_first=first)


# ---------------------------------------------------------------------------
# payoff parity with the host engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps,construction,antithetic", qc.parity_launches(),
                         ids=lambda v: str(v))
def test_payoff_parity_with_the_host_engine(n_steps, construction, antithetic):
    """Per observation |gpu - host| <= 1e-11 |host| + 1e-12 spot, no exclusions
    (test_qmc_host.py keeps every monitored spot 1e-9 away from its threshold).
    The bound is the existing kernel's: the normals agree to an ulp (central
    branch exactly), the table recurrence is the same IEEE operations, and the
    path differs through one device exp per step, 3 n_steps 2^-53 <= 2.2e-14
    relative at 64 steps."""
    plan = capi.mc_qmc_plan(n_steps, 1)
    print(f"instance qmc_path_kernel<{plan['threads']}, {str(antithetic).lower()}>")
    assert plan["obs_per_block"] == qc.chunk_of(n_steps)
    group = qc.parity_group(n_steps)
    n_obs = plan["obs_per_block"] + 257
    kw = dict(rng="sobol", seed=qc.PARITY_SEED, replicates=qc.PARITY_REPLICATES,
              construction=construction, want_payoffs=True)
    rep_g, pay_g = mc_barrier.simulate(group, n_obs, antithetic, engine="hip", **kw)
    rep_h, pay_h = mc_barrier.simulate(group, n_obs, antithetic, engine="host", **kw)
    assert pay_g.shape == pay_h.shape == (len(group), qc.PARITY_REPLICATES, n_obs)
    spot = np.array([c.params[capi.MC_P_SPOT] for c in group])[:, None, None]
    err = np.abs(pay_g - pay_h)
    bound = 1e-11 * np.abs(pay_h) + 1e-12 * spot
    k = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"worst payoff error {err.max():.3e}; closest to its bound at contract {k[0]}: "
          f"{err[k]:.3e} of {bound[k]:.3e}")
    assert np.all(err <= bound)
    # the sums of the payoffs: the per-observation bounds added up
    assert np.all(np.abs(rep_g[..., 0] - rep_h[..., 0])
                  <= 1e-11 * np.abs(rep_h[..., 0]) + 1e-12 * spot[:, :, 0] * n_obs)
    # the comparison is not of zeros: all but the six contracts that cannot pay
    # on a single monitor date (down-and-in calls, up-and-in puts) pay somewhere
    assert np.sum(pay_h.reshape(len(group), -1).max(axis=1) > 0.0) >= 24


# ---------------------------------------------------------------------------
# determinism and independence (bitwise)
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_batch():
    pool = qc.parity_group(8)
    return [pool[(7 * k) % len(pool)] for k in range(37)]


def _qmc(group, n_obs, **kw):
    P, F, S = mc_barrier._stack(group, kw.pop("stream_ids", list(range(len(group)))))
    dirnum, idx, bw = mc_barrier.qmc_tables(group, kw.pop("construction", "bridge"))
    return capi.mc_qmc_batch(P, F, S, n_obs, kw.pop("R", 2), True, dirnum, idx, bw,
                             want_payoffs=True, **kw)


def test_result_is_independent_of_the_batch(mixed_batch):
    assert {int(p.flags[capi.MC_F_KIND]) for p in mixed_batch} == {0, 1, 2, 3, 4}
    n_obs = qc.chunk_of(8) + 904
    alone = _qmc([mixed_batch[17]], n_obs, stream_ids=[17], seed=99)
    mixed = _qmc(mixed_batch, n_obs, seed=99)
    again = _qmc(mixed_batch, n_obs, seed=99)
    for a, m in zip(alone, mixed):
        assert np.array_equal(a[0], m[17])
    for m, g in zip(mixed, again):
        assert np.array_equal(m, g)
    other = _qmc([mixed_batch[17]], n_obs, stream_ids=[18], seed=99)
    assert not np.array_equal(other[2], alone[2])  # another stream id, another shift


def test_replicate_ranges_are_independent_replicates(mixed_batch):
    group, n_obs = mixed_batch[:6], qc.chunk_of(8) + 31
    _, whole, pay = _qmc(group, n_obs, R=5, seed=5)
    _, head, pay_h = _qmc(group, n_obs, R=2, seed=5, rep_first=0)
    _, tail, pay_t = _qmc(group, n_obs, R=3, seed=5, rep_first=2)
    assert np.array_equal(whole, np.concatenate([head, tail], axis=1))
    assert np.array_equal(pay, np.concatenate([pay_h, pay_t], axis=1))
    assert not np.array_equal(pay[:, 0], pay[:, 1])


def test_observation_ranges_continue_one_point_set(mixed_batch):
    group = [mixed_batch[3]]
    n, k = qc.chunk_of(8) + 1904, 1500
    assert k % qc.chunk_of(8) != 0
    stats, rep, pay = _qmc(group, n, R=3, seed=5, stream_ids=[4])
    _, rep_a, pay_a = _qmc(group, k, R=3, seed=5, stream_ids=[4])
    _, rep_b, pay_b = _qmc(group, n - k, R=3, seed=5, stream_ids=[4], obs_first=k)
    assert np.array_equal(pay[0], np.concatenate([pay_a[0], pay_b[0]], axis=1))
    parts = [(r, m, *part[0, r]) for part, m in ((rep_a, k), (rep_b, n - k)) for r in range(3)]
    merged = mc_barrier.merge_qmc_stats(parts)
    assert merged["replicates"] == 3 and merged["observations_per_replicate"] == n
    assert abs(merged["price"] - stats[0, 0]) <= 1e-14 * abs(stats[0, 0])
    # the device's own statistics are those of its replicate sums
    price, stderr, means = mc_barrier._qmc_stats(n, rep[0, :, 0])
    assert stats[0, 0] == price and abs(stats[0, 1] - stderr) <= 1e-12 * stderr
    assert stats[0, 2] == sum(means[1:], means[0])


def test_unshifted_run_is_one_replicate_with_zero_stderr(mixed_batch):
    group = mixed_batch[:4]
    stats, rep, pay = _qmc(group, 777, R=1, scramble=False)
    assert np.all(stats[:, 1] == 0.0) and rep.shape == (4, 1, 2)
    host = mc_barrier.simulate_qmc(group, 777, True, engine="host", replicates=1,
                                   scramble=False, want_payoffs=True)[1]
    spot = np.array([c.params[capi.MC_P_SPOT] for c in group])[:, None, None]
    assert np.all(np.abs(pay - host) <= 1e-11 * np.abs(host) + 1e-12 * spot)


# ---------------------------------------------------------------------------
# statistics against the Philox kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["large"], ids=lambda c: c["name"])
def test_statistics_against_philox_and_the_closed_form(case):
    """16 replicates x 2^14 points against a Philox run of the same total."""
    kw = fx.kwargs_for(case["inputs"], mc_barrier)
    kw["cfg"] = MCConfig(n_paths=2 * 16 * 2 ** 14, seed=7, antithetic=True)
    sob = price_discrete_barrier_mc(engine="hip", rng="sobol", **kw)
    phi = price_discrete_barrier_mc(engine="hip", rng="philox", **kw)
    print(f"{case['name']}: sobol {sob['price']:.6f} +- {sob['stderr']:.3e}  philox "
          f"{phi['price']:.6f} +- {phi['stderr']:.3e}  stderr ratio "
          f"{phi['stderr'] / sob['stderr']:.1f}")
    assert sob["replicates"] == 16 and sob["observations_per_replicate"] == 2 ** 14
    assert sob["n_observations"] == phi["n_observations"] == 16 * 2 ** 14
    assert abs(sob["price"] - phi["price"]) <= 5.0 * math.hypot(sob["stderr"], phi["stderr"])
    assert sob["stderr"] < phi["stderr"]
    inp = case["inputs"]
    if inp["barrier"]["type"] == "none" and not inp["dividends"]:
        r = math.log(1.0 + inp["rate"])  # flat NACA: DF = (1 + naca)^-tau
        bs = float(analytic.black_scholes("p" if inp["option_type"] == "put" else "c",
                                          inp["spot"], inp["strike"], r, r, inp["vol"],
                                          31 / 365.0))
        print(f"  closed form {bs:.6f} diff {sob['price'] - bs:.3e}")
        assert abs(sob["price"] - bs) <= 5.0 * sob["stderr"]


def test_batch_facade_shards_merge_to_the_whole_run():
    kws = []
    for case in CASES["large"]:
        kw = fx.kwargs_for(case["inputs"], mc_barrier)
        kw.pop("cfg")
        kws.append(kw)
    cfg = MCConfig(n_paths=2 * 4 * 3000, seed=3, antithetic=True)
    run = lambda **k: mc_barrier.mc_barrier_batch(kws, cfg, engine="hip", rng="sobol",  # noqa: E731
                                                  replicates=4, **k)
    whole = run()
    parts = [run(rep_range=range(0, 1)), run(rep_range=range(1, 4), obs_range=range(0, 1111)),
             run(rep_range=range(1, 4), obs_range=range(1111, 3000))]
    for b in range(len(kws)):
        merged = mc_barrier.merge_qmc_stats([p[b] for p in parts])
        assert abs(merged["price"] - whole[b]["price"]) <= 1e-14 * abs(whole[b]["price"])
        assert whole[b]["replicates"] == 4 and whole[b]["construction"] == "bridge"


# ---------------------------------------------------------------------------
# device-pointer entry
# ---------------------------------------------------------------------------
def test_dev_entry_matches_the_host_entry(mixed_batch):
    import torch
    group = mixed_batch[:9]
    B, R, n_obs = len(group), 3, qc.chunk_of(8) + 77
    P, F, S = mc_barrier._stack(group, list(range(B)))
    dirnum, idx, bw = mc_barrier.qmc_tables(group, "bridge")
    want, want_rep, want_pay = capi.mc_qmc_batch(P, F, S, n_obs, R, True, dirnum, idx, bw, seed=21,
                                                 rep_first=1, want_payoffs=True)
    dev = torch.device("cuda:0")
    dP, dF, dS, dW = (torch.from_numpy(a).to(dev) for a in (P, F, S, bw))
    dD = torch.from_numpy(dirnum.view(np.int32)).to(dev)  # the same 32-bit words
    stats = torch.zeros((B, capi.MC_NSTAT), dtype=torch.float64, device=dev)
    rep = torch.zeros((B, R, 2), dtype=torch.float64, device=dev)
    pay = torch.zeros((B, R, n_obs), dtype=torch.float64, device=dev)
    ws_bytes = capi.mc_qmc_plan(8, n_obs, R)["ws_bytes_per_contract"] * B
    canary = 64
    ws = torch.full((ws_bytes // 8 + canary,), -12345.0, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream

    def call(stats_t, rep_ptr, pay_ptr, ws_ptr, nbytes):
        capi.mc_qmc_batch_dev(B, 8, n_obs, R, True, True, dP.data_ptr(), dF.data_ptr(),
                              dS.data_ptr(), dD.data_ptr(), idx, dW.data_ptr(), 21, 0, 1,
                              stats_t.data_ptr(), rep_ptr, pay_ptr, ws_ptr, nbytes,
                              stream.cuda_stream)
    with torch.cuda.stream(stream):
        call(stats, rep.data_ptr(), pay.data_ptr(), ws.data_ptr(), ws_bytes)
    stream.synchronize()
    assert np.array_equal(stats.cpu().numpy(), want)
    assert np.array_equal(rep.cpu().numpy(), want_rep)
    assert np.array_equal(pay.cpu().numpy(), want_pay)
    tail = ws[ws_bytes // 8:].cpu().numpy()
    assert tail.shape == (canary,) and np.all(tail == -12345.0)  # nothing past the plan's size
    # library-owned scratch (NULL workspace) gives the same numbers
    stats2 = torch.zeros_like(stats)
    call(stats2, None, None, None, 0)
    stream.synchronize()
    assert np.array_equal(stats2.cpu().numpy(), want)
    # one byte short: refused on the host, nothing launched
    with pytest.raises(capi.FdcnError, match="workspace"):
        call(stats, None, None, ws.data_ptr(), ws_bytes - 1)
