"""Quasi-Monte Carlo on the host: qmc.py (the NumPy restatement of the
generator contract of include/fdcn.h) against torch's Sobol engine and
CPython's inverse normal CDF, the path-construction tables, the host engine
under rng="sobol", the guard that lets the GPU parity test allow no
exclusions, and the library's argument validation (which returns before any
device call, so it runs without a GPU)."""
import ctypes
import math
import statistics

import numpy as np
import pytest

import mc_fixture as fx
import qmc_cases as qc
from finite_difference_amd import analytic, capi, mc_barrier, qmc
from finite_difference_amd.mc_barrier import MCConfig, price_discrete_barrier_mc

CASES = fx.load_cases()
Z_TOL = 1e-13  # the project's bound for its normals (test_gpu_mc.py)


# ---------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 8, 64])
def test_sobol_words_are_torchs_unscrambled_draws(d):
    import torch
    n = 1025
    got = qmc.sobol_words(n, qmc.direction_numbers(d)).astype(np.float64) * 2.0 ** -32
    want = torch.quasirandom.SobolEngine(d, scramble=False).draw(n, dtype=torch.float64).numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want)


def test_sobol_words_continue_from_an_offset():
    D = qmc.direction_numbers(5)
    whole = qmc.sobol_words(700, D)
    assert np.array_equal(qmc.sobol_words(300, D, obs_first=400), whole[400:])
    assert qmc.direction_numbers(5).dtype == np.uint32 and not D[:, 30:].any()


def test_digital_shifts_are_philox_words():
    s = qmc.digital_shifts(3, [0, 4], seed=7 + (9 << 32), stream_id=2)
    assert s.shape == (2, 3) and s.dtype == np.uint32
    for k, rho in enumerate((0, 4)):
        for j in range(3):
            x0 = fx.philox(j, rho, 0, 2, 7, 9)[0]
            assert int(s[k, j]) == int(x0)
    assert len({int(v) for v in s.ravel()}) == 6


def test_as241_matches_cpythons_inverse_cdf():
    nd = statistics.NormalDist()
    e25 = math.exp(-25.0)
    u = np.concatenate([
        [0.075, 0.925, np.nextafter(0.075, 0.0), np.nextafter(0.925, 1.0),
         np.nextafter(0.075, 1.0), np.nextafter(0.925, 0.0),
         e25, np.nextafter(e25, 0.0), np.nextafter(e25, 1.0), e25 * 0.5, e25 * 2.0,
         1.0 - 2.0 * e25, 2.0 ** -33, 1.0 - 2.0 ** -33, 0.5],
        np.random.default_rng(241).random(1000)])
    got = qmc.as241(u)
    want = np.array([nd.inv_cdf(float(x)) for x in u])
    worst = float(np.max(np.abs(got - want)))
    print(f"as241: worst |dz| {worst:.3e} over {u.size} inputs")
    assert worst <= Z_TOL
    central = np.abs(u - 0.5) <= 0.425
    assert central.sum() > 800 and (~central).sum() > 100
    assert np.array_equal(got[central], want[central])  # no transcendental there
    # the 32-bit uniforms never reach the far tail (r > 5 needs u < exp(-25))
    assert qmc.uniforms(np.array([0], dtype=np.uint32))[0] == 2.0 ** -33 > e25
    assert 1.0 - qmc.uniforms(np.array([0xFFFFFFFF], dtype=np.uint32))[0] == 2.0 ** -33
    with pytest.raises(ValueError):
        qmc.as241([0.0])


# ---------------------------------------------------------------------------
# path-construction tables
# ---------------------------------------------------------------------------
def _check_with_library(idx):
    """The library's own table check, reached through a call that is otherwise
    valid: past validation it fails for want of a device (or runs, on a GPU)."""
    rc, msg = _raw(bridge_idx=idx, n_steps=idx.shape[0])
    return rc, msg


def _linear_map(idx, w):
    """A [n + 1, n]: W = A y, built row by row from the table."""
    n = idx.shape[0]
    A = np.zeros((n + 1, n))
    for j in range(n):
        t, l, r = (int(v) for v in idx[j])
        A[t] = w[j, 0] * A[l] + w[j, 1] * A[r]
        A[t, j] += w[j, 2]
    return A


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13, 64])
def test_bridge_plan_reproduces_brownian_covariance(n):
    diff = 0.25 * np.sqrt(np.random.default_rng(n).uniform(0.2, 2.0, n) / n)
    t = qmc.var_times(diff)
    assert t[0] == 0.0 and t.shape == (n + 1,)
    want = np.minimum.outer(t[1:], t[1:])
    cov = {}
    for construction in qc.CONSTRUCTIONS:
        idx, w = qmc.bridge_plan(t, construction, diff=diff)
        assert idx.shape == (n, 3) and idx.dtype == np.int32 and w.shape == (n, 3)
        assert sorted(idx[:, 0].tolist()) == list(range(1, n + 1))
        qmc.check_table(idx)
        rc, msg = _check_with_library(idx)
        assert rc in (0, -3), (rc, msg)  # FDCN_OK or FDCN_ENODEV: the table passed
        A = _linear_map(idx, w)
        cov[construction] = (A @ A.T)[1:, 1:]
        err = np.max(np.abs(cov[construction] - want) / want)
        print(f"n={n} {construction}: worst relative covariance error {err:.2e}")
        assert err <= 1e-12
    assert np.max(np.abs(cov["bridge"] - cov["incremental"]) / want) <= 1e-12
    # the order depends on n only
    other, _ = qmc.bridge_plan(qmc.var_times(diff[::-1] * 3.0))
    assert np.array_equal(other, qmc.bridge_plan(t)[0])
    assert tuple(qmc.bridge_plan(t)[0][0]) == (n, 0, 0)


def test_zero_vol_contract_has_zero_weights_and_a_deterministic_price():
    kw = fx.kwargs_for(CASES["large"][0]["inputs"], mc_barrier)
    kw["vol"] = 0.0
    kw["cfg"] = MCConfig(n_paths=2 * 4 * 64, seed=3, antithetic=True)
    plan = mc_barrier.plan_contract(**kw)
    for construction in qc.CONSTRUCTIONS:
        _, _, bw = mc_barrier.qmc_tables([plan], construction)
        assert np.all(bw[0][:, 2] == 0.0) and np.all(np.isfinite(bw))
        if construction == "bridge":
            assert np.all(bw[0][1:] == (1.0, 0.0, 0.0))
        out = price_discrete_barrier_mc(engine="host", rng="sobol", replicates=4,
                                        construction=construction, **kw)
        assert math.isfinite(out["price"]) and out["stderr"] == 0.0
        assert len(set(out["rep_sum_p"])) == 1


# ---------------------------------------------------------------------------
# the host engine
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large_runs():
    """(case, sobol result, philox result): 16 replicates x 2^12 points against
    Philox on the same total number of paths, host engine."""
    runs = []
    for case in CASES["large"]:
        kw = fx.kwargs_for(case["inputs"], mc_barrier)
        kw["cfg"] = MCConfig(n_paths=2 * 16 * 2 ** 12, seed=7, antithetic=True)
        runs.append((case, price_discrete_barrier_mc(engine="host", rng="sobol", **kw),
                     price_discrete_barrier_mc(engine="host", rng="philox", **kw)))
    return runs


def test_host_engine_on_the_large_cases(large_runs):
    vanilla = 0
    for case, sob, phi in large_runs:
        ratio = phi["stderr"] / sob["stderr"]
        print(f"{case['name']}: sobol {sob['price']:.6f} +- {sob['stderr']:.2e}  philox "
              f"{phi['price']:.6f} +- {phi['stderr']:.2e}  stderr ratio {ratio:.1f}")
        assert sob["replicates"] == 16 and sob["construction"] == "bridge"
        assert sob["observations_per_replicate"] == 2 ** 12
        assert sob["n_observations"] == phi["n_observations"] == 16 * 2 ** 12
        assert len(sob["rep_sum_p"]) == len(sob["rep_sum_p2"]) == 16
        assert set(case["result"]) <= set(sob)
        assert sob["stderr"] < phi["stderr"]
        inp = case["inputs"]
        if inp["barrier"]["type"] == "none" and not inp["dividends"]:
            vanilla += 1
            r = math.log(1.0 + inp["rate"])
            bs = float(analytic.black_scholes("p" if inp["option_type"] == "put" else "c",
                                              inp["spot"], inp["strike"], r, r, inp["vol"],
                                              31 / 365.0))
            print(f"  closed form {bs:.6f} diff {sob['price'] - bs:.3e}")
            assert abs(sob["price"] - bs) <= 5.0 * sob["stderr"]
    assert vanilla >= 1


def test_merge_qmc_stats_by_replicate_and_by_observation(large_runs):
    case, whole, _ = large_runs[0]
    kw = fx.kwargs_for(case["inputs"], mc_barrier)
    cfg = MCConfig(n_paths=2 * 16 * 2 ** 12, seed=7, antithetic=True)
    kw.pop("cfg")
    run = lambda **k: mc_barrier.mc_barrier_batch([kw], cfg, engine="host", rng="sobol",  # noqa: E731
                                                  stream_ids=[0], **k)[0]
    parts = [run(rep_range=range(0, 5)), run(rep_range=range(5, 16), obs_range=range(0, 1000)),
             run(rep_range=range(5, 16), obs_range=range(1000, 2 ** 12))]
    merged = mc_barrier.merge_qmc_stats(parts)
    assert merged["replicates"] == 16 and merged["observations_per_replicate"] == 2 ** 12
    assert abs(merged["price"] - whole["price"]) <= 1e-13 * abs(whole["price"])
    assert abs(merged["stderr"] - whole["stderr"]) <= 1e-9 * whole["stderr"]
    with pytest.raises(ValueError):
        mc_barrier.merge_qmc_stats(parts[:2])  # replicates of different lengths
    with pytest.raises(ValueError):
        run(obs_range=range(0, 2 ** 12 + 1))
    with pytest.raises(ValueError):
        price_discrete_barrier_mc(engine="host", rng="sobol", replicates=1, cfg=cfg, **kw)


def test_facade_rejects_points_beyond_the_table():
    c = qc.make_contract(2, 0, False, None, False, 1)
    with pytest.raises(ValueError, match="2\\^30"):
        mc_barrier.simulate([c], 8, False, engine="host", rng="sobol", obs_first=2 ** 30 - 7)
    with pytest.raises(ValueError, match="construction"):
        mc_barrier.simulate([c], 8, False, engine="host", rng="sobol", construction="spiral")


# ---------------------------------------------------------------------------
# what lets the GPU payoff parity allow no exclusions
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_steps", qc.STEPS)
def test_no_parity_path_sits_on_its_threshold(n_steps):
    """For every launch of test_gpu_qmc's payoff parity: no monitored spot
    within 1e-9 relative of the threshold, so an ulp of the device's exp cannot
    flip a barrier test.  If this fails, change qmc_cases.PARITY_SEED."""
    assert capi.mc_qmc_plan(n_steps, 1)["obs_per_block"] == qc.chunk_of(n_steps)
    n_obs = qc.chunk_of(n_steps) + 257
    group = qc.parity_group(n_steps)
    worst = np.inf
    for construction in qc.CONSTRUCTIONS:
        for b, c in enumerate(group):
            if int(c.flags[capi.MC_F_KIND]) == 0:
                continue
            for rho in range(qc.PARITY_REPLICATES):
                dW = qc.increments(c, n_obs, construction, qc.PARITY_SEED, b, rho)
                worst = min(worst, qc.min_margin(c, dW, True))
    print(f"n_steps {n_steps}: closest monitored spot {worst:.3e} from its threshold")
    assert worst > qc.NEAR


# ---------------------------------------------------------------------------
# library validation: before any device call
# ---------------------------------------------------------------------------
EINVAL, ENODEV = -1, -3


def _raw(*, B=1, n_steps=3, n_obs=100, R=2, antithetic=1, scramble=1, obs_first=0, rep_first=0,
         bridge_idx=None, null=(), kind=1, spot=100.0, bridge_w=None, dev=False, ws_bytes=None):
    """fdcn_mc_qmc_batch[_dev] straight through ctypes with one thing wrong."""
    n = max(1, n_steps)
    c = qc.make_contract(min(n, 64), kind if 0 <= kind <= 4 else 1, False, None, False, 5)
    P = np.tile(c.params, (max(B, 1), 1))
    P[:, capi.MC_P_SPOT] = spot
    F = np.tile(c.flags, (max(B, 1), 1)).astype(np.int32)
    F[:, capi.MC_F_KIND] = kind
    S = np.tile(c.step, (max(B, 1), 1, 1))
    D = np.ones((n, 32), dtype=np.uint32)
    idx, w = qmc.bridge_plan(qmc.var_times(c.step[:, capi.MC_S_DIFF]))
    X = np.ascontiguousarray(idx if bridge_idx is None else bridge_idx, dtype=np.int32)
    W = np.tile(w, (max(B, 1), 1, 1)) if bridge_w is None else np.asarray(bridge_w, dtype=float)
    stats = np.zeros((max(B, 1), 4))
    arrays = dict(params=P, flags=F, step=S, dirnum=D, bridge_idx=X, bridge_w=W, stats=stats)
    ptr = {k: (None if k in null else v.ctypes.data) for k, v in arrays.items()}
    L = capi.lib()
    args = [B, n_steps, n_obs, R, antithetic, scramble, ptr["params"], ptr["flags"], ptr["step"],
            ptr["dirnum"], ptr["bridge_idx"], ptr["bridge_w"], 7, obs_first, rep_first,
            ptr["stats"], None, None]
    if dev:
        # host memory stands in for device memory: validation reads none of it
        # and a short workspace is refused before anything is launched
        need = capi.mc_qmc_plan(n_steps, n_obs, R)["ws_bytes_per_contract"] * B
        ws = np.zeros(need // 8 + 1)
        rc = L.fdcn_mc_qmc_batch_dev(*args, ws.ctypes.data, need - 1 if ws_bytes is None
                                     else ws_bytes, None)
    else:
        rc = L.fdcn_mc_qmc_batch(*args)
    return rc, L.fdcn_last_error().decode()


BAD_ARGUMENTS = [
    (dict(B=0), "B"), (dict(n_obs=0), "n_obs"), (dict(R=0), "R"),
    (dict(n_steps=0), "n_steps"), (dict(n_steps=65), "n_steps"),
    (dict(antithetic=2), "antithetic"), (dict(antithetic=-1), "antithetic"),
    (dict(scramble=2), "scramble"), (dict(scramble=-1), "scramble"),
    (dict(scramble=0, R=2), "scramble"),
    (dict(obs_first=-1), "obs_first"), (dict(obs_first=2 ** 32 - 99), "obs_first"),
    (dict(rep_first=-1), "rep_first"),
    (dict(null=("params",)), "params"), (dict(null=("flags",)), "flags"),
    (dict(null=("step",)), "step"), (dict(null=("dirnum",)), "dirnum"),
    (dict(null=("bridge_idx",)), "bridge_idx"), (dict(null=("bridge_w",)), "bridge_w"),
    (dict(null=("stats",)), "stats"),
    (dict(dev=True), "workspace"),
    (dict(kind=5), "kind"), (dict(spot=0.0), "spot"),
    (dict(bridge_w=np.full((1, 3, 3), np.nan)), "bridge_w"),
    (dict(bridge_w=np.full((1, 3, 3), np.inf)), "bridge_w"),
]


@pytest.mark.parametrize("kw,word", BAD_ARGUMENTS, ids=[f"{w}-{i}" for i, (_, w)
                                                        in enumerate(BAD_ARGUMENTS)])
def test_library_rejects_bad_arguments(kw, word):
    rc, msg = _raw(**kw)
    assert rc == EINVAL and word in msg and msg.startswith("mc_qmc_batch"), (rc, msg)


BAD_TABLES = {
    "duplicate target": [[3, 0, 0], [1, 0, 3], [1, 0, 3]],
    "target 0": [[3, 0, 0], [0, 0, 3], [2, 1, 3]],
    "target above n": [[4, 0, 0], [1, 0, 3], [2, 1, 3]],
    "undefined left": [[3, 0, 0], [2, 1, 3], [1, 0, 2]],
    "left not below target": [[3, 0, 0], [1, 3, 3], [2, 1, 3]],
    "negative left": [[3, 0, 0], [1, -1, 3], [2, 1, 3]],
    "right between left and target": [[1, 0, 0], [3, 0, 1], [2, 1, 3]],
    "right inside": [[3, 0, 0], [2, 0, 1], [1, 0, 2]],
    "undefined right": [[2, 0, 0], [1, 0, 3], [3, 2, 2]],
    "right above n": [[3, 0, 0], [1, 0, 4], [2, 1, 3]],
}


@pytest.mark.parametrize("dev", [False, True], ids=["host", "dev"])
@pytest.mark.parametrize("name", sorted(BAD_TABLES))
def test_library_rejects_malformed_tables(name, dev):
    rc, msg = _raw(bridge_idx=np.array(BAD_TABLES[name]), dev=dev, ws_bytes=1 << 20)
    assert rc == EINVAL and "bridge_idx row" in msg, (name, rc, msg)


def test_library_accepts_valid_arguments_until_the_device():
    """Past validation the host entry needs a device: FDCN_ENODEV here, FDCN_OK
    on a GPU host.  obs_first + n_obs = 2^32 exactly is inside the range."""
    for kw in (dict(), dict(scramble=0, R=1), dict(obs_first=2 ** 32 - 100),
               dict(n_steps=64), dict(bridge_idx=np.array([[1, 0, 0], [2, 1, 1], [3, 2, 2]]))):
        rc, msg = _raw(**kw)
        assert rc in (0, ENODEV), (kw, rc, msg)
    p = capi.mc_qmc_plan(64, 5000, 3)
    assert p["obs_per_block"] == 1024 and p["blocks_per_replicate"] == 5 and p["threads"] == 64
    assert p["ws_bytes_per_contract"] == (3 * 5 * 2 + 3) * 8
    assert capi.mc_qmc_plan(30, 4097)["blocks_per_replicate"] == 2
    assert capi.mc_qmc_plan(31, 1)["threads"] == 64
    with pytest.raises(capi.FdcnError, match="n_steps"):
        capi.mc_qmc_plan(65, 10)


def test_existing_generators_are_untouched():
    """rng="philox" and rng="numpy" run the code they ran before."""
    case = CASES["small"][0]
    kw = fx.kwargs_for(case["inputs"], mc_barrier)
    out = price_discrete_barrier_mc(engine="host", rng="numpy", **kw)
    assert abs(out["price"] - case["result"]["price"]) <= 1e-12 * case["result"]["price"]
    assert sorted(out) == sorted(case["result"])
    with pytest.raises(ValueError, match="rng"):
        price_discrete_barrier_mc(engine="host", rng="halton", **kw)
