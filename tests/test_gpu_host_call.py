"""The host-array entry points of libfdcn stage their arrays through one helper
(csrc/fdcn_host_call.h: one stream-ordered block of 256-byte-aligned regions
on the calling thread's stream).  On the device:

* each host entry gives, bit for bit, what its `_dev` entry gives on the same
  arrays staged through torch -- at the smallest shapes at which staging can
  go wrong: region sizes that are no multiple of 256 B, every optional array
  present and absent, monitor arrays with and without entries, more than one
  workgroup with a partial one, an odd step count;
* the entry points test_gpu_boundary.test_host_entry_points_are_reentrant does
  not reach (closed forms, spot-space march, the three Monte Carlo engines)
  run from four threads at once and give the single-threaded results bitwise.

Compared elsewhere at such shapes, and not repeated here: the closed forms'
host against `_dev` entry at B = 257 (test_gpu_analytic_precision.py) and
fdcn_mc_normals against the documented mapping at n_obs = 4097, n_steps = 3
(test_gpu_mc.test_generator_parity).  IT solves take no monitors, so the
American march has the n_mon = 0 case only.  What no device test can reach --
a failed allocation, copy or launch -- is tests/test_host_call_driver.py's."""
import threading

import numpy as np
import pytest

import analytic_mp_fixture as afx
import bgk_fixture as bfx
import lsm_fixture as lf
import mc_fixture as mfx
import vc_cases as vc
from finite_difference_amd import bgk_barrier, capi, mc_american, mc_barrier
from finite_difference_amd.engine import pack
from plan_factory import random_solve

pytestmark = pytest.mark.gpu

N_OBS = 4097   # two workgroups of 4096 observations, the second with one
N_STEPS = 3    # odd: the last Philox pair's sine is dropped
SEED = 21


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


class Dev:
    """Host arrays staged through torch, a side stream for the `_dev` call."""

    def __init__(self):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda:0")
        self.stream = torch.cuda.Stream(device=self.dev)

    def put(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a if a.size else np.zeros(1, a.dtype)).to(self.dev)

    def zeros(self, *shape):
        return self.torch.zeros(shape, dtype=self.torch.float64, device=self.dev)

    @staticmethod
    def ptr(t):
        return None if t is None else t.data_ptr()

    def run(self, launch):
        self.torch.cuda.synchronize()  # the fills ran on the default stream
        launch(self.stream.cuda_stream)
        self.stream.synchronize()


# ---------------------------------------------------------------------------
# the log-spot march: cn (with and without monitors) and it
# ---------------------------------------------------------------------------
def _march_group(it, n_mon):
    rng = np.random.default_rng(5 + 2 * int(it) + n_mon)
    solves = [random_solve(rng, 131, 9, 2, it=it, ko=False) for _ in range(3)]
    if n_mon:
        solves[1].ko_lo, solves[1].mon_steps, solves[1].mon_rebates = 20, [3, 7], [0.0, 1.5]
    g = pack(solves, [0, 1, 2])
    assert g.B == 3 and len(g.mon_step) == n_mon and (8 * g.B * g.n_nodes) % 256 != 0
    return g


@pytest.mark.parametrize("it,n_mon", [(False, 0), (False, 2), (True, 0)],
                         ids=["cn", "cn_mon2", "it"])
def test_march_host_entry_is_the_dev_entry_bitwise(it, n_mon):
    g = _march_group(it, n_mon)
    if it:
        want = capi.it_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                             g.payoff)
    else:
        want = capi.cn_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                             g.mon_step, g.mon_rebate)
    d = Dev()
    P, I, V, F = d.put(g.params), d.put(g.iparams), d.put(g.v_init), d.put(g.payoff)
    MS, MR = d.put(g.mon_step), d.put(g.mon_rebate)
    out = d.zeros(g.B, g.n_nodes)
    k_cap = capi.sm_extent(g.n_nodes, g.n_time, g.n_ranna, g.params)
    ws_bytes = capi.plan(g.n_nodes, it, k_cap, n_time=g.n_time, B=g.B)["ws_bytes_per_scen"] * g.B
    ws = d.zeros(ws_bytes // 8 + 1)
    if it:
        d.run(lambda s: capi.it_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, P.data_ptr(),
                                          I.data_ptr(), V.data_ptr(), F.data_ptr(),
                                          out.data_ptr(), k_cap, ws.data_ptr(), ws_bytes, s))
    else:
        d.run(lambda s: capi.cn_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, P.data_ptr(),
                                          I.data_ptr(), V.data_ptr(), n_mon, MS.data_ptr(),
                                          MR.data_ptr(), out.data_ptr(), k_cap, ws.data_ptr(),
                                          ws_bytes, s))
    assert _same(out.cpu().numpy(), want)
    assert not _same(want, g.v_init)  # the march ran


# ---------------------------------------------------------------------------
# the spot-space march
# ---------------------------------------------------------------------------
VC_NODES = 257  # the smallest variant's 256 slots plus node 0 outside them


def _vc_group(n_time):
    g = vc.small_grids(VC_NODES)            # 17 steps; rows 1 and 3 carry monitors
    if n_time:
        return vc.take(g, [0, 1, 2])
    import dataclasses
    g = vc.take(g, [0, 2, 0])               # no step: no boundary values, no monitors
    return dataclasses.replace(g, n_time=0, n_ranna=0, bnd=np.zeros((3, 0, 2)),
                               mon_step=np.zeros(0, np.int32), mon_rebate=np.zeros(0))


def _vc_host(g):
    return capi.vc_batch(g.n_nodes, g.n_time, g.n_ranna, g.diag, g.bnd, g.v_init, g.iparams,
                         g.mon_step, g.mon_rebate)


@pytest.mark.parametrize("n_time", [0, 17])
def test_vc_host_entry_is_the_dev_entry_bitwise(n_time):
    g = _vc_group(n_time)
    assert g.B == 3 and g.n_time == n_time and (8 * g.B * g.n_nodes) % 256 != 0
    assert capi.vc_variant_name(g.n_nodes, B=g.B) == "fdcn_vc_march<1,4>"
    want = _vc_host(g)
    d = Dev()
    D, Bd, V, I = d.put(g.diag), d.put(g.bnd), d.put(g.v_init), d.put(g.iparams)
    MS, MR = d.put(g.mon_step), d.put(g.mon_rebate)
    out = d.zeros(g.B, g.n_nodes)
    d.run(lambda s: capi.vc_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, D.data_ptr(),
                                      Bd.data_ptr(), V.data_ptr(), I.data_ptr(), len(g.mon_step),
                                      MS.data_ptr(), MR.data_ptr(), out.data_ptr(), None, 0, s))
    assert _same(out.cpu().numpy(), want)
    if n_time:
        assert len(g.mon_step) > 0 and not _same(want, g.v_init)


# ---------------------------------------------------------------------------
# the Monte Carlo engines
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mc_inputs():
    """Two contracts of the eight-step fixtures, cut to three steps (a step
    row stands alone), and normals for the supplied-z case."""
    cases = [c for c in mfx.load_cases()["small"] if c["result"]["steps"] == 8][:2]
    plans = [mc_barrier.plan_contract(**mfx.kwargs_for(c["inputs"], mc_barrier)) for c in cases]
    P, F, S = mc_barrier._stack(plans, [0, 1])
    z = np.random.default_rng(3).standard_normal((N_OBS, N_STEPS))
    return P, F, np.ascontiguousarray(S[:, :N_STEPS]), z


@pytest.mark.parametrize("pay", [False, True], ids=["stats", "payoffs"])
@pytest.mark.parametrize("supplied", [False, True], ids=["philox", "z"])
def test_mc_host_entry_is_the_dev_entry_bitwise(mc_inputs, supplied, pay):
    P, F, S, z = mc_inputs
    z = z if supplied else None
    B = P.shape[0]
    got = capi.mc_barrier_batch(P, F, S, N_OBS, True, z=z, seed=SEED, want_payoffs=pay)
    want_stats, want_pay = got if pay else (got, None)
    d = Dev()
    dP, dF, dS, dZ = d.put(P), d.put(F), d.put(S), d.put(z)
    stats, payoff = d.zeros(B, capi.MC_NSTAT), d.zeros(B, N_OBS) if pay else None
    ws_bytes = capi.mc_plan(N_OBS)["ws_bytes_per_contract"] * B
    ws = d.zeros(ws_bytes // 8) if pay else None  # without: the library's own scratch
    d.run(lambda s: capi.mc_barrier_batch_dev(
        B, N_STEPS, N_OBS, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), d.ptr(dZ), SEED, 0,
        stats.data_ptr(), d.ptr(payoff), d.ptr(ws), ws_bytes if pay else 0, s))
    assert _same(stats.cpu().numpy(), want_stats)
    if pay:
        assert _same(payoff.cpu().numpy(), want_pay)


@pytest.fixture(scope="module")
def bgk_inputs():
    """Two trades x two Greeks scenarios of the seven-step fixtures, cut to
    three steps."""
    cases = bfx.load_cases()
    groups = []
    for name in ("uo_call_smooth_7", "dbl_out_call_smooth_rebate_hit_7"):
        case = next(c for c in cases["paths"] + cases["closed"] if c["name"] == name)
        p = bgk_barrier.DiscreteBarrierBGKPricer(engine="hip", **bfx.kwargs_for(case["inputs"]))
        groups.append([j.plan for j in p._bumped_jobs(1e-4 * p.spot_price, 1e-4)][:2])
    P = np.stack([np.stack([p.params for p in grp]) for grp in groups])
    S = np.stack([np.stack([p.step[:N_STEPS] for p in grp]) for grp in groups])
    F = np.stack([grp[0].flags for grp in groups]).astype(np.int32)
    F[:, capi.BGK_F_STREAM] = np.arange(len(groups))
    z = np.random.default_rng(4).standard_normal((N_OBS, N_STEPS))
    return P, F, np.ascontiguousarray(S), z


@pytest.mark.parametrize("pay", [False, True], ids=["stats", "payoffs"])
@pytest.mark.parametrize("supplied", [False, True], ids=["philox", "z"])
def test_bgk_host_entry_is_the_dev_entry_bitwise(bgk_inputs, supplied, pay):
    P, F, S, z = bgk_inputs
    z = z if supplied else None
    B, G = P.shape[:2]
    assert (B, G, S.shape[2]) == (2, 2, N_STEPS)
    got = capi.mc_bgk_batch(P, F, S, N_OBS, True, z=z, seed=SEED, want_payoffs=pay)
    want_stats, want_pay = got if pay else (got, None)
    d = Dev()
    dP, dF, dS, dZ = d.put(P), d.put(F), d.put(S), d.put(z)
    stats = d.zeros(B, G, capi.BGK_NSTAT)
    payoff = d.zeros(B, G, 2, 2 * N_OBS) if pay else None
    ws_bytes = capi.mc_bgk_plan(N_OBS, G)["ws_bytes_per_trade"] * B
    ws = d.zeros(ws_bytes // 8) if pay else None
    d.run(lambda s: capi.mc_bgk_batch_dev(
        B, G, N_STEPS, N_OBS, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), d.ptr(dZ), SEED,
        0, stats.data_ptr(), d.ptr(payoff), d.ptr(ws), ws_bytes if pay else 0, s))
    assert _same(stats.cpu().numpy(), want_stats)
    if pay:
        assert _same(payoff.cpu().numpy(), want_pay)


LSM_STEPS, LSM_G = 4, 2


@pytest.fixture(scope="module")
def lsm_inputs():
    t4 = [0.1, 0.2, 0.35, 0.5]
    plans = lf.plan_batch([
        lf._contract("up-and-out", "put", t4, (1, 3), range(4), rebate=1.0, at_hit=True),
        lf._contract("none", "call", t4, (), (1, 3))])
    return mc_american._stack(plans, [5, 6])


@pytest.mark.parametrize("values,coef", [(False, False), (True, True), (True, False),
                                         (False, True)],
                         ids=["stats", "both_dumps", "values", "coef"])
def test_lsm_host_entry_is_the_dev_entry_bitwise(lsm_inputs, values, coef):
    P, F, S = lsm_inputs
    B = P.shape[0]
    assert (B, S.shape[1]) == (2, LSM_STEPS)
    want_stats, want_val, want_coef = capi.mc_lsm_batch(
        P, F, S, LSM_G, True, seed=SEED, want_values=values, want_coef=coef)
    plan = capi.mc_lsm_plan(LSM_STEPS, LSM_G, True)
    d = Dev()
    dP, dF, dS = d.put(P), d.put(F), d.put(S)
    stats = d.zeros(B, capi.LSM_NSTAT)
    val = d.zeros(B, plan["values_per_contract"]) if values else None
    cf = d.zeros(B, plan["coef_per_contract"]) if coef else None
    ws_bytes = plan["ws_bytes_per_contract"] * B
    ws = d.zeros(ws_bytes // 8) if values else None
    d.run(lambda s: capi.mc_lsm_batch_dev(
        B, LSM_STEPS, LSM_G, True, dP.data_ptr(), dF.data_ptr(), dS.data_ptr(), SEED, 0,
        stats.data_ptr(), d.ptr(val), d.ptr(cf), d.ptr(ws), ws_bytes if values else 0, s))
    assert _same(stats.cpu().numpy(), want_stats)
    if values:
        assert _same(val.cpu().numpy(), want_val)
    if coef:
        assert _same(cf.cpu().numpy().reshape(want_coef.shape), want_coef)


# ---------------------------------------------------------------------------
# reentrancy
# ---------------------------------------------------------------------------
def _closed_form_rows(engine, B=257):
    fix = afx.load()
    P = np.concatenate([afx.arrays(g)[0] for g in fix[engine]])
    F = np.concatenate([afx.arrays(g)[1] for g in fix[engine]])
    idx = np.arange(B) % len(P)
    return np.ascontiguousarray(P[idx]), np.ascontiguousarray(F[idx])


def test_the_other_host_entry_points_are_reentrant(mc_inputs, bgk_inputs, lsm_inputs):
    """Four threads in one process, each calling its entry points five times
    (own stream, pooled block): every result equals the single-threaded one
    bitwise.  The closed forms used to synchronise the whole device here."""
    rrP, rrF = _closed_form_rows("single")
    dbP, dbF = _closed_form_rows("double")
    g = _vc_group(17)
    mP, mF, mS, mz = mc_inputs
    bP, bF, bS, _ = bgk_inputs
    lP, lF, lS = lsm_inputs
    calls = {
        "rr": lambda: capi.rr_barrier_batch(rrP, rrF),
        "double": lambda: (capi.double_barrier_batch(dbP, dbF, 4),),
        "vc": lambda: (_vc_host(g),),
        "mc": lambda: capi.mc_barrier_batch(mP, mF, mS, N_OBS, True, z=mz, seed=SEED,
                                            want_payoffs=True),
        "bgk": lambda: capi.mc_bgk_batch(bP, bF, bS, N_OBS, True, seed=SEED, want_payoffs=True),
        "lsm": lambda: capi.mc_lsm_batch(lP, lF, lS, LSM_G, True, seed=SEED, want_values=True,
                                         want_coef=True),
    }
    names = list(calls)
    single = {n: calls[n]() for n in names}
    errors = []

    def work(t):
        try:
            for n in names[t::4]:
                for _ in range(5):
                    for a, b in zip(calls[n](), single[n]):
                        if not _same(a, b):
                            errors.append(f"thread {t}: {n} differs")
        except Exception as e:  # pragma: no cover - reported below
            errors.append(f"thread {t}: {e!r}")

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a thread hung"
    assert not errors, errors
