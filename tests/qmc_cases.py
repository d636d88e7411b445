"""Contracts and launches shared by tests/test_qmc_host.py and
tests/test_gpu_qmc.py: synthetic McContracts on unequal step grids of any
length (the fixtures' dated trades stop at eight steps), the launches the GPU
payoff-parity test runs, and the walk that measures how close a monitored spot
comes to its threshold."""
import numpy as np

from finite_difference_amd import capi, mc_barrier, qmc

STEPS = (1, 2, 3, 5, 8, 13, 64)
CONSTRUCTIONS = ("bridge", "incremental")
PARITY_SEED = 20250728   # changed here if test_qmc_host's near-threshold check objects
PARITY_REPLICATES = 2
NEAR = 1e-9              # relative distance of a monitored spot from its threshold


def make_contract(n_steps, kind, put, div_mode, rebate_at_hit, seed, vol=0.25):
    """One contract on n_steps unequal steps over a quarter of a year.
    div_mode: None, "first" (dividend before the monitor test) or "last".
    Every second step and the last are monitored; a cash dividend of 0.75 falls
    on the middle step; a knock-out pays a rebate of 2."""
    rng = np.random.default_rng(seed)
    tau = rng.uniform(0.5, 1.5, n_steps)
    tau *= 0.25 / tau.sum()
    r = 0.05
    t_end = np.cumsum(tau)
    step = np.zeros((n_steps, capi.MC_NSTEP))
    step[:, capi.MC_S_DRIFT] = (r - 0.5 * vol * vol) * tau
    step[:, capi.MC_S_DIFF] = vol * np.sqrt(tau)
    if div_mode is not None:
        step[n_steps // 2, capi.MC_S_DIV] = 0.75
    mon = np.zeros(n_steps)
    mon[1::2] = 1.0
    mon[-1] = 1.0
    step[:, capi.MC_S_MONITOR] = mon
    df_T = float(np.exp(-r * t_end[-1]))
    at_hit = bool(rebate_at_hit and kind in (1, 2))
    step[:, capi.MC_S_DF_END] = np.where((mon != 0.0) & at_hit, np.exp(-r * t_end), df_T)
    spot = 100.0
    thr = {0: 0.0, 1: 94.0, 2: 106.0, 3: 94.0, 4: 106.0}[kind]
    params = np.array([spot, 103.0 if put else 97.0, df_T, thr, 2.0 if kind in (1, 2) else 0.0,
                       1e-12])
    flags = np.array([int(put), kind, int(at_hit), int(div_mode != "last"), 0], dtype=np.int32)
    name = mc_barrier._KINDS[kind]
    return mc_barrier.McContract(params=params, flags=flags, step=step, grid=[None] * (n_steps + 1),
                                 barrier_type=name, barrier_level=thr or None, band=0.0)


def parity_group(n_steps):
    """30 contracts on one grid length: every kind 0-4, put and call, without
    dividends and with them in both orders; the knock-outs alternate between
    the rebate at maturity and at the hit."""
    group = []
    for kind in range(5):
        for put in (False, True):
            for d, div_mode in enumerate((None, "first", "last")):
                group.append(make_contract(n_steps, kind, put, div_mode,
                                           rebate_at_hit=(d + put) % 2 == 0,
                                           seed=1000 * n_steps + len(group)))
    return group


def parity_launches():
    """(n_steps, construction, antithetic) of every GPU payoff-parity launch."""
    return [(n, c, a) for n in STEPS for c in CONSTRUCTIONS for a in (False, True)]


def chunk_of(n_steps):
    """Observations per workgroup: 256 x 16 up to 30 steps, 64 x 16 above (the
    library's fdcn_mc_qmc_plan; test_qmc_host checks this against it)."""
    return (256 if n_steps <= 30 else 64) * 16


def min_margin(c, dW, antithetic):
    """Smallest |s / threshold - 1| over the monitored steps of the paths with
    increments dW [n, n_steps] (and of their mirrors), walking as the engines
    do.  inf for a contract without a barrier."""
    kind = int(c.flags[capi.MC_F_KIND])
    if kind == 0:
        return np.inf
    spot, _, _, thr, _, floor = (float(v) for v in c.params)
    div_first = bool(c.flags[capi.MC_F_DIV_FIRST])
    worst = np.inf
    for sign in ((1.0, -1.0) if antithetic else (1.0,)):
        s = np.full(dW.shape[0], spot)
        for i in range(c.n_steps):
            s = s * np.exp(c.step[i, capi.MC_S_DRIFT] + sign * dW[:, i])
            div = float(c.step[i, capi.MC_S_DIV])
            if div_first and div != 0.0:
                s = np.maximum(s - div, floor)
            if c.step[i, capi.MC_S_MONITOR] != 0.0:
                worst = min(worst, float(np.min(np.abs(s / thr - 1.0))))
            if not div_first and div != 0.0:
                s = np.maximum(s - div, floor)
    return worst


def increments(c, n_obs, construction, seed, stream_id, replicate, obs_first=0):
    """dW [n_obs, n_steps] of one replicate of one contract, from qmc.py."""
    diff = c.step[:, capi.MC_S_DIFF]
    idx, w = qmc.bridge_plan(qmc.var_times(diff), construction, diff=diff)
    _, y = qmc.normals(n_obs, qmc.direction_numbers(c.n_steps), seed=seed, stream_id=stream_id,
                       replicate=replicate, obs_first=obs_first)
    return qmc.qmc_increments(y, idx, w)
