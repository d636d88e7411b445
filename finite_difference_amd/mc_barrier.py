"""Monte Carlo pricer for discretely monitored single-barrier options.

The independent cross-check of the FD barrier engines, with the reference's
names and signatures (mc_discrete_barrier_option.py): cash dividends on the
path, carry per interval from the forward curve, the barrier test with a
basis-point band, a rebate discounted from its own hit date.

The host side builds the event grid and the per-step arrays in the
reference's operation order (:193-222, :268-293); the paths run

* ``engine="hip"``: in libfdcn's path kernel (csrc/fdcn_mc.hip) -- B contracts
  per launch, normals generated on the device (``rng="philox"``, the default
  there) or handed over (``rng="numpy"``: ``default_rng(seed)`` chunk by chunk
  as the reference draws them, which reproduces its numbers);
* ``engine="host"``: in NumPy, in the reference's operation order -- the CPU
  fallback and the timed CPU baseline.  ``rng="philox"`` restates the device
  generator in NumPy (philox_normals), so both engines can run one stream.

``rng="sobol"`` (either engine) replaces the pseudo-random normals by
quasi-Monte Carlo points: `replicates` digitally shifted copies of one Sobol
point set, inverse-CDF normals, laid onto the path through a Brownian bridge
(``construction="bridge"``) or step by step (``"incremental"``) -- qmc.py and
csrc/fdcn_mc_qmc.hip, the contract in include/fdcn.h.  The standard error is
that of the replicate means.  ``cfg.n_paths`` stays the total.

A missing GPU under ``engine="hip"`` is an error, never a silent fallback.
"""
from __future__ import annotations

import datetime as dt
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import capi, market, qmc

_KINDS = ("none", "down-and-out", "up-and-out", "down-and-in", "up-and-in")
_DOWN = ("down-and-out", "down-and-in")
_OUT = ("down-and-out", "up-and-out")


class NacaCurve:
    """Daily NACA curve with exact-date lookup: a DataFrame with a date column
    (anything pandas parses) and a numeric NACA column.
    DF(valuation, d) = (1 + NACA(d)) ** -tau(valuation, d)."""

    def __init__(self, discount_curve_df, valuation_date: dt.date, day_count: str = "ACT/365F",
                 date_col: str = "Date", naca_col: str = "NACA") -> None:
        import pandas as pd
        self.valuation_date = valuation_date
        self.day_count = day_count
        df = discount_curve_df.copy()
        if date_col not in df.columns or naca_col not in df.columns:
            raise ValueError(f"Curve df must have columns [{date_col}, {naca_col}].")
        df[date_col] = pd.to_datetime(df[date_col]).dt.strftime("%Y-%m-%d")
        df[naca_col] = pd.to_numeric(df[naca_col], errors="coerce")
        missing = df[naca_col].isna()
        if missing.any():
            raise ValueError(f"Found non-numeric NACA values. Examples:\n{df[missing].head(5)}")
        self._df = df[[date_col, naca_col]].rename(columns={date_col: "Date", naca_col: "NACA"})
        # a repeated date keeps its last row
        self._map: Dict[str, float] = dict(zip(self._df["Date"].values, self._df["NACA"].values))

    @classmethod
    def from_csv(cls, path: str, valuation_date: dt.date, day_count: str = "ACT/365F",
                 date_col: str = "Date", naca_col: str = "NACA",
                 date_format: Optional[str] = None) -> "NacaCurve":
        import pandas as pd
        df = pd.read_csv(path)
        if date_format is not None:
            df[date_col] = pd.to_datetime(df[date_col], format=date_format)
        return cls(df, valuation_date=valuation_date, day_count=day_count, date_col=date_col,
                   naca_col=naca_col)

    def year_fraction(self, start_date: dt.date, end_date: dt.date) -> float:
        return market.year_fraction(self.day_count, start_date, end_date)

    def get_naca(self, lookup_date: dt.date) -> float:
        iso = lookup_date.isoformat()
        if iso not in self._map:
            raise ValueError(f"NACA not found for date: {iso}")
        return float(self._map[iso])

    def get_discount_factor(self, lookup_date: dt.date) -> float:
        naca = self.get_naca(lookup_date)
        tau = self.year_fraction(self.valuation_date, lookup_date)
        return (1.0 + naca) ** (-tau)

    def get_forward_nacc_rate(self, start_date: dt.date, end_date: dt.date) -> float:
        """-ln(DF(end) / DF(start)) / tau(start, end)."""
        df_far = self.get_discount_factor(end_date)
        df_near = self.get_discount_factor(start_date)
        tau = self.year_fraction(start_date, end_date)
        return -math.log(df_far / df_near) / max(1e-12, tau)


@dataclass(frozen=True)
class BarrierSpec:
    barrier_type: str            # one of "none", "down-and-out", "up-and-out", "down-and-in", "up-and-in"
    level: Optional[float] = None
    tol_bps: float = 0.0         # band in basis points of the level
    abs_tol: float = 0.0         # absolute band; the larger of the two applies


@dataclass(frozen=True)
class RebateSpec:
    amount: float = 0.0
    rebate_at_hit: bool = False  # discount from the hit date instead of maturity


@dataclass(frozen=True)
class MCConfig:
    n_paths: int = 200_000
    seed: int = 42
    antithetic: bool = True
    chunk_size: int = 50_000
    dividend_before_monitor: bool = True
    spot_floor: float = 1e-12


@dataclass
class McContract:
    """One contract as the path engines take it (include/fdcn.h, fdcn_mc_*)."""
    params: np.ndarray   # [MC_NPARAM]
    flags: np.ndarray    # [MC_NFLAG] int32 (stream id 0; set per launch)
    step: np.ndarray     # [n_steps, MC_NSTEP]
    grid: List[dt.date]
    barrier_type: str
    barrier_level: Optional[float]
    band: float

    @property
    def n_steps(self) -> int:
        return self.step.shape[0]


def _event_grid(valuation, maturity, dividends, monitor_dates, include_maturity_monitor):
    """Sorted union of valuation, maturity, dividend and monitor dates; the
    cash per dividend date; the monitored dates (:193-222)."""
    if maturity <= valuation:
        raise ValueError("maturity must be after valuation.")
    cash: Dict[dt.date, float] = {}
    for d, amount in dividends:
        if valuation < d <= maturity and float(amount) != 0.0:
            cash[d] = cash.get(d, 0.0) + float(amount)
    monitored = {d for d in monitor_dates if valuation < d <= maturity}
    if include_maturity_monitor:
        monitored.add(maturity)
    grid = sorted({valuation, maturity} | set(cash) | monitored)
    return grid, cash, monitored


def plan_contract(*, spot: float, strike: float, vol: float, option_type: str,
                  valuation: dt.date, maturity: dt.date, discount_curve: NacaCurve,
                  forward_curve: Optional[NacaCurve] = None,
                  dividends: Sequence[Tuple[dt.date, float]] = (),
                  monitor_dates: Sequence[dt.date] = (),
                  barrier: BarrierSpec = BarrierSpec("none"), rebate: RebateSpec = RebateSpec(),
                  cfg: MCConfig = MCConfig(), include_maturity_monitor: bool = True) -> McContract:
    """Everything the path engines need for one contract: the checks, the
    event grid and the per-step arrays, in the reference's order."""
    if spot <= 0.0 or strike <= 0.0:
        raise ValueError("spot and strike must be positive.")
    if vol < 0.0:
        raise ValueError("vol must be non-negative.")
    fwd = forward_curve or discount_curve
    grid, cash, monitored = _event_grid(valuation, maturity, dividends, monitor_dates,
                                        include_maturity_monitor)
    n_steps = len(grid) - 1
    if n_steps <= 0:
        raise ValueError("Event grid has no steps.")
    step = np.zeros((n_steps, capi.MC_NSTEP))
    for i in range(n_steps):
        d0, d1 = grid[i], grid[i + 1]
        tau = discount_curve.year_fraction(d0, d1)
        carry = fwd.get_forward_nacc_rate(d0, d1)
        step[i, capi.MC_S_DRIFT] = (carry - 0.5 * vol * vol) * tau
        step[i, capi.MC_S_DIFF] = vol * math.sqrt(max(tau, 0.0))
        step[i, capi.MC_S_DIV] = cash.get(d1, 0.0)
        step[i, capi.MC_S_MONITOR] = 1.0 if d1 in monitored else 0.0
    df_T = discount_curve.get_discount_factor(maturity)

    bt = barrier.barrier_type
    if bt not in _KINDS:
        raise ValueError(f"unknown barrier_type {bt!r}")
    band, threshold = 0.0, 0.0
    if bt != "none":
        if barrier.level is None or barrier.level <= 0.0:
            raise ValueError("barrier.level must be provided and positive for barrier options.")
        band = max(barrier.abs_tol, abs(barrier.level) * (barrier.tol_bps * 1e-4))
        threshold = barrier.level + band if bt in _DOWN else barrier.level - band
    # the hit date's own discount factor, where a path can be paid from it
    at_hit = bt in _OUT and rebate.rebate_at_hit and rebate.amount != 0.0
    for i in range(n_steps):
        pays_here = at_hit and step[i, capi.MC_S_MONITOR] != 0.0
        step[i, capi.MC_S_DF_END] = (discount_curve.get_discount_factor(grid[i + 1])
                                     if pays_here else df_T)
    params = np.array([spot, strike, df_T, threshold, rebate.amount, cfg.spot_floor], dtype=float)
    flags = np.array([option_type != "call", capi.MC_KIND[bt], bool(rebate.rebate_at_hit),
                      bool(cfg.dividend_before_monitor), 0], dtype=np.int32)
    return McContract(params=params, flags=flags, step=step, grid=grid, barrier_type=bt,
                      barrier_level=barrier.level, band=float(band))


def _n_observations(cfg: MCConfig) -> int:
    n_paths = int(cfg.n_paths)
    if n_paths <= 0:
        raise ValueError("cfg.n_paths must be positive.")
    n_obs = n_paths // 2 if cfg.antithetic else n_paths
    if cfg.antithetic and n_obs <= 0:
        raise ValueError("With antithetic=True, set n_paths >= 2.")
    return n_obs


# ---------------------------------------------------------------------------
# the Philox mapping of include/fdcn.h, in NumPy
# ---------------------------------------------------------------------------
def philox4x32_10(counter: np.ndarray, key) -> np.ndarray:
    """Philox4x32-10 of counter [..., 4] (uint32) under key (k0, k1)."""
    c = [np.asarray(counter[..., k], dtype=np.uint64) for k in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    mask = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c[3] ^ np.uint64(k1),
             p0 & mask]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def philox_normals(n_obs: int, n_steps: int, seed: int, stream_id: int = 0,
                   obs_first: int = 0) -> np.ndarray:
    """z [n_obs, n_steps] of (seed, stream id) for observations obs_first ..:
    the device generator's mapping (include/fdcn.h), equal to it up to the
    last ulps of log / sincos."""
    n_pairs = (n_steps + 1) // 2
    obs = (np.arange(n_obs, dtype=np.uint64) + np.uint64(int(obs_first) & (2 ** 64 - 1)))
    ctr = np.empty((n_obs, n_pairs, 4), dtype=np.uint64)
    ctr[..., 0] = (obs & np.uint64(0xFFFFFFFF))[:, None]
    ctr[..., 1] = (obs >> np.uint64(32))[:, None]
    ctr[..., 2] = np.arange(n_pairs, dtype=np.uint64)[None, :]
    ctr[..., 3] = np.uint64(int(stream_id))
    seed = int(seed) & (2 ** 64 - 1)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))

    def u53(hi, lo):
        return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0
                + (lo >> np.uint32(6)).astype(np.float64) + 0.5) * 2.0 ** -53
    u1, u2 = u53(x[..., 0], x[..., 1]), u53(x[..., 2], x[..., 3])
    r = np.sqrt(-2.0 * np.log(u1))
    z = np.empty((n_obs, 2 * n_pairs))
    z[:, 0::2] = r * np.cos(2.0 * np.pi * u2)
    z[:, 1::2] = r * np.sin(2.0 * np.pi * u2)
    return np.ascontiguousarray(z[:, :n_steps])


# ---------------------------------------------------------------------------
# engines
# ---------------------------------------------------------------------------
def host_payoffs(c: McContract, Z: np.ndarray, increments: bool = False) -> np.ndarray:
    """Discounted payoff of each row of Z [n, n_steps] (one path per row), in
    NumPy, with the reference's operations in the reference's order.  With
    `increments`, Z holds the scaled Brownian increments W[m] - W[m-1] of a
    path construction (qmc.qmc_increments) and a step is s *= exp(drift + dW)."""
    P, F, S = c.params, c.flags, c.step
    spot, strike, df_T, thr, rebate, floor = (float(v) for v in P)
    kind = int(F[capi.MC_F_KIND])
    div_first = bool(F[capi.MC_F_DIV_FIRST])
    n = Z.shape[0]
    s = np.full(n, spot, dtype=float)
    untouched = np.ones(n, dtype=bool)
    hit_df = np.full(n, df_T)
    for i in range(c.n_steps):
        if increments:
            s *= np.exp(S[i, capi.MC_S_DRIFT] + Z[:, i])
        else:
            s *= np.exp(S[i, capi.MC_S_DRIFT] + S[i, capi.MC_S_DIFF] * Z[:, i])
        div = float(S[i, capi.MC_S_DIV])
        if div_first and div != 0.0:
            s = np.maximum(s - div, floor)
        if kind != 0 and S[i, capi.MC_S_MONITOR] != 0.0:
            breached = s <= thr if kind in (1, 3) else s >= thr
            hit_df[breached & untouched] = S[i, capi.MC_S_DF_END]
            untouched &= ~breached
        if not div_first and div != 0.0:
            s = np.maximum(s - div, floor)
    vanilla = np.maximum(strike - s, 0.0) if F[capi.MC_F_PUT] else np.maximum(s - strike, 0.0)
    pv = df_T * vanilla
    if kind == 0:
        return pv
    if kind <= 2:
        paid = rebate * (hit_df if F[capi.MC_F_REBATE_AT_HIT] else df_T)
        return np.where(untouched, pv, paid)
    return pv * ~untouched


def _host_observations(c: McContract, Z: np.ndarray, antithetic: bool,
                       increments: bool = False) -> np.ndarray:
    if antithetic:
        return 0.5 * (host_payoffs(c, Z, increments) + host_payoffs(c, -Z, increments))
    return host_payoffs(c, Z, increments)


def _stats(n: int, sum_p: float, sum_p2: float) -> Tuple[float, float]:
    """price and stderr of n observations (:407-410)."""
    nf = float(n)
    price = sum_p / nf
    var = max(0.0, (sum_p2 / nf) - price * price)
    return price, math.sqrt(var / nf)


def merge_mc_stats(parts) -> Dict[str, float]:
    """Price and stderr of the union of disjoint observation ranges, from
    their (n, sum p, sum p^2) -- tuples, or the result dicts of
    mc_barrier_batch.  Ranks that shard a contract's paths
    (distributed.shard_range + obs_range) gather these three numbers."""
    n, sp, sp2 = 0, 0.0, 0.0
    for part in parts:
        if isinstance(part, dict):
            part = (part["n_observations"], part["sum_p"], part["sum_p2"])
        n += int(part[0])
        sp += float(part[1])
        sp2 += float(part[2])
    if n <= 0:
        raise ValueError("merge_mc_stats: no observations")
    price, stderr = _stats(n, sp, sp2)
    return {"price": price, "stderr": stderr, "n_observations": n, "sum_p": sp, "sum_p2": sp2}


def _qmc_stats(n: int, rep_sum_p) -> Tuple[float, float, List[float]]:
    """price, stderr and the replicate means of R replicates of n observations
    each, in the order of the device's finalize kernel (include/fdcn.h)."""
    means = [float(sp) / float(n) for sp in rep_sum_p]
    R = len(means)
    total = 0.0
    for m in means:
        total += m
    price = total / float(R)
    ss = 0.0
    for m in means:
        ss += (m - price) * (m - price)
    stderr = math.sqrt(ss / float(R - 1) / float(R)) if R > 1 else 0.0
    return price, stderr, means


def merge_qmc_stats(parts) -> Dict[str, object]:
    """Price and stderr of a quasi-Monte Carlo run from its shards, merged by
    replicate id: tuples (replicate id, n, sum p, sum p^2), or result dicts of
    mc_barrier_batch / price_discrete_barrier_mc under rng="sobol".  Shards of
    one replicate (disjoint observation ranges) add; distinct ids are
    independent replicates.  Every replicate must end with the same n."""
    acc: Dict[int, List[float]] = {}
    for part in parts:
        if isinstance(part, dict):
            rows = zip(part["replicate_ids"], [part["observations_per_replicate"]] *
                       len(part["replicate_ids"]), part["rep_sum_p"], part["rep_sum_p2"])
        else:
            rows = [part]
        for rid, n, sp, sp2 in rows:
            a = acc.setdefault(int(rid), [0, 0.0, 0.0])
            a[0] += int(n)
            a[1] += float(sp)
            a[2] += float(sp2)
    if not acc:
        raise ValueError("merge_qmc_stats: no replicates")
    ids = sorted(acc)
    ns = {acc[k][0] for k in ids}
    if len(ns) != 1 or min(ns) <= 0:
        raise ValueError("merge_qmc_stats: the replicates hold different numbers of observations")
    n = ns.pop()
    price, stderr, _ = _qmc_stats(n, [acc[k][1] for k in ids])
    return {"price": price, "stderr": stderr, "replicates": len(ids), "replicate_ids": ids,
            "observations_per_replicate": n, "n_observations": n * len(ids),
            "rep_sum_p": [acc[k][1] for k in ids], "rep_sum_p2": [acc[k][2] for k in ids]}


def qmc_tables(group: Sequence[McContract], construction: str):
    """(dirnum [n_steps, 32], bridge_idx [n_steps, 3], bridge_w [B, n_steps, 3])
    of a launch: the order is shared, the weights follow each contract's DIFF
    column (its variance clock)."""
    n_steps = group[0].n_steps
    if n_steps > qmc.MAX_STEPS:
        raise ValueError(f"rng='sobol' takes at most {qmc.MAX_STEPS} steps (got {n_steps})")
    idx, ws = None, []
    for c in group:
        diff = c.step[:, capi.MC_S_DIFF]
        idx, w = qmc.bridge_plan(qmc.var_times(diff), construction, diff=diff)
        ws.append(w)
    return qmc.direction_numbers(n_steps), idx, np.stack(ws)


def simulate_qmc(group: Sequence[McContract], n_obs: int, antithetic: bool, *,
                 engine: str = "hip", seed: int = 0, stream_ids: Optional[Sequence[int]] = None,
                 obs_first: int = 0, replicates: int = 16, rep_first: int = 0,
                 construction: str = "bridge", scramble: bool = True,
                 chunk_size: Optional[int] = None, want_payoffs: bool = False):
    """Observations obs_first .. obs_first + n_obs - 1 of replicates rep_first
    .. rep_first + replicates - 1 for contracts that share n_steps.  Returns
    rep [B, R, 2] = sum p, sum p^2 of each replicate (and payoffs [B, R, n_obs]
    with want_payoffs).  Both engines perform the operations of include/fdcn.h
    (fdcn_mc_qmc_batch) in its order."""
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    if construction not in qmc.CONSTRUCTIONS:
        raise ValueError(f"construction must be one of {qmc.CONSTRUCTIONS}")
    B, n_obs, R = len(group), int(n_obs), int(replicates)
    obs_first, rep_first = int(obs_first), int(rep_first)
    n_steps = group[0].n_steps
    if any(c.n_steps != n_steps for c in group):
        raise ValueError("simulate: the contracts of a launch share n_steps")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError("simulate: one stream id per contract")
    if n_obs < 1 or R < 1 or obs_first < 0 or rep_first < 0:
        raise ValueError("simulate: observations and replicates must be non-empty ranges")
    if not scramble and R != 1:
        raise ValueError("simulate: without the digital shift there is one replicate")
    if obs_first + n_obs > 2 ** qmc.TABLE_BITS:
        raise ValueError(f"rng='sobol': observation indices must stay below 2^{qmc.TABLE_BITS} "
                         f"(the direction-number table has {qmc.TABLE_BITS} bits)")
    dirnum, idx, BW = qmc_tables(group, construction)
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)
        out = capi.mc_qmc_batch(P, F, S, n_obs, R, antithetic, dirnum, idx, BW,
                                scramble=scramble, seed=seed, obs_first=obs_first,
                                rep_first=rep_first, want_payoffs=want_payoffs)
        return (out[1], out[2]) if want_payoffs else out[1]
    rep = np.zeros((B, R, 2))
    pay = np.empty((B, R, n_obs)) if want_payoffs else None
    chunk = max(1, int(chunk_size or n_obs))
    for lo in range(0, n_obs, chunk):
        m = min(chunk, n_obs - lo)
        words = qmc.sobol_words(m, dirnum, obs_first + lo)
        for b, c in enumerate(group):
            shifts = (qmc.digital_shifts(n_steps, range(rep_first, rep_first + R), seed, ids[b])
                      if scramble else np.zeros((1, n_steps), dtype=np.uint32))
            for k in range(R):
                y = qmc.as241(qmc.uniforms(words ^ shifts[k][None, :]))
                p = _host_observations(c, qmc.qmc_increments(y, idx, BW[b]), antithetic,
                                       increments=True)
                rep[b, k, 0] += float(np.sum(p))
                rep[b, k, 1] += float(np.sum(p * p))
                if want_payoffs:
                    pay[b, k, lo:lo + m] = p
    return (rep, pay) if want_payoffs else rep


def _stack(group: Sequence[McContract], stream_ids: Sequence[int]):
    P = np.stack([c.params for c in group])
    F = np.stack([c.flags for c in group]).astype(np.int32)
    F[:, capi.MC_F_STREAM] = np.asarray(stream_ids, dtype=np.int32)
    S = np.stack([c.step for c in group])
    return P, F, S


def simulate(group: Sequence[McContract], n_obs: int, antithetic: bool, *, engine: str = "hip",
             rng: str = "philox", seed: int = 0, chunk_size: Optional[int] = None,
             stream_ids: Optional[Sequence[int]] = None, obs_first: int = 0, z=None,
             want_payoffs: bool = False, replicates: int = 16, construction: str = "bridge",
             rep_first: int = 0):
    """Run n_obs observations of contracts that share n_steps.  Returns
    sums [B, 2] = sum p, sum p^2 (and payoffs [B, n_obs] with want_payoffs).
    rng="sobol" runs n_obs observations of each of `replicates` replicates and
    returns simulate_qmc's per-replicate sums [B, R, 2] (payoffs [B, R, n_obs]).

    Normals: `z` [n_obs, n_steps] if given; else rng="numpy" draws
    default_rng(seed).standard_normal((m, n_steps)) per chunk of `chunk_size`
    observations, shared by the group, and the sums accumulate chunk by chunk;
    rng="philox" is the stream (seed, stream id) from observation obs_first."""
    if engine not in ("hip", "host"):
        raise ValueError("engine must be 'hip' or 'host'")
    if rng not in ("philox", "numpy", "sobol"):
        raise ValueError("rng must be 'philox', 'numpy' or 'sobol'")
    if rng == "sobol":
        if z is not None:
            raise ValueError("simulate: rng='sobol' generates its own normals")
        return simulate_qmc(group, n_obs, antithetic, engine=engine, seed=seed,
                            stream_ids=stream_ids, obs_first=obs_first, replicates=replicates,
                            rep_first=rep_first, construction=construction,
                            chunk_size=chunk_size, want_payoffs=want_payoffs)
    B = len(group)
    n_steps = group[0].n_steps
    if any(c.n_steps != n_steps for c in group):
        raise ValueError("simulate: the contracts of a launch share n_steps")
    ids = list(range(B)) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != B:
        raise ValueError("simulate: one stream id per contract")
    n_obs = int(n_obs)
    sums = np.zeros((B, 2))
    pay = np.empty((B, n_obs)) if want_payoffs else None
    if engine == "hip":
        capi.require_device()
        P, F, S = _stack(group, ids)

    def run(Z, lo, m):
        """observations lo .. lo+m-1, normals Z (None: the device's Philox)"""
        if engine == "hip":
            out = capi.mc_barrier_batch(P, F, S, m, antithetic, z=Z, seed=seed,
                                        obs_first=obs_first + lo, want_payoffs=want_payoffs)
            st, p = out if want_payoffs else (out, None)
            sums[:, 0] += st[:, 2]
            sums[:, 1] += st[:, 3]
            if want_payoffs:
                pay[:, lo:lo + m] = p
            return
        for b, c in enumerate(group):
            Zb = Z if Z is not None else philox_normals(m, n_steps, seed, ids[b], obs_first + lo)
            p = _host_observations(c, Zb, antithetic)
            sums[b, 0] += float(np.sum(p))
            sums[b, 1] += float(np.sum(p * p))
            if want_payoffs:
                pay[b, lo:lo + m] = p

    if z is not None:
        Z = np.ascontiguousarray(z, dtype=np.float64)
        if Z.shape != (n_obs, n_steps):
            raise ValueError(f"simulate: z must be [n_obs, n_steps] = {(n_obs, n_steps)}")
        run(Z, 0, n_obs)
    elif rng == "numpy":
        gen = np.random.default_rng(seed)
        chunk = max(1, int(chunk_size or n_obs))
        lo = 0
        while lo < n_obs:
            m = min(chunk, n_obs - lo)
            run(gen.standard_normal(size=(m, n_steps)), lo, m)
            lo += m
    elif engine == "hip":
        run(None, 0, n_obs)  # one launch, normals generated in the kernel
    else:
        chunk = max(1, int(chunk_size or n_obs))
        for lo in range(0, n_obs, chunk):
            run(None, lo, min(chunk, n_obs - lo))
    return (sums, pay) if want_payoffs else sums


def _result(c: McContract, cfg: MCConfig, n_obs: int, sum_p: float, sum_p2: float) -> dict:
    price, stderr = _stats(n_obs, sum_p, sum_p2)
    return {
        "price": float(price),
        "stderr": float(stderr),
        "ci_95": (float(price - 1.96 * stderr), float(price + 1.96 * stderr)),
        "n_observations": int(n_obs),
        "antithetic": bool(cfg.antithetic),
        "grid_points": int(len(c.grid)),
        "steps": int(c.n_steps),
        "barrier_type": c.barrier_type,
        "barrier_level": c.barrier_level,
        "barrier_band": float(c.band),
        "dividend_before_monitor": bool(cfg.dividend_before_monitor),
    }


def _qmc_result(c: McContract, cfg: MCConfig, n_rep: int, rep_ids: Sequence[int],
                rep_sums: np.ndarray, construction: str) -> dict:
    """The reference's keys with the replicate estimator: stderr is that of the
    replicate means; n_observations counts all replicates."""
    price, stderr, _ = _qmc_stats(n_rep, rep_sums[:, 0])
    res = _result(c, cfg, n_rep * len(rep_ids), 0.0, 0.0)
    res.update(price=float(price), stderr=float(stderr),
               ci_95=(float(price - 1.96 * stderr), float(price + 1.96 * stderr)),
               replicates=len(rep_ids), construction=construction,
               replicate_ids=[int(r) for r in rep_ids], observations_per_replicate=int(n_rep),
               rep_sum_p=[float(v) for v in rep_sums[:, 0]],
               rep_sum_p2=[float(v) for v in rep_sums[:, 1]])
    return res


def _qmc_split(cfg: MCConfig, replicates: int) -> int:
    """Observations per replicate: cfg.n_paths stays the total."""
    replicates = int(replicates)
    if replicates < 2:
        raise ValueError("rng='sobol' needs replicates >= 2 (the stderr is that of the "
                         "replicate means)")
    n_rep = _n_observations(cfg) // replicates
    if n_rep < 1:
        raise ValueError("cfg.n_paths gives fewer than one observation per replicate")
    return n_rep


def _default_rng(engine: str, rng: Optional[str]) -> str:
    return rng if rng is not None else ("philox" if engine == "hip" else "numpy")


def price_discrete_barrier_mc(*, spot: float, strike: float, vol: float, option_type: str,
                              valuation: dt.date, maturity: dt.date, discount_curve: NacaCurve,
                              forward_curve: Optional[NacaCurve] = None,
                              dividends: Sequence[Tuple[dt.date, float]] = (),
                              monitor_dates: Sequence[dt.date] = (),
                              barrier: BarrierSpec = BarrierSpec("none"),
                              rebate: RebateSpec = RebateSpec(), cfg: MCConfig = MCConfig(),
                              include_maturity_monitor: bool = True, engine: str = "hip",
                              rng: Optional[str] = None, replicates: int = 16,
                              construction: str = "bridge") -> Dict[str, object]:
    """Monte Carlo price of a discretely monitored single-barrier option: the
    reference's function, keys and errors, on the chosen engine (module
    docstring).  rng defaults to "philox" on the GPU (stream id 0) and to
    "numpy" on the host.  rng="sobol": `replicates` shifted Sobol point sets of
    observations // replicates points each through `construction`; the result
    adds "replicates", "construction" and the per-replicate sums."""
    c = plan_contract(spot=spot, strike=strike, vol=vol, option_type=option_type,
                      valuation=valuation, maturity=maturity, discount_curve=discount_curve,
                      forward_curve=forward_curve, dividends=dividends,
                      monitor_dates=monitor_dates, barrier=barrier, rebate=rebate, cfg=cfg,
                      include_maturity_monitor=include_maturity_monitor)
    if _default_rng(engine, rng) == "sobol":
        n_rep = _qmc_split(cfg, replicates)
        reps = simulate_qmc([c], n_rep, bool(cfg.antithetic), engine=engine, seed=cfg.seed,
                            stream_ids=[0], replicates=replicates, construction=construction,
                            chunk_size=cfg.chunk_size)
        return _qmc_result(c, cfg, n_rep, range(int(replicates)), reps[0], construction)
    n_obs = _n_observations(cfg)
    sums = simulate([c], n_obs, bool(cfg.antithetic), engine=engine,
                    rng=_default_rng(engine, rng), seed=cfg.seed, chunk_size=cfg.chunk_size,
                    stream_ids=[0])
    return _result(c, cfg, n_obs, float(sums[0, 0]), float(sums[0, 1]))


def mc_barrier_batch(contracts: Sequence[dict], cfg: MCConfig = MCConfig(), *,
                     engine: str = "hip", rng: Optional[str] = None,
                     stream_ids: Optional[Sequence[int]] = None,
                     obs_range: Optional[range] = None, replicates: int = 16,
                     construction: str = "bridge",
                     rep_range: Optional[range] = None) -> List[dict]:
    """Price many contracts, one launch per distinct n_steps.  `contracts`:
    the keyword arguments of price_discrete_barrier_mc (without cfg, engine,
    rng) per contract; cfg is shared.  The Philox stream id of a contract is
    its index in `contracts`, or stream_ids[index].  `obs_range` (a contiguous
    range within [0, n_obs)) runs that part of every contract's observations
    only -- a rank's shard, or the rest of a resumed run -- which continues
    the same Philox streams; merge_mc_stats combines the parts.  Results, in
    input order: the reference's dict plus "sum_p" and "sum_p2".
    rng="sobol": `replicates` replicates of observations // replicates points;
    obs_range then lies within one replicate's observations and `rep_range`
    (within range(replicates)) picks the replicates a shard runs;
    merge_qmc_stats combines the parts by replicate id."""
    rng = _default_rng(engine, rng)
    plans = [plan_contract(cfg=cfg, **kw) for kw in contracts]
    sobol = rng == "sobol"
    if rep_range is not None and not sobol:
        raise ValueError("rep_range needs rng='sobol'")
    n_total = _qmc_split(cfg, replicates) if sobol else _n_observations(cfg)
    r_lo, r_hi = 0, int(replicates)
    if sobol and rep_range is not None:
        r_lo, r_hi = rep_range.start, rep_range.stop
        if rep_range.step != 1 or not 0 <= r_lo < r_hi <= int(replicates):
            raise ValueError("rep_range must be a non-empty contiguous range within "
                             "range(replicates)")
    lo, hi = 0, n_total
    if obs_range is not None:
        lo, hi = obs_range.start, obs_range.stop
        if obs_range.step != 1 or not 0 <= lo < hi <= n_total:
            raise ValueError("obs_range must be a non-empty contiguous range within the "
                             "contract's observations")
        if rng == "numpy" and (lo, hi) != (0, n_total):
            raise ValueError("obs_range needs rng='philox' or 'sobol' (a counter-based stream)")
    ids = list(range(len(plans))) if stream_ids is None else [int(s) for s in stream_ids]
    if len(ids) != len(plans):
        raise ValueError("one stream id per contract")
    out: List[Optional[dict]] = [None] * len(plans)
    by_steps: Dict[int, List[int]] = {}
    for k, c in enumerate(plans):
        by_steps.setdefault(c.n_steps, []).append(k)
    for members in by_steps.values():
        if sobol:
            reps = simulate_qmc([plans[k] for k in members], hi - lo, bool(cfg.antithetic),
                                engine=engine, seed=cfg.seed, chunk_size=cfg.chunk_size,
                                stream_ids=[ids[k] for k in members], obs_first=lo,
                                replicates=r_hi - r_lo, rep_first=r_lo, construction=construction)
            for row, k in enumerate(members):
                out[k] = _qmc_result(plans[k], cfg, hi - lo, range(r_lo, r_hi), reps[row],
                                     construction)
            continue
        sums = simulate([plans[k] for k in members], hi - lo, bool(cfg.antithetic), engine=engine,
                        rng=rng, seed=cfg.seed, chunk_size=cfg.chunk_size,
                        stream_ids=[ids[k] for k in members], obs_first=lo)
        for row, k in enumerate(members):
            res = _result(plans[k], cfg, hi - lo, float(sums[row, 0]), float(sums[row, 1]))
            res["sum_p"], res["sum_p2"] = float(sums[row, 0]), float(sums[row, 1])
            out[k] = res
    return out  # type: ignore[return-value]
