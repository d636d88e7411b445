"""Quasi-Monte Carlo points and path constructions for the barrier MC pricer.

The NumPy restatement of the generator contract of include/fdcn.h
(fdcn_mc_qmc_batch) -- Sobol word, digital shift, uniform, AS241 normal, the
table-driven path construction -- and with it the host engine of
``mc_barrier`` under ``rng="sobol"``.  The device kernel
(csrc/fdcn_mc_qmc.hip) performs the same operations in the same order; only
its ``log`` / ``sqrt`` (the tails of AS241) and ``exp`` may differ in the last
ulp.

* ``direction_numbers(n_dims)``  the table the caller hands to the library
  (the library embeds none): torch's Joe-Kuo numbers, left-aligned to 32 bits
* ``sobol_words``                Gray-code points, unscrambled
* ``digital_shifts``             one Philox word per (replicate, dimension)
* ``as241``                      Wichura's PPND16, CPython's constants and order
* ``bridge_plan``                Brownian-bridge or incremental table + weights
* ``qmc_increments``             normals -> W[m] - W[m-1] through a table
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

MAX_STEPS = 64          # FDCN_QMC_MAX_STEPS
TABLE_BITS = 30         # torch's sobolstate: observation indices below 2^30
CONSTRUCTIONS = ("bridge", "incremental")


def direction_numbers(n_dims: int) -> np.ndarray:
    """dirnum [n_dims, 32] uint32, bit 31 = 1/2, from
    torch.quasirandom.SobolEngine's table (int64 [n_dims, 30], bit 29 = 1/2)
    shifted left by two; the last two columns are zero, so points with an
    index of 2^30 or more are not available from it."""
    import torch  # lazily: nothing else here needs it
    n_dims = int(n_dims)
    if not 1 <= n_dims <= MAX_STEPS:
        raise ValueError(f"direction_numbers: n_dims must be in 1 .. {MAX_STEPS}")
    state = torch.quasirandom.SobolEngine(n_dims, scramble=False).sobolstate.numpy()
    if state.shape != (n_dims, TABLE_BITS):
        raise ValueError(f"unexpected sobolstate shape {state.shape}")
    out = np.zeros((n_dims, 32), dtype=np.uint32)
    out[:, :TABLE_BITS] = (state.astype(np.uint64) << np.uint64(32 - TABLE_BITS)).astype(np.uint32)
    return out


def sobol_words(n_obs: int, dirnum: np.ndarray, obs_first: int = 0) -> np.ndarray:
    """w [n_obs, n_dims] uint32 of observations obs_first ..: with
    g = o ^ (o >> 1), the XOR of dirnum[j][k] over the set bits k of g."""
    D = np.ascontiguousarray(dirnum, dtype=np.uint32)
    if D.ndim != 2 or D.shape[1] != 32:
        raise ValueError("sobol_words: dirnum must be [n_dims, 32]")
    n_obs, obs_first = int(n_obs), int(obs_first)
    if n_obs < 1 or obs_first < 0 or obs_first + n_obs > 2 ** 32:
        raise ValueError("sobol_words: observations must lie in 0 .. 2^32 - 1")
    o = np.arange(obs_first, obs_first + n_obs, dtype=np.uint64)
    g = o ^ (o >> np.uint64(1))
    w = np.zeros((n_obs, D.shape[0]), dtype=np.uint32)
    for k in range(int(obs_first + n_obs - 1).bit_length()):
        on = ((g >> np.uint64(k)) & np.uint64(1)).astype(bool)
        w[on] ^= D[None, :, k]
    return w


def digital_shifts(n_dims: int, replicates, seed: int, stream_id: int = 0) -> np.ndarray:
    """shift [len(replicates), n_dims] uint32: x0 of Philox4x32-10 with counter
    (j, rho, 0, stream id) under key (seed lo, seed hi)."""
    from .mc_barrier import philox4x32_10
    reps = np.asarray(list(replicates), dtype=np.uint64)
    ctr = np.zeros((reps.shape[0], int(n_dims), 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(int(n_dims), dtype=np.uint64)[None, :]
    ctr[..., 1] = reps[:, None]
    ctr[..., 3] = np.uint64(int(stream_id))
    seed = int(seed) & (2 ** 64 - 1)
    return philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))[..., 0]


def uniforms(words: np.ndarray) -> np.ndarray:
    """u = (w + 0.5) 2^-32: exact, never 0 or 1."""
    return (np.asarray(words, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


_A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4,
      4.5921953931549871457e+4, 1.3731693765509461125e+4, 1.9715909503065514427e+3,
      1.3314166789178437745e+2, 3.3871328727963666080e+0)
_B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4,
      2.1213794301586595867e+4, 5.3941960214247511077e+3, 6.8718700749205790830e+2,
      4.2313330701600911252e+1, 1.0)
_C = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1,
      1.27045825245236838258e+0, 3.64784832476320460504e+0, 5.76949722146069140550e+0,
      4.63033784615654529590e+0, 1.42343711074968357734e+0)
_D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2,
      1.48103976427480074590e-1, 6.89767334985100004550e-1, 1.67638483018380384940e+0,
      2.05319162663775882187e+0, 1.0)
_E = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3,
      2.65321895265761230930e-2, 2.96560571828504891230e-1, 1.78482653991729133580e+0,
      5.46378491116411436990e+0, 6.65790464350110377720e+0)
_F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5,
      7.86869131145613259100e-4, 1.48753612908506148525e-2, 1.36929880922735805310e-1,
      5.99832206555888793690e-1, 1.0)


def _horner(coef, r):
    acc = coef[0] * r + coef[1]
    for c in coef[2:]:
        acc = acc * r + c
    return acc


def as241(u) -> np.ndarray:
    """Phi^-1(u), u in (0, 1): Wichura's AS241 (PPND16) with the branches,
    constants and Horner order of CPython's statistics._normal_dist_inv_cdf.
    The central branch has no transcendental and equals it bit for bit."""
    p = np.asarray(u, dtype=np.float64)
    if np.any(~((p > 0.0) & (p < 1.0))):
        raise ValueError("as241: u must lie strictly between 0 and 1")
    q = p - 0.5
    out = np.empty_like(p)
    mid = np.abs(q) <= 0.425
    qm = q[mid]
    r = 0.180625 - qm * qm
    out[mid] = (_horner(_A, r) * qm) / _horner(_B, r)
    tail = ~mid
    qt, pt = q[tail], p[tail]
    r = np.sqrt(-np.log(np.where(qt <= 0.0, pt, 1.0 - pt)))
    near = r <= 5.0
    x = np.empty_like(r)
    rn = r[near] - 1.6
    x[near] = _horner(_C, rn) / _horner(_D, rn)
    rf = r[~near] - 5.0
    x[~near] = _horner(_E, rf) / _horner(_F, rf)
    out[tail] = np.where(qt < 0.0, -x, x)
    return out


def var_times(diff) -> np.ndarray:
    """t [n + 1]: t_0 = 0, t_m = sum_{k <= m} DIFF_k^2 accumulated in step
    order (the variance clock of a contract's per-step DIFF column)."""
    d = np.asarray(diff, dtype=np.float64).ravel()
    t = np.zeros(d.shape[0] + 1)
    for m in range(d.shape[0]):
        t[m + 1] = t[m] + d[m] * d[m]
    return t


def bridge_order(n: int) -> np.ndarray:
    """idx [n, 3] int32 (target, left, right) of the Brownian bridge: row 0
    sets n from 0 (right == left: an extension), then each segment (l, r) with
    r - l >= 2 is bisected at (l + r) // 2, breadth first.  Depends on n only."""
    n = int(n)
    if not 1 <= n <= MAX_STEPS:
        raise ValueError(f"bridge_order: n must be in 1 .. {MAX_STEPS}")
    rows = [(n, 0, 0)]
    level = [(0, n)]
    while level:
        nxt = []
        for l, r in level:
            if r - l < 2:
                continue
            i = (l + r) // 2
            rows.append((i, l, r))
            nxt += [(l, i), (i, r)]
        level = nxt
    return np.asarray(rows, dtype=np.int32)


def bridge_plan(t, construction: str = "bridge",
                diff: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(idx [n, 3] int32, w [n, 3]) for variance times t [n + 1] (var_times).

    "bridge": row 0 is target n from 0 with sd = sqrt(t_n); a bisection of
    (l, r) at i has wl = (t_r - t_i) / (t_r - t_l), wr = (t_i - t_l) /
    (t_r - t_l), sd = sqrt((t_i - t_l)(t_r - t_i) / (t_r - t_l)); a bracket of
    zero length gives (1, 0, 0).
    "incremental": row m - 1 = (m, m - 1, m - 1) with weights (1, 0, DIFF_m):
    `diff` if given, else sqrt(t_m - t_{m-1})."""
    t = np.asarray(t, dtype=np.float64).ravel()
    n = t.shape[0] - 1
    if construction == "incremental":
        m = np.arange(1, n + 1, dtype=np.int32)
        idx = np.stack([m, m - 1, m - 1], axis=1).astype(np.int32)
        w = np.zeros((n, 3))
        w[:, 0] = 1.0
        w[:, 2] = (np.asarray(diff, dtype=np.float64).ravel() if diff is not None
                   else np.sqrt(np.maximum(t[1:] - t[:-1], 0.0)))
        return idx, w
    if construction != "bridge":
        raise ValueError(f"construction must be one of {CONSTRUCTIONS}")
    idx = bridge_order(n)
    w = np.zeros((n, 3))
    w[0] = (1.0, 0.0, np.sqrt(t[n]))
    for j in range(1, n):
        i, l, r = (int(v) for v in idx[j])
        span = t[r] - t[l]
        if span > 0.0:
            w[j] = ((t[r] - t[i]) / span, (t[i] - t[l]) / span,
                    np.sqrt((t[i] - t[l]) * (t[r] - t[i]) / span))
        else:
            w[j] = (1.0, 0.0, 0.0)
    return idx, w


def check_table(idx) -> None:
    """The library's rule for bridge_idx (include/fdcn.h), restated."""
    idx = np.asarray(idx)
    n = idx.shape[0]
    defined = {0}
    for j, (t, l, r) in enumerate(idx.tolist()):
        ok = (1 <= t <= n and t not in defined and 0 <= l < t and l in defined
              and (r == l or (t < r <= n and r in defined)))
        if not ok:
            raise ValueError(f"bridge_idx row {j} = {(t, l, r)} breaks the table's rules")
        defined.add(t)


def qmc_paths(y: np.ndarray, idx: np.ndarray, w: np.ndarray) -> np.ndarray:
    """W [n_obs, n + 1] from normals y [n_obs, n]: W[0] = 0 and, row by row,
    W[target] = (wl W[left] + wr W[right]) + sd y_j."""
    y = np.asarray(y, dtype=np.float64)
    n = idx.shape[0]
    W = np.zeros((y.shape[0], n + 1))
    for j in range(n):
        t, l, r = (int(v) for v in idx[j])
        W[:, t] = (w[j, 0] * W[:, l] + w[j, 1] * W[:, r]) + w[j, 2] * y[:, j]
    return W


def qmc_increments(y: np.ndarray, idx: np.ndarray, w: np.ndarray) -> np.ndarray:
    """dW [n_obs, n]: W[m] - W[m - 1] of qmc_paths, what a step adds to its
    drift inside the exponent."""
    W = qmc_paths(y, idx, w)
    return W[:, 1:] - W[:, :-1]


def normals(n_obs: int, dirnum: np.ndarray, *, seed: int = 0, stream_id: int = 0,
            replicate: int = 0, scramble: bool = True, obs_first: int = 0):
    """(words [n_obs, n_dims] uint32, y [n_obs, n_dims]) of one replicate."""
    words = sobol_words(n_obs, dirnum, obs_first)
    if scramble:
        words = words ^ digital_shifts(words.shape[1], [replicate], seed, stream_id)[0][None, :]
    return words, as241(uniforms(words))
