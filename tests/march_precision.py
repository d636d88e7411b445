"""A condition-aware rounding yardstick for the march kernels (no GPU import).

For one packed group (engine.Group) the reference is V_ext, the long-double
march of oracle/fdcn_oracle_ext.c on the same fp64 plan.  How far an honest
fp64 evaluation of that march may be from V_ext depends on the grid (the
Courant number dt sigma^2 / dx^2 spans 0.01 .. 1e6 over the suite's cases), so
the bound is not a constant: it is measured, per solve, on three fp64
realisations of the same sequential algorithm --

  f64     the literal march (bit-identical to oracle_cn_batch / oracle_it_batch)
  f64fma  the same with every a*b+c contracted to one rounding
  mirror  the literal march on the mirrored plan (node order reversed, so the
          Thomas elimination runs from the other end), mirrored back

With u = 2^-53, per solve:
  N     = max over the realisations of max_j |V - V_ext|
  vmax  = max_j |V_ext|
  T     = { j : |V_ext,j| <= 1e-3 vmax }          the out-of-the-money tail
  N_T   = N over T only
and a candidate V passes when
  max_j     |V - V_ext| <= 8 max(N,   2 u vmax)
  max_{j∈T} |V - V_ext| <= 8 max(N_T, 2 u 1e-3 vmax) + 2e-18 n_time vmax

A fourth realisation, KERNEL_ORDER, restates the kernels' own reassociation
of the solve sequentially on the CPU (fdcn_oracle_ext.c, EXT_CONVERGED and
EXT_RECOVERY: converged LU factors with every coefficient pre-divided by the
root r and rounded once per phase, Sherman-Morrison for the first row, and
the Crank-Nicolson right-hand side recovered from the previous step's).  Its
once-rounded constants perturb every step the same way, so on about one solve
in a hundred it is 10 to 30 times further from V_ext than all three Thomas
orderings -- and the kernels are there with it, to within a few per cent
(DESIGN section 5).  It joins N only for the input groups where the kernels
exceeded the three-realisation bound (march_cases.KERNEL_ORDER_GROUPS), and
is never part of the leave-one-out condition.

8 is three bits over the spread of fp64 evaluation orders of one algorithm
(test_march_precision.py's leave-one-out run holds every realisation to the
bound built from the other two).  2e-18 n_time vmax is DESIGN section 5,
deviation 1: the kernel cuts two series per step at 1e-18 of the carried
values.  Nothing here is taken from a kernel's output.

Errors are (V - hi) - lo in fp64 with V_ext = hi + lo, so knocked-out nodes
and exact zeros compare equal.

The spot-space per-row march (engine.VcGroup, csrc/fdcn_vc.hip) goes through
the same Yardstick with the same constants.  Its three realisations are the
literal march of oracle_vc_batch, the same contracted, and the mirrored plan
(sub <-> sup and a <-> c swapped, every row array reversed, the bnd columns
swapped, ko_lo / ko_hi -> n-1-ko_hi / n-1-ko_lo, v_init reversed, the result
reversed back).  The 2e-18 n_time vmax term is 0 for these groups: fdcn_vc.hip
truncates nothing.  Its factor kernel finds the pivots by an exact projective
product scan (powers of two only rescale it), the march's two recurrences are
exact affine scans over all lanes and waves with the Dirichlet values as
carry-ins, and no cut-off constant appears in the file -- read against the
source: the only literals in its arithmetic are 0 and 1.  Its own ordering
(rows stored scaled by 1 / pivot, rounded once per phase; the pointwise form
x = alpha V + u) is restated sequentially by oracle_ext.vc_batch(order=1, 2):
KERNEL_STENCIL and KERNEL_POINTWISE below, a fourth realisation only for the
groups of vc_cases.KERNEL_ORDER_GROUPS and never part of leave-one-out.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np

from finite_difference_amd import capi
from finite_difference_amd.engine import Group, VcGroup

U = 2.0 ** -53
FACTOR = 8.0
TAIL_REL = 1e-3
SERIES_CUT = 2e-18
REALISATIONS = ("f64", "f64fma", "mirror")
KERNEL_ORDER = "kernel_order"
KERNEL_STENCIL, KERNEL_POINTWISE = "kernel_stencil", "kernel_pointwise"  # VcGroup only
_VC_ORDER = {KERNEL_STENCIL: 1, KERNEL_POINTWISE: 2}
NTHREADS = 8
OLD_TOL = 1e-10


def _mirror_vc(g: VcGroup) -> VcGroup:
    n = g.n_nodes
    I = g.iparams.copy()
    I[:, capi.I_KO_LO] = n - 1 - g.iparams[:, capi.I_KO_HI]
    I[:, capi.I_KO_HI] = n - 1 - g.iparams[:, capi.I_KO_LO]
    D = g.diag[:, :, [2, 1, 0, 5, 4, 3], ::-1]  # sub <-> sup, a <-> c, rows reversed
    return dataclasses.replace(
        g, diag=np.ascontiguousarray(D), bnd=np.ascontiguousarray(g.bnd[:, :, ::-1]),
        iparams=I, v_init=np.ascontiguousarray(g.v_init[:, ::-1]))


def mirror_group(g: Union[Group, VcGroup]) -> Union[Group, VcGroup]:
    """The same marches with the node order reversed: a <-> c, the boundary
    blocks and forms swapped, ko_lo / ko_hi -> n-1-ko_hi / n-1-ko_lo, v_init
    and the payoff reversed.  The monitor schedule is unchanged."""
    if isinstance(g, VcGroup):
        return _mirror_vc(g)
    n = g.n_nodes
    P = g.params.copy()
    I = g.iparams.copy()
    P[:, capi.P_A], P[:, capi.P_C] = g.params[:, capi.P_C], g.params[:, capi.P_A]
    P[:, capi.P_LO_C0:capi.P_LO_E1 + 1] = g.params[:, capi.P_HI_C0:capi.P_HI_E1 + 1]
    P[:, capi.P_HI_C0:capi.P_HI_E1 + 1] = g.params[:, capi.P_LO_C0:capi.P_LO_E1 + 1]
    I[:, capi.I_LO_FORM], I[:, capi.I_HI_FORM] = g.iparams[:, capi.I_HI_FORM], g.iparams[:, capi.I_LO_FORM]
    I[:, capi.I_KO_LO] = n - 1 - g.iparams[:, capi.I_KO_HI]
    I[:, capi.I_KO_HI] = n - 1 - g.iparams[:, capi.I_KO_LO]
    return dataclasses.replace(
        g, params=P, iparams=I, v_init=np.ascontiguousarray(g.v_init[:, ::-1]),
        payoff=None if g.payoff is None else np.ascontiguousarray(g.payoff[:, ::-1]))


def march(kind: str, g: Union[Group, VcGroup], order: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(hi, lo) of the group's marches in the arithmetic `kind` of oracle_ext
    (order: oracle_ext.vc_batch's, VcGroup only)."""
    from oracle import oracle_ext
    if isinstance(g, VcGroup):
        return oracle_ext.vc_batch(kind, g.n_nodes, g.n_time, g.n_ranna, g.diag, g.bnd, g.v_init,
                                   g.iparams, g.mon_step, g.mon_rebate, NTHREADS, order)
    if g.it:
        return oracle_ext.it_batch(kind, g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams,
                                   g.v_init, g.payoff, NTHREADS)
    return oracle_ext.cn_batch(kind, g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams,
                               g.v_init, g.mon_step, g.mon_rebate, NTHREADS)


def march_mirrored(kind: str, g: Group) -> Tuple[np.ndarray, np.ndarray]:
    hi, lo = march(kind, mirror_group(g))
    return np.ascontiguousarray(hi[:, ::-1]), np.ascontiguousarray(lo[:, ::-1])


def realise(name: str, g: Group) -> np.ndarray:
    if name == "mirror":
        return march_mirrored("f64", g)[0]
    if name in _VC_ORDER:
        return march("f64fma", g, _VC_ORDER[name])[0]
    if name == KERNEL_ORDER:
        return march("f64rec", g)[0]
    return march(name, g)[0]


def _ratio(err: np.ndarray, bound: np.ndarray) -> np.ndarray:
    """err / bound per solve; 0 where both are 0, inf where only the bound is."""
    out = np.zeros_like(err)
    pos = bound > 0.0
    out[pos] = err[pos] / bound[pos]
    out[~pos & (err > 0.0)] = np.inf
    return out


@dataclass
class Yardstick:
    g: Union[Group, VcGroup]
    hi: np.ndarray                 # [B, n]  (double) V_ext
    lo: np.ndarray                 # [B, n]  (double)(V_ext - hi)
    real: Dict[str, np.ndarray]    # the fp64 realisations, [B, n] each

    @property
    def vmax(self) -> np.ndarray:
        return np.max(np.abs(self.hi), axis=1)

    @property
    def tail(self) -> np.ndarray:
        """[B, n] bool: the nodes of T."""
        return np.abs(self.hi) <= TAIL_REL * self.vmax[:, None]

    def err(self, V: np.ndarray) -> np.ndarray:
        return np.abs((np.asarray(V, np.float64) - self.hi) - self.lo)

    def noise(self, exclude: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(N, N_T) per solve over the realisations other than `exclude`."""
        names = [k for k in self.real if k != exclude]
        e = np.max(np.stack([self.err(self.real[k]) for k in names]), axis=0)
        return np.max(e, axis=1), np.max(np.where(self.tail, e, 0.0), axis=1)

    def bounds(self, exclude: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(max-norm bound, tail bound) per solve."""
        N, NT = self.noise(exclude)
        vmax = self.vmax
        b_max = FACTOR * np.maximum(N, 2.0 * U * vmax)
        cut = 0.0 if isinstance(self.g, VcGroup) else SERIES_CUT  # fdcn_vc truncates nothing
        b_tail = (FACTOR * np.maximum(NT, 2.0 * U * TAIL_REL * vmax)
                  + cut * self.g.n_time * vmax)
        return b_max, b_tail

    def ratios(self, V: np.ndarray, exclude: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray]:
        """error / bound per solve, for the max-norm and the tail bound."""
        V = np.asarray(V, np.float64)
        assert V.shape == self.hi.shape, (V.shape, self.hi.shape)
        finite = np.all(np.isfinite(V), axis=1)
        e = self.err(np.where(np.isfinite(V), V, 0.0))
        b_max, b_tail = self.bounds(exclude)
        r_max = _ratio(np.max(e, axis=1), b_max)
        r_tail = _ratio(np.max(np.where(self.tail, e, 0.0), axis=1), b_tail)
        r_max[~finite] = np.inf
        r_tail[~finite] = np.inf
        return r_max, r_tail

    def check(self, V: np.ndarray, label: str, exclude: Optional[str] = None) -> Tuple[float, float]:
        """Assert both bounds on every solve; returns the worst ratios."""
        r_max, r_tail = self.ratios(V, exclude)
        w_max, w_tail = float(np.max(r_max)), float(np.max(r_tail))
        N, _ = self.noise(exclude)
        with np.errstate(divide="ignore", invalid="ignore"):
            noise_u = float(np.max(np.where(self.vmax > 0, N / (U * self.vmax), 0.0)))
        print(f"[{label}] solves={self.g.B} n={self.g.n_nodes} m={self.g.n_time} "
              f"ratio_max={w_max:.3f} ratio_tail={w_tail:.3f} N<={noise_u:.3g}u")
        bad = [int(i) for i in np.flatnonzero((r_max > 1.0) | (r_tail > 1.0))]
        assert not bad, (f"{label}: solves {bad} outside the rounding yardstick: "
                         f"max-norm ratios {[float(r_max[i]) for i in bad]}, "
                         f"tail ratios {[float(r_tail[i]) for i in bad]}")
        return w_max, w_tail


def yardstick(g: Union[Group, VcGroup], realisations: Sequence[str] = REALISATIONS) -> Yardstick:
    hi, lo = march("ld", g)
    return Yardstick(g, hi, lo, {k: realise(k, g) for k in realisations})


def old_bound_ok(V: np.ndarray, ref: np.ndarray, tol: float = OLD_TOL) -> bool:
    """The fixed tolerance of test_gpu_kernels.py, per solve (1-D arrays)."""
    return float(np.max(np.abs(V - ref))) <= tol * max(1.0, float(np.max(np.abs(ref))))
