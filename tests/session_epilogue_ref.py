"""References and a rounding yardstick for the session's epilogue kernels
(csrc/fdcn_session.hip: read_grid / greeks_kernel, dividend_jump_kernel).
No GPU import; numpy and the standard library only.

Readouts
  read_grid_f64 / trade_f64      the kernel's arithmetic in Python floats, one
                                 rounding per operation, in its operation
                                 order: the linear interpolation, the 3-point
                                 stencil, the 4x4 cubic fit by LU with partial
                                 pivoting (strict > on ties, rp = 1 / A[j][j]
                                 then multiply, the substitutions as written)
                                 and the four FDCN_GK_* combinations.
  read_grid_exact / trade_exact  the same formulas in fractions.Fraction (a
                                 double converts exactly, every operation is
                                 rational, the 4x4 solved by exact elimination).
A readout is the triple (V, ri, rd): the value vector, the five ints
[slot, icase, ilo, idx, dg_mode] and the eight doubles of include/fdcn.h.

Spline
  jump_f64    fdcn_dividend_jump (csrc/fdcn_host.hip) restated literally
  jump_exact  the natural cubic spline and its evaluation at the exact
              S_i - D in Fraction (n <= 257)
  jump_ld     the same in np.longdouble (n = 2049; needs a 64-bit mantissa)

Yardstick (the convention of march_precision.py), u = 2^-53, per trade and
output / per spline vector:
  N      = max over a set of fp64 realisations of |value - exact|
  bound  = 8 max(N, 2 u scale);  a candidate passes when |got - exact| <= bound
The realisations of a trade are trade_f64, the same with the cubic fit
solved by np.linalg.solve (LAPACK), and trade_f64 with the cubic's stencil
listed in reverse node order.  Those of a spline vector are jump_f64 and
jump_f64 on the mirrored problem (s -> -s, D -> -D, arrays reversed, result
reversed back; the exercise value of a call is applied afterwards, in the
original orientation).  For a vector N is the maximum over its nodes.

scale is the magnitude the output is a difference of.  Per readout, with
vmax the largest |V| among the nodes it reads and h the smallest spacing of
its Delta/Gamma stencil:
  price  p = vmax over the interpolation nodes (|V[0]|, |V[ilo]|)
  Delta  d = vmax / h        Gamma  g = vmax / h^2      (0 for dg_mode 0)
and per trade, propagated through the combination with absolute values:
  BARRIER   price p0, Delta d0, Gamma g0, vega (p1 + p0) / (|dv| 100),
            theta = sigma^2 S^2 g0 / 2 + |carry - q| S d0 + |r| p0
  CNLOG     vega (p1 + p2) / (2 |dv|), theta with |b| for the carry
  AMERICAN  X = (4 x1 + x0) / 3 for price, Delta, Gamma;
            vega (4 (p2 + p3) / (2|h|) + (p4 + p5) / (4|h|)) / 300;
            theta from the three; aux (4 p6 + p0) / 3
  READOUT   p0, d0, g0
and for a spline vector scale = max_j |v_j|.

Case families.  Every vector lives on a geometric grid s = exp(x0 + i dx),
dx from 10^-3.5 to 10^-1, or on a uniform dyadic grid where a case needs
exact ties; the values are a put payoff kink plus a smooth bump.  A cubic
whose S_dg lies 50 spacings outside its stencil extrapolates a derivative
over 50 h: its three realisations spread by the cube of that distance and do
not bound each other, so that family ("far") is ill-conditioned by
construction; it stays in the bitwise set and is left out of the accuracy
set.  Readouts of vectors holding inf / NaN in a node they use have no exact
value and are in the bitwise set only.  Every other family is in both.

Measured worst ratios error / bound (CPU realisations leave-one-out, device
on the MI355X) are quoted in test_session_epilogue_ref.py and
test_gpu_session_epilogue.py.
"""
from __future__ import annotations

import bisect
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from finite_difference_amd.session import (GK_AMERICAN, GK_BARRIER, GK_CNLOG, GK_NPARAM,
                                           GK_NRDBL, GK_NRINT, GK_READOUT, READOUTS, Readout,
                                           readout)

U = 2.0 ** -53
FACTOR = 8.0
OUTPUTS = ("price", "delta", "gamma", "vega", "theta", "aux")
REALISATIONS = ("lu", "lapack", "reversed")
JUMP_REALISATIONS = ("f64", "mirror")
HAVE_LD = np.finfo(np.longdouble).nmant >= 63


# ---------------------------------------------------------------------------
# readouts
# ---------------------------------------------------------------------------
def _div(a, b):
    """a / b; IEEE for a float zero divisor (the kernel does not trap)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def lu_solve(A: List[List], y: List, tie_last: bool = False) -> List:
    """read_grid's 4x4 solve: LU with partial pivoting in dgetf2 order.
    tie_last=True takes the last of equal pivots (>=), which the kernel must
    not; only test_session_epilogue_ref.py uses it, to show that the tie cases
    can tell the two apart."""
    A = [row[:] for row in A]
    perm = [0, 1, 2, 3]
    for j in range(4):
        p = j
        for i in range(j + 1, 4):
            if (abs(A[i][j]) >= abs(A[p][j])) if tie_last else (abs(A[i][j]) > abs(A[p][j])):
                p = i
        if p != j:
            A[j], A[p] = A[p], A[j]
            perm[j], perm[p] = perm[p], perm[j]
        rp = _div(1.0, A[j][j]) if isinstance(A[j][j], float) else 1 / A[j][j]
        for i in range(j + 1, 4):
            A[i][j] = A[i][j] * rp
            for k in range(j + 1, 4):
                A[i][k] = A[i][k] - A[i][j] * A[j][k]
    x = [y[perm[i]] for i in range(4)]
    for j in range(4):
        for i in range(j + 1, 4):
            x[i] = x[i] - x[j] * A[i][j]
    for j in range(3, -1, -1):
        x[j] = _div(x[j], A[j][j])
        for i in range(j):
            x[i] = x[i] - x[j] * A[i][j]
    return x


def lapack_solve(A: List[List[float]], y: List[float]) -> List[float]:
    return [float(v) for v in np.linalg.solve(np.array(A, np.float64), np.array(y, np.float64))]


def _read_grid(V, ri, rd, num, solve, reverse: bool = False) -> Tuple:
    """read_grid in the number type `num`, the cubic through `solve`."""
    icase, ilo, idx, mode = (int(x) for x in ri[1:5])
    rd = [num(float(x)) for x in rd]
    val = lambda i: num(float(V[i]))  # noqa: E731
    one, two = num(1.0), num(2.0)
    if icase == 1:
        price = val(0)
    elif icase == 2:
        price = val(ilo)
    else:
        w = _div(rd[0] - rd[1], rd[2] - rd[1])
        price = (one - w) * val(ilo) + w * val(ilo + 1)
    delta = gamma = num(0.0)
    if mode == 1:
        h1, h2 = rd[5] - rd[4], rd[6] - rd[5]
        Vm, V0, Vp = val(idx - 1), val(idx), val(idx + 1)
        delta = (_div(-h2, h1 * (h1 + h2)) * Vm + _div(h2 - h1, h1 * h2) * V0
                 + _div(h1, h2 * (h1 + h2)) * Vp)
        gamma = two * (_div(Vm, h1 * (h1 + h2)) - _div(V0, h1 * h2) + _div(Vp, h2 * (h1 + h2)))
    elif mode == 2:
        A, y = [], []
        for k in ((3, 2, 1, 0) if reverse else (0, 1, 2, 3)):
            zk = rd[4 + k] - rd[3]
            A.append([zk * zk * zk, zk * zk, zk, one])
            y.append(val(idx - 1 + k))
        x = solve(A, y)
        delta = x[2]
        gamma = two * x[1]
    return price, delta, gamma


def read_grid_f64(V, ri, rd, fit: str = "lu") -> Tuple[float, float, float]:
    """(price, delta, gamma) of one readout as the kernel computes them.
    fit: "lu" the kernel's solve, "lapack" np.linalg.solve, "reversed" the
    kernel's solve with the stencil rows in reverse node order."""
    solve = lapack_solve if fit == "lapack" else lu_solve
    return _read_grid(V, ri, rd, float, solve, reverse=(fit == "reversed"))


def read_grid_exact(V, ri, rd) -> Tuple[Fraction, Fraction, Fraction]:
    return _read_grid(V, ri, rd, Fraction, lu_solve)


def _trade(kind: int, R: Sequence[Tuple], P: Sequence, num) -> Tuple:
    """The FDCN_GK_* combinations of greeks_kernel over read-out triples R."""
    P = [num(float(x)) for x in P]
    zero, half, two, three, four = num(0.0), num(0.5), num(2.0), num(3.0), num(4.0)
    vega = theta = aux = zero
    if kind == GK_BARRIER:
        b, u = R[0], R[1]
        price, delta, gamma = b
        vega = _div(u[0] - b[0], P[5] * 100)
        theta = -(half * P[0] * P[0] * P[1] * P[1] * gamma + (P[2] - P[3]) * P[1] * delta
                  - P[4] * price)
    elif kind == GK_CNLOG:
        b, u, d = R[0], R[1], R[2]
        price, delta, gamma = b
        theta = -(half * P[0] * P[0] * P[1] * P[1] * gamma + P[2] * P[1] * delta - P[3] * price)
        vega = _div(u[0] - d[0], two * P[4])
    elif kind == GK_AMERICAN:
        n1, n2 = R[0], R[1]
        price = (four * n2[0] - n1[0]) / three
        delta = (four * n2[1] - n1[1]) / three
        gamma = (four * n2[2] - n1[2]) / three
        h = P[4]
        first_h = _div(R[2][0] - R[3][0], two * h)
        first_2h = _div(R[4][0] - R[5][0], four * h)
        dvds = (four * first_h - first_2h) / three
        vega = dvds / num(100.0)
        q = zero
        theta = -(half * P[0] * P[0] * P[1] * P[1] * gamma + (P[2] - q) * P[1] * delta
                  - P[3] * price)
        aux = (four * R[6][0] - n1[0]) / three
    elif kind == GK_READOUT:
        price, delta, gamma = R[0]
    else:
        raise ValueError(f"unknown kind {kind}")
    return price, delta, gamma, vega, theta, aux


def _params(P) -> List[float]:
    P = [float(x) for x in P]
    return P + [0.0] * (GK_NPARAM - len(P))


def trade_f64(kind: int, readouts: Sequence[Tuple], P: Sequence[float],
              fit: str = "lu") -> Tuple[float, ...]:
    """The six outputs of one trade as greeks_kernel computes them.
    readouts: (V, ri, rd) triples, READOUTS[kind] of them."""
    assert len(readouts) == READOUTS[kind]
    return _trade(kind, [read_grid_f64(V, ri, rd, fit) for V, ri, rd in readouts],
                  _params(P), float)


def trade_exact(kind: int, readouts: Sequence[Tuple], P: Sequence[float]) -> Tuple[Fraction, ...]:
    assert len(readouts) == READOUTS[kind]
    return _trade(kind, [read_grid_exact(V, ri, rd) for V, ri, rd in readouts], _params(P),
                  Fraction)


def triples(rds: Sequence[Readout], vectors: Sequence[np.ndarray]) -> List[Tuple]:
    """session.Readout objects (slot = index into `vectors`) as (V, ri, rd)."""
    return [(vectors[r.slot], (r.slot, r.icase, r.ilo, r.idx, r.dg_mode), r.dbl) for r in rds]


def readout_scale(V, ri, rd) -> Tuple[float, float, float]:
    """(p, d, g) of the module docstring for one readout."""
    icase, ilo, idx, mode = (int(x) for x in ri[1:5])
    a = lambda i: abs(float(V[i]))  # noqa: E731
    p = a(0) if icase == 1 else a(ilo) if icase == 2 else max(a(ilo), a(ilo + 1))
    if mode == 0:
        return p, 0.0, 0.0
    k = 3 if mode == 1 else 4
    nodes = [float(x) for x in rd[4:4 + k]]
    h = min(b - c for b, c in zip(nodes[1:], nodes[:-1]))
    vmax = max(a(idx - 1 + j) for j in range(k))
    return p, vmax / h, vmax / (h * h)


def trade_scale(kind: int, readouts: Sequence[Tuple], P: Sequence[float]) -> Tuple[float, ...]:
    """scale of the six outputs (module docstring)."""
    signed = _params(P)
    P = [abs(x) for x in signed]
    s = [readout_scale(*r) for r in readouts]

    def theta(carry, r, p, d, g):
        return 0.5 * P[0] * P[0] * P[1] * P[1] * g + carry * P[1] * d + r * p
    if kind == GK_BARRIER:
        p, d, g = s[0]
        return (p, d, g, (s[1][0] + p) / (P[5] * 100),
                theta(abs(signed[2] - signed[3]), P[4], p, d, g), 0.0)
    if kind == GK_CNLOG:
        p, d, g = s[0]
        return p, d, g, (s[1][0] + s[2][0]) / (2.0 * P[4]), theta(P[2], P[3], p, d, g), 0.0
    if kind == GK_AMERICAN:
        p, d, g = ((4.0 * s[1][k] + s[0][k]) / 3.0 for k in range(3))
        h = P[4]
        vega = (4.0 * (s[2][0] + s[3][0]) / (2.0 * h) + (s[4][0] + s[5][0]) / (4.0 * h)) / 300.0
        return p, d, g, vega, theta(P[2], P[3], p, d, g), (4.0 * s[6][0] + s[0][0]) / 3.0
    p, d, g = s[0]
    return p, d, g, 0.0, 0.0, 0.0


def _ratio(err: float, bound: float) -> float:
    if bound > 0.0:
        return err / bound
    return 0.0 if err == 0.0 else math.inf


@dataclass
class TradeYardstick:
    exact: Tuple[Fraction, ...]
    real: Dict[str, Tuple[float, ...]]
    scale: Tuple[float, ...]

    def err(self, got: Sequence[float]) -> List[float]:
        return [float(abs(Fraction(float(g)) - e)) if math.isfinite(g) else math.inf
                for g, e in zip(got, self.exact)]

    def bounds(self, exclude: Optional[str] = None) -> List[float]:
        errs = [self.err(v) for k, v in self.real.items() if k != exclude]
        return [FACTOR * max(max(e[i] for e in errs), 2.0 * U * self.scale[i])
                for i in range(len(OUTPUTS))]

    def ratios(self, got: Sequence[float], exclude: Optional[str] = None) -> List[float]:
        return [_ratio(e, b) for e, b in zip(self.err(got), self.bounds(exclude))]


def trade_yardstick(kind: int, readouts: Sequence[Tuple], P: Sequence[float]) -> TradeYardstick:
    return TradeYardstick(trade_exact(kind, readouts, P),
                          {f: trade_f64(kind, readouts, P, f) for f in REALISATIONS},
                          trade_scale(kind, readouts, P))


# ---------------------------------------------------------------------------
# spline
# ---------------------------------------------------------------------------
def _spline_cont(s: List, v: List, D, num, q_of=None) -> List:
    """Continuation values V(s_i - D) through the natural cubic spline, in
    fdcn_dividend_jump's operation order, in the number type `num`."""
    n = len(s)
    three, two = num(3.0), num(2.0)
    zero = num(0.0)
    h = [s[i + 1] - s[i] for i in range(n - 1)]
    alpha = [zero] * n
    for i in range(1, n - 1):
        alpha[i] = three / h[i] * (v[i + 1] - v[i]) - three / h[i - 1] * (v[i] - v[i - 1])
    l, mu, z, c = [num(1.0)] * n, [zero] * n, [zero] * n, [zero] * n
    for i in range(1, n - 1):
        l[i] = two * (s[i + 1] - s[i - 1]) - h[i - 1] * mu[i - 1]
        mu[i] = h[i] / l[i]
        z[i] = (alpha[i] - h[i - 1] * z[i - 1]) / l[i]
    b, d = [zero] * (n - 1), [zero] * (n - 1)
    for j in range(n - 2, -1, -1):
        c[j] = z[j] - mu[j] * c[j + 1]
        b[j] = (v[j + 1] - v[j]) / h[j] - h[j] * (c[j + 1] + two * c[j]) / three
        d[j] = (c[j + 1] - c[j]) / (three * h[j])
    out = []
    for i in range(n):
        q = s[i] - D
        if q <= s[0]:
            cont = v[0]
        elif q >= s[n - 1]:
            cont = v[n - 1]
        else:
            j = min(bisect.bisect_right(s, q) - 1, n - 2)
            t = q - s[j]
            cont = v[j] + b[j] * t + c[j] * t * t + d[j] * t * t * t
        out.append(cont)
    return out


def _exercise(s: List, cont: List, K, zero) -> List:
    """max(cont, max(s - K, 0)) for a call (K >= 0, -0.0 included)."""
    if not K >= zero:
        return cont
    out = []
    for si, ci in zip(s, cont):
        e = si - K
        ex = zero if zero > e else e
        out.append(ex if ex > ci else ci)
    return out


def _floats(a) -> List[float]:
    return [float(x) for x in a]


def jump_f64(s, v, D: float, K: float = -1.0) -> np.ndarray:
    """fdcn_dividend_jump (csrc/fdcn_host.hip) restated in Python floats."""
    s, v = _floats(s), _floats(v)
    return np.array(_exercise(s, _spline_cont(s, v, float(D), float), float(K), 0.0))


def jump_f64_mirror(s, v, D: float, K: float = -1.0) -> np.ndarray:
    s, v = _floats(s), _floats(v)
    cont = _spline_cont([-x for x in reversed(s)], v[::-1], -float(D), float)[::-1]
    return np.array(_exercise(s, cont, float(K), 0.0))


def jump_exact(s, v, D: float, K: float = -1.0) -> List[Fraction]:
    s, v = [Fraction(x) for x in _floats(s)], [Fraction(x) for x in _floats(v)]
    return _exercise(s, _spline_cont(s, v, Fraction(float(D)), Fraction), Fraction(float(K)),
                     Fraction(0))


def jump_ld(s, v, D: float, K: float = -1.0) -> np.ndarray:
    ld = np.longdouble
    s, v = [ld(x) for x in _floats(s)], [ld(x) for x in _floats(v)]
    return np.array(_exercise(s, _spline_cont(s, v, ld(float(D)), ld), ld(float(K)), ld(0.0)),
                    dtype=np.longdouble)


@dataclass
class JumpYardstick:
    exact: list                     # Fractions, or an np.longdouble array
    real: Dict[str, np.ndarray]
    scale: float

    def err(self, got) -> float:
        got = np.asarray(got, np.float64)
        if not np.all(np.isfinite(got)):
            return math.inf
        if isinstance(self.exact, np.ndarray):
            return float(np.max(np.abs(got.astype(np.longdouble) - self.exact)))
        return float(max(abs(Fraction(float(g)) - e) for g, e in zip(got, self.exact)))

    def bound(self, exclude: Optional[str] = None) -> float:
        N = max(self.err(v) for k, v in self.real.items() if k != exclude)
        return FACTOR * max(N, 2.0 * U * self.scale)

    def ratio(self, got, exclude: Optional[str] = None) -> float:
        return _ratio(self.err(got), self.bound(exclude))


@functools.lru_cache(maxsize=None)
def _jump_yardstick(s: tuple, v: tuple, D: float, K: float) -> JumpYardstick:
    exact = jump_exact(s, v, D, K) if len(s) <= 257 else jump_ld(s, v, D, K)
    return JumpYardstick(exact, {"f64": jump_f64(s, v, D, K),
                                 "mirror": jump_f64_mirror(s, v, D, K)},
                         max(abs(x) for x in v))


def jump_yardstick(s, v, D: float, K: float = -1.0) -> JumpYardstick:
    """Exact for n <= 257, long double above (check HAVE_LD first)."""
    return _jump_yardstick(tuple(_floats(s)), tuple(_floats(v)), float(D), float(K))


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------
def geometric_grid(n: int, x0: float, dx: float) -> List[float]:
    return [math.exp(x0 + i * dx) for i in range(n)]


def option_values(s: Sequence[float], strike: float, amp: float, centre: float,
                  width: float) -> np.ndarray:
    """A put payoff kink at `strike` plus a smooth bump."""
    s = np.asarray(s, np.float64)
    return np.maximum(strike - s, 0.0) + amp * np.exp(-((np.log(s) - math.log(centre)) / width) ** 2)


@dataclass
class GreeksCases:
    """vectors: the host value vectors (Readout.slot indexes this list);
    uploads: lists of vector indices of one length each, one Session.upload
    per entry; trades: (kind, [Readout], params); family: one label per
    trade; accuracy: whether the trade is in the accuracy set."""
    vectors: List[np.ndarray] = field(default_factory=list)
    uploads: List[List[int]] = field(default_factory=list)
    trades: List[tuple] = field(default_factory=list)
    family: List[str] = field(default_factory=list)
    accuracy: List[bool] = field(default_factory=list)

    def add_upload(self, vs: Sequence[np.ndarray]) -> List[int]:
        ids = list(range(len(self.vectors), len(self.vectors) + len(vs)))
        self.vectors.extend(np.asarray(v, np.float64) for v in vs)
        self.uploads.append(ids)
        return ids

    def add(self, family: str, kind: int, rds: List[Readout], P, accuracy: bool = True) -> None:
        self.trades.append((kind, rds, tuple(float(x) for x in P)))
        self.family.append(family)
        self.accuracy.append(accuracy)

    def triples(self, t: int) -> List[Tuple]:
        return triples(self.trades[t][1], self.vectors)


def cubic_readout(slot: int, s: Sequence[float], S_i: float, S_dg: float, idx: int) -> Readout:
    return readout(slot, s, S_i, S_dg, dg_mode=2, idx=idx)


NS = (5, 6, 66, 2049)


def greeks_cases(seed: int = 0) -> GreeksCases:
    """The edge families of the Greeks epilogue (module docstring), on
    vectors of n in NS (one upload per n), a uniform dyadic grid (ties), a
    grid with spacings in ratio 10^6 (dg_mode 1) and a short vector under a
    longer grid (ilo = n_v - 1 < n - 1)."""
    rng = np.random.default_rng(seed)
    C = GreeksCases()
    grids: Dict[int, List[float]] = {}
    P_am = lambda S: (0.2 + 0.3 * rng.random(), S, 0.03, 0.05, 1e-3)  # noqa: E731
    for n in NS:
        dx = 10.0 ** rng.uniform(-3.5, -1.0) if n < 2049 else 10.0 ** -3.5
        x0 = math.log(100.0) - 0.5 * (n - 1) * dx
        s = geometric_grid(n, x0, dx)
        vs = [option_values(s, 100.0 * math.exp(rng.uniform(-1, 1) * dx), rng.uniform(0.5, 5.0),
                            100.0, max(3 * dx, 0.05)) for _ in range(7)]
        ids = C.add_upload(vs)
        grids[n] = s
        a = ids[0]
        # price branch
        C.add("icase1", GK_READOUT, [readout(a, s, 0.5 * s[0])], ())
        C.add("icase2", GK_READOUT, [readout(a, s, 2.0 * s[-1])], ())
        C.add("ilo0", GK_READOUT, [readout(a, s, 0.5 * (s[0] + s[1]))], ())
        C.add("ilo_n-2", GK_READOUT, [readout(a, s, 0.5 * (s[-2] + s[-1]))], ())
        C.add("w0", GK_READOUT, [readout(a, s, s[n // 2])], ())
        C.add("ulp_below_hi", GK_READOUT, [readout(a, s, math.nextafter(s[n // 2], 0.0))], ())
        # 3-point stencil at both ends, inside barrier / CN-log trades
        for idx in (1, n - 2):
            rb = readout(a, s, s[idx] * (1 + 0.3 * dx), s[idx], dg_mode=1, idx=idx)
            C.add("mode1", GK_BARRIER, [rb, readout(ids[1], s, rb.dbl[0])],
                  (0.25, s[idx], 0.04, 0.01, 0.05, 1e-4))
            C.add("mode1", GK_CNLOG, [rb, readout(ids[1], s, rb.dbl[0]),
                                      readout(ids[2], s, rb.dbl[0])],
                  (0.25, s[idx], 0.03, 0.05, 1e-3))
        rb = readout(a, s, 100.0, 100.0, dg_mode=1)  # idx from nearest_interior
        C.add("mode1", GK_READOUT, [rb], ())
        # cubic: both ends, each stencil node, outside by 1 and by 50 spacings
        for idx in sorted({1, n - 3, min(max(n // 2, 1), n - 3)}):
            h = s[idx + 1] - s[idx]
            C.add("cubic", GK_READOUT, [cubic_readout(a, s, s[idx] + 0.3 * h, s[idx] + 0.3 * h,
                                                      idx)], ())
            for k in (-1, 0, 1, 2):
                C.add("on_node", GK_READOUT, [cubic_readout(a, s, s[idx + k], s[idx + k], idx)], ())
            for sign, base in ((-1, s[idx - 1]), (1, s[idx + 2])):
                C.add("outside1", GK_READOUT, [cubic_readout(a, s, s[idx], base + sign * h, idx)],
                      ())
                C.add("far", GK_READOUT, [cubic_readout(a, s, s[idx], base + sign * 50 * h, idx)],
                      (), accuracy=False)
            S = s[idx] + 0.4 * h
            rds = [cubic_readout(ids[0], s, S, S, idx), cubic_readout(ids[1], s, S, S, idx)]
            rds += [readout(ids[k], s, S) for k in (2, 3, 4, 5, 6)]
            C.add("american", GK_AMERICAN, rds, P_am(S))
    # uniform dyadic stencil: S_dg at its midpoint, |z^3| equal in rows 0 and 3
    for n, h in ((6, 0.25), (9, 0.5), (66, 2.0 ** -6)):
        s = [64.0 + i * h for i in range(n)]
        vs = [option_values(s, s[n // 2] + 0.3 * h, rng.uniform(0.5, 5.0), s[n // 2], 0.05)
              + rng.uniform(0.0, 0.3, n) for _ in range(3)]
        ids = C.add_upload(vs)
        for a in ids:
            for idx in sorted({1, n // 2 - 1, n - 3}):
                mid = 0.5 * (s[idx] + s[idx + 1])
                C.add("tie", GK_READOUT, [cubic_readout(a, s, mid, mid, idx)], ())
    # spacings in ratio 10^6 around the 3-point stencil
    n = 6
    s = [100.0]
    for i in range(n - 1):
        s.append(s[-1] + (1e-4 if i % 2 == 0 else 100.0))
    ids = C.add_upload([option_values(s, 150.0, 2.0, 200.0, 0.5),
                        option_values(s, 210.0, 1.0, 200.0, 0.3)])
    for a in ids:
        for idx in (1, n - 2):
            C.add("mode1_ratio", GK_READOUT, [readout(a, s, s[idx], s[idx], dg_mode=1, idx=idx)],
                  ())
    # a vector one node shorter than its grid (the barrier march drops the top node)
    n = 66
    s = grids[n] + [grids[n][-1] * 1.01]
    a = C.uploads[2][0]
    assert len(C.vectors[a]) == n
    rb = readout(a, s, 2.0 * s[-1], s[n // 2], dg_mode=1, n_v=n)
    assert (rb.icase, rb.ilo) == (2, n - 1) and rb.ilo < len(s) - 1
    C.add("icase2_nv", GK_BARRIER, [rb, readout(a + 1, s, 2.0 * s[-1], n_v=n)],
          (0.3, s[n // 2], 0.04, 0.0, 0.05, 1e-4))
    # special values
    n = 6
    s = geometric_grid(n, math.log(90.0), 0.05)
    sp = np.array([-0.0, 5e-324, 1.5, math.inf, math.nan, 2.0])
    nan_unused = np.array([7.0, 6.0, 4.5, 3.5, 3.0, math.nan])
    ids = C.add_upload([sp, nan_unused])
    C.add("special", GK_READOUT, [readout(ids[0], s, 0.5 * s[0])], (), False)           # -0.0
    C.add("special", GK_READOUT, [readout(ids[0], s, s[1])], (), False)                 # subnormal, w = 0
    C.add("special", GK_READOUT, [readout(ids[0], s, 0.5 * (s[0] + s[1]), s[1], 1, 1)], (), False)
    C.add("special", GK_READOUT, [readout(ids[0], s, 0.5 * (s[2] + s[3]), s[2], 1, 2)], (), False)
    C.add("special", GK_READOUT, [readout(ids[0], s, 0.5 * (s[3] + s[4]), s[4], 1, 4)], (), False)
    C.add("special", GK_READOUT, [readout(ids[0], s, 2.0 * s[-1])], (), False)
    C.add("special", GK_READOUT, [cubic_readout(ids[0], s, s[1], s[1], 1)], (), False)  # inf used
    C.add("special", GK_READOUT, [readout(ids[1], s, s[1] * 1.01, s[1], 1, 1)], (), False)
    C.add("nan_unused", GK_READOUT, [cubic_readout(ids[1], s, s[2] * 1.01, s[2] * 1.01, 2)], ())
    C.add("special", GK_READOUT, [cubic_readout(ids[1], s, s[3], s[3], 3)], (), False)  # NaN used
    return C


def uses_cubic(trade: tuple) -> bool:
    return any(r.dg_mode == 2 for r in trade[1])


def flatten(trades: Sequence[tuple], slot_of, order: Optional[Sequence[int]] = None):
    """greeks_raw arrays for `trades`, the readout blocks laid out in `order`
    (a permutation of the trades: `first` is then not monotone).  A trade
    whose readout list is the same object as an earlier one's shares its
    block.  slot_of maps Readout.slot to the device slot."""
    T = len(trades)
    order = list(range(T)) if order is None else list(order)
    kind = np.array([t[0] for t in trades], np.int32).reshape(T)
    first = np.zeros(T, np.int32)
    tp = np.zeros((T, GK_NPARAM))
    rint, rdbl, seen = [], [], {}
    for t in order:
        k, rds, par = trades[t]
        tp[t, :len(par)] = par
        if id(rds) in seen:
            first[t] = seen[id(rds)]
            continue
        first[t] = seen[id(rds)] = len(rint)
        for r in rds:
            rint.append((slot_of(r.slot), r.icase, r.ilo, r.idx, r.dg_mode))
            rdbl.append(r.dbl)
    return (kind, first, tp, np.array(rint, np.int32).reshape(-1, GK_NRINT),
            np.array(rdbl, np.float64).reshape(-1, GK_NRDBL))


JUMP_NS = (2, 3, 4, 63, 64, 65, 257)
JUMP_BS = (1, 70)
JUMP_GRIDS = ("uniform", "geometric", "ratio")


def jump_grid(kind: str, n: int, b: int = 0) -> List[float]:
    if kind == "uniform":
        return [64.0 + 8.0 * b + 0.25 * i for i in range(n)]
    if kind == "geometric":
        dx = 10.0 ** (-3.5 + 2.5 * ((b * 7 + n) % 11) / 10.0)
        return geometric_grid(n, math.log(100.0) - 0.5 * (n - 1) * dx, dx)
    s = [50.0 + b]
    for i in range(n - 1):
        s.append(s[-1] + (1e-4 if (i + b) % 2 == 0 else 100.0))
    return s


def jump_case(kind: str, n: int, B: int, seed: int = 0):
    """(s [B, n], v [B, n], D [B], K [B]): different data per vector; D
    cycles through {0, tiny, mid-grid, beyond the grid, negative} (multiples
    of the spacing on the uniform grid, so q lands on nodes), K through
    {-1, -0.0, 0.0, mid-grid}."""
    rng = np.random.default_rng([seed, n, B, JUMP_GRIDS.index(kind)])
    S, V, Ds, Ks = [], [], [], []
    i_n = JUMP_NS.index(n) if n in JUMP_NS else 2
    off = (i_n + 2 * JUMP_GRIDS.index(kind)) % 5 if B == 1 else 0
    for b in range(B):
        s = jump_grid(kind, n, b)
        span, mid = s[-1] - s[0], s[n // 2]
        if kind == "uniform":
            h = s[1] - s[0]
            D = (0.0, h, (n // 2) * h, (n + 1) * h, -2 * h)[(b + off) % 5]
        else:
            D = (0.0, 1e-9 * s[0], s[n // 2] - s[0] if n > 2 else 0.4 * span, 1.5 * span,
                 -0.3 * span)[(b + off) % 5]
        K = (-1.0, -0.0, 0.0, mid)[(b + off // 2 + (b + off) // 5) % 4]
        v = (option_values(s, mid + 0.3 * (s[1] - s[0]), rng.uniform(0.5, 5.0), mid,
                           max(0.05, 3 * math.log(s[1] / s[0])))
             + rng.uniform(0.0, 0.05, n))
        S.append(s), V.append(v), Ds.append(D), Ks.append(K)
    return np.array(S), np.array(V), np.array(Ds), np.array(Ks)


def jump_accuracy_rows(B: int) -> List[int]:
    """Rows of a jump_case in the accuracy set: every row of B = 1, the
    first five (one per kind of D) of a larger batch up to n = 65."""
    return [0] if B == 1 else list(range(5))
