"""The extended-precision closed-form fixture (tests/golden/analytic_mp_cases.json,
written by tests/golden/make_golden_analytic_mp.py) and the bound it is used
with.  Needs neither mpmath nor scipy: the GPU tests import only this.

Layout: ``single`` and ``double`` are lists of groups.  A group holds ``P``
(rows of libfdcn's parameter layout: s, b, r, t, x, sigma, h, k for the single
barrier, S, X, L, U, sigma, b, r, T for the double barrier), ``F`` (libfdcn's
flag rows), the exact values as decimal strings and a condition number M per
output.  Overflow groups also hold ``host``: what the host engine did with the
contract ("finite", "nan", "inf" or "raise").

The bound: |got - ref| <= K * 2**-53 * M + 2**-1000, evaluated exactly in
decimal arithmetic (a double converts to Decimal without rounding).
"""
from decimal import Decimal, localcontext
from fractions import Fraction
import math
import warnings

import numpy as np

from conftest import load_golden

FIXTURE = "analytic_mp_cases.json"

# Worst K of the host engines over the committed fixture's non-overflow groups
# (test_analytic_mp.py measures and asserts them); the device gets 16x.
K_HOST = {"single": 2.43, "double": 1.19}
DEVICE_FACTOR = 16.0

_EPS = Fraction(1, 2 ** 53)
_TINY = Fraction(1, 2 ** 1000)


def load():
    return load_golden(FIXTURE)


def groups(fix, engine, overflow=False):
    return [g for g in fix[engine] if bool(g.get("overflow")) == overflow]


def arrays(group):
    return (np.array(group["P"], dtype=np.float64).reshape(-1, 8),
            np.array(group["F"], dtype=np.int32))


def outputs(group, engine):
    """[(name, refs, Ms)] of a group."""
    if engine == "single":
        return [("price", group["price"], group["M_price"]),
                ("vanilla", group["vanilla"], group["M_vanilla"])]
    return [("price", group["price"], group["M"])]


def _frac(ref):
    with localcontext() as ctx:
        ctx.prec = 100
        d = Decimal(ref)
    return Fraction(d)


def k_needed(got, ref, M):
    """Smallest K with |got - ref| <= K * 2**-53 * M + 2**-1000; inf when no K
    does (got not finite, or M == 0 and got differs from ref)."""
    got = float(got)
    if not math.isfinite(got):
        return math.inf
    err = abs(Fraction(got) - _frac(ref)) - _TINY
    if err <= 0:
        return 0.0
    if M == 0.0:
        return math.inf
    return float(err / (_EPS * Fraction(float(M))))


def worst_k(got, refs, Ms):
    """(worst K, its index) of one output column."""
    ks = [k_needed(g, r, m) for g, r, m in zip(got, refs, Ms)]
    i = max(range(len(ks)), key=ks.__getitem__)
    return ks[i], i


def rr_kwargs(p, f, i=0):
    """BarrierEngine's keyword arguments for one fixture row.  Row i spells
    "not crossed" as None (even i) or 'not_crossed' (odd i); both encode to
    the same flag."""
    s, b, r, t, x, sigma, h, k = (float(v) for v in p)
    return dict(s=s, b=b, r=r, t=t, x=x, sigma=sigma, h=h, k=k,
                optionflag="cp"[f[0]], directionflag="ud"[f[1]], in_out_flag="io"[f[2]],
                barrier_status="crossed" if f[3] else (None, "not_crossed")[i % 2],
                rebate_timing_in="hit" if f[4] & 1 else "expiry",
                rebate_timing_out="expiry" if f[4] & 2 else "hit")


def db_kwargs(p, f, m):
    """(DoubleBarrier's constructor arguments, price()'s arguments)."""
    S, X, L, U, sigma, b, r, T = (float(v) for v in p)
    return (dict(S=S, X=X, L=L, U=U, sigma=sigma, callflag="cp"[f[0]],
                 inflag=("in", "out")[f[1]], m=int(m), corrected_put=bool(f[2])),
            dict(b=b, r=r, T=T))


def host_status(fn):
    """What a host engine does with a contract: finite / nan / inf / raise."""
    try:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            vals = [float(v) for v in fn()]
    except (OverflowError, ZeroDivisionError, FloatingPointError):
        return "raise"
    if any(math.isnan(v) for v in vals):
        return "nan"
    if any(math.isinf(v) for v in vals):
        return "inf"
    return "finite"
