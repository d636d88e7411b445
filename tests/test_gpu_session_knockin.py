"""fdcn_session_knockin on the MI355X.

The knock-in event is bit-identical to the NumPy statement
``np.where(knocked, src, V)``, in place, reads its source slots only, and
writes nothing outside [0, n_nodes) of each slot: the vectors lie between two
sentinel rows of the same upload (the rows next to them in memory), which
come back untouched."""
import copy

import numpy as np
import pytest

from finite_difference_amd import capi
from finite_difference_amd.engine import Engine
from finite_difference_amd.session import Session
from plan_factory import random_solve

pytestmark = pytest.mark.gpu


def thresholds(n):
    """(ko_lo, ko_hi): none, none with a far upper value, lower only, upper
    only, both, ko_lo = n - 1, ko_hi = 0, crossing."""
    return [(-1, n), (-1, 1 << 30), (n // 3, n), (-1, (2 * n) // 3), (n // 3, (2 * n) // 3),
            (n - 1, n), (-1, 0), ((2 * n) // 3, n // 3)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


SHAPES = [(B, n) for n in (1, 2, 255, 256, 257, 513) for B in (1, 3)] + [(300, 257)]


@pytest.mark.parametrize("B,n", SHAPES)
def test_knockin_is_the_numpy_statement_bitwise(B, n):
    rng = np.random.default_rng(1000 * B + n)
    cases = thresholds(n)
    j = np.arange(n)
    with Session() as S:
        for shift in range(len(cases)):  # another threshold pair for every b
            lo = np.array([cases[(b + shift) % len(cases)][0] for b in range(B)], np.int32)
            hi = np.array([cases[(b + shift) % len(cases)][1] for b in range(B)], np.int32)
            knocked = (j[None, :] <= lo[:, None]) | (j[None, :] >= hi[:, None])
            src = rng.uniform(-2.0, 6.0, (B, n))
            rows = rng.uniform(-1.0, 5.0, (B + 2, n))  # rows 0 and B+1: sentinels
            ss, sl = S.upload(src), S.upload(rows)
            S.knockin(sl[1:-1], n, lo, hi, ss)
            got = S.fetch(sl, n)
            want = rows.copy()
            want[1:-1] = np.where(knocked, src, rows[1:-1])
            assert np.array_equal(got[0], rows[0]) and np.array_equal(got[-1], rows[-1])
            assert np.array_equal(got, want), shift
            assert np.array_equal(S.fetch(ss, n), src)  # the source is only read


def test_nan_and_inf_pass_through():
    n, B = 257, 3
    rng = np.random.default_rng(9)
    src = rng.standard_normal((B, n))
    v = rng.standard_normal((B, n))
    lo, hi = np.array([40, -1, 100], np.int32), np.array([n, 200, 90], np.int32)
    src[0, :5] = [np.nan, np.inf, -np.inf, -0.0, 0.0]
    bits(src)[0, 5] = 0x7FF8_0000_DEAD_BEEF  # a NaN with a payload, knocked
    src[1, 250], src[1, 100] = np.nan, np.nan  # knocked / not knocked
    v[0, 100], v[1, 10] = np.nan, -np.inf     # live nodes: they stay
    bits(v)[1, 11] = 0xFFF8_0000_0000_0001    # a negative NaN with a payload, live
    v[0, 3] = np.nan                          # a knocked node: overwritten
    j = np.arange(n)
    knocked = (j[None, :] <= lo[:, None]) | (j[None, :] >= hi[:, None])
    assert knocked[2].all() and knocked[0, 5] and not knocked[1, 100] and not knocked[1, 11]
    with Session() as S:
        ss, sl = S.upload(src), S.upload(v)
        S.knockin(sl, n, lo, hi, ss)
        got = S.fetch(sl, n)
        assert np.array_equal(bits(got), bits(np.where(knocked, src, v)))
        assert np.array_equal(bits(S.fetch(ss, n)), bits(src))


def test_knockin_after_a_march_and_before_the_next():
    """Ordering: the event waits for the march that produced its slots, and
    the next march waits for the event."""
    rng = np.random.default_rng(78)
    n = 257
    solves = [random_solve(rng, n, 40, 2, it=False, ko=False) for _ in range(3)]
    for s in solves:
        s.tau_accumulate = True
    ref = Engine().run(solves)
    src = rng.uniform(0.0, 30.0, (3, n))
    lo, hi = [40, -1, 10], [n, 200, 180]
    j = np.arange(n)
    mid = [np.where((j <= a) | (j >= b), w, v) for v, w, a, b in zip(ref, src, lo, hi)]
    second = [copy.copy(s) for s in solves]
    for s, v in zip(second, mid):
        s.v_init = v
    want = Engine().run(second)
    with Session() as S:
        e = Engine()
        ss = S.upload(src)
        s1 = e.march_slots(S, solves)
        S.knockin(s1, n, lo, hi, ss)
        s2 = e.march_slots(S, second, list(s1))
        assert np.array_equal(S.fetch(s1, n), np.array(mid))
        assert np.array_equal(S.fetch(s2, n), np.array(want))
        assert np.array_equal(S.fetch(ss, n), src)


def test_knockin_sees_a_source_march_queued_on_another_stream():
    """The coupled chains are different launch groups (Ikonen-Toivanen and
    Crank-Nicolson, here also another step count), so source and destination
    come from different streams: the event waits for both."""
    rng = np.random.default_rng(79)
    n = 513
    dst = [random_solve(rng, n, 24, 2, it=False, ko=False) for _ in range(3)]
    srcs = [random_solve(rng, n, 400, 2, it=True) for _ in range(3)]
    v_ref, w_ref = Engine().run(dst), Engine().run(srcs)
    lo, hi = [100, -1, 50], [n, 300, 400]
    j = np.arange(n)
    want = [np.where((j <= a) | (j >= b), w, v) for v, w, a, b in zip(v_ref, w_ref, lo, hi)]
    with Session() as S:
        e = Engine()
        sv = e.march_slots(S, dst)
        sw = e.march_slots(S, srcs)  # queued just before the event, the longer march
        S.knockin(sv, n, lo, hi, sw)
        assert np.array_equal(S.fetch(sv, n), np.array(want))
        assert np.array_equal(S.fetch(sw, n), np.array(w_ref))


def test_knockin_rejects_bad_arguments_and_launches_nothing():
    rows = np.arange(4 * 16, dtype=np.float64).reshape(4, 16)
    with Session() as S:
        sl = S.upload(rows)
        with pytest.raises(capi.FdcnError, match="twice"):
            S.knockin([sl[0], sl[0]], 16, [-1, -1], [16, 16], [sl[2], sl[3]])
        with pytest.raises(capi.FdcnError, match="source slot"):
            S.knockin([sl[0], sl[1]], 16, [-1, -1], [16, 16], [sl[2], sl[0]])
        with pytest.raises(capi.FdcnError, match="nodes"):
            S.knockin([sl[0]], 15, [15], [15], [sl[1]])
        with pytest.raises(capi.FdcnError, match="B >= 1"):
            S.knockin([], 16, [], [], [])
        with pytest.raises(capi.FdcnError, match="does not exist"):
            S.knockin([sl[0]], 16, [15], [16], [99])
        with pytest.raises(ValueError):
            S.knockin([sl[0], sl[1]], 16, [-1], [16, 16], [sl[2], sl[3]])
        assert S.slots() == 4
        assert np.array_equal(S.fetch(sl, 16), rows)
