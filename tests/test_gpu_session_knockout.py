"""fdcn_session_knockout and fdcn_session_upload on the MI355X.

The knock-out event is bit-identical to the NumPy statement
``np.where(knocked, np.maximum(floor, R), V)`` (``np.where(knocked, R, V)``
without floor slots), in place, and writes nothing outside [0, n_nodes) of
each slot: the vectors lie between two sentinel rows of the same upload (the
rows next to them in memory), which come back untouched."""
import numpy as np
import pytest

from finite_difference_amd.session import Session

pytestmark = pytest.mark.gpu

REBATES = (0.0, -1.5, 2.25, 7.0)


def thresholds(n):
    """(ko_lo, ko_hi): none, none with a far upper value, lower only, upper
    only, both, everything knocked, ko_lo = 0, ko_hi = n - 1."""
    return [(-1, n), (-1, 1 << 30), (n // 3, n), (-1, (2 * n) // 3), (n // 3, (2 * n) // 3),
            (n - 2, n - 1), (0, n), (-1, n - 1)]


@pytest.mark.parametrize("n", [5, 66, 257, 2049])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_knockout_is_the_numpy_statement_bitwise(B, n):
    rng = np.random.default_rng(1000 * B + n)
    cases = thresholds(n)
    j = np.arange(n)
    with Session() as S:
        for shift in range(len(cases)):
            lo = np.array([cases[(b + shift) % len(cases)][0] for b in range(B)], np.int32)
            hi = np.array([cases[(b + shift) % len(cases)][1] for b in range(B)], np.int32)
            R = np.array([REBATES[(b + shift) % len(REBATES)] for b in range(B)])
            knocked = (j[None, :] <= lo[:, None]) | (j[None, :] >= hi[:, None])
            floor = rng.uniform(-2.0, 6.0, (B, n))
            floor[:, ::7] = 0.0
            fs = S.upload(floor)
            for with_floor in (True, False):
                rows = rng.uniform(-1.0, 5.0, (B + 2, n))  # rows 0 and B+1: sentinels
                sl = S.upload(rows)
                S.knockout(sl[1:-1], n, lo, hi, R, fs if with_floor else None)
                got = S.fetch(sl, n)
                want = rows.copy()
                want[1:-1] = np.where(knocked, np.maximum(floor, R[:, None]) if with_floor
                                      else np.broadcast_to(R[:, None], (B, n)), rows[1:-1])
                assert np.array_equal(got[0], rows[0]) and np.array_equal(got[-1], rows[-1])
                assert np.array_equal(got, want), (shift, with_floor)
            assert np.array_equal(S.fetch(fs, n), floor)  # the floor is only read


def test_knockout_after_a_march_and_before_the_next():
    """Ordering: the event waits for the march that produced its slots, and
    the next march (another stream) waits for the event."""
    from finite_difference_amd.engine import Engine
    from plan_factory import random_solve
    rng = np.random.default_rng(77)
    n = 257
    solves = [random_solve(rng, n, 40, 2, it=True) for _ in range(3)]
    for s in solves:
        s.tau_accumulate = True
    ref = Engine().run(solves)
    lo, hi, R = [40, -1, 10], [n, 200, 180], [0.0, 1.0, 0.5]
    j = np.arange(n)
    mid = [np.where((j <= a) | (j >= b), np.maximum(s.payoff, r), v)
           for s, v, a, b, r in zip(solves, ref, lo, hi, R)]
    import copy
    second = [copy.copy(s) for s in solves]
    for s, v in zip(second, mid):
        s.v_init = v
    want = Engine().run(second)
    with Session() as S:
        e = Engine()
        pay = S.upload(np.array([s.payoff for s in solves]))
        s1 = e.march_slots(S, solves, None, list(pay))
        S.knockout(s1, n, lo, hi, R, pay)
        s2 = e.march_slots(S, second, list(s1), list(pay))
        assert np.array_equal(S.fetch(s1, n), np.array(mid))
        assert np.array_equal(S.fetch(s2, n), np.array(want))


def test_upload_round_trips_bitwise():
    rng = np.random.default_rng(5)
    with Session() as S:
        a = rng.standard_normal((7, 513))
        a[0, :3] = [0.0, -0.0, np.inf]
        sa = S.upload(a)
        buf = S.host_buffer(4 * 300)
        buf[:] = rng.standard_normal(4 * 300)
        view = buf.reshape(4, 300)
        sb = S.upload(view)
        assert S.slots() == 11
        assert np.array_equal(S.fetch(sa, 513).view(np.uint64), a.view(np.uint64))
        assert np.array_equal(S.fetch(sb, 300), view)
        assert np.array_equal(S.fetch(sb[::-1], 300), view[::-1])
        del buf, view


def test_knockout_rejects_repeated_and_aliased_slots():
    from finite_difference_amd import capi
    with Session() as S:
        sl = S.upload(np.zeros((3, 16)))
        with pytest.raises(capi.FdcnError, match="twice"):
            S.knockout([sl[0], sl[0]], 16, [-1, -1], [16, 16], [0.0, 0.0])
        with pytest.raises(capi.FdcnError, match="floor slot"):
            S.knockout([sl[0], sl[1]], 16, [-1, -1], [16, 16], [0.0, 0.0], [sl[2], sl[0]])
        with pytest.raises(capi.FdcnError, match="nodes"):
            S.knockout([sl[0]], 15, [-1], [15], [0.0])
