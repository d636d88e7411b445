"""fdcn_session_exercise and fdcn_session_exercise_regions on the MI355X.

The exercise event is bit-identical to the NumPy statement
``np.where(knocked, np.maximum(floor, R), np.maximum(V, floor))``, in place,
and writes nothing outside [0, n_nodes) of each slot: the vectors lie between
two sentinel rows of the same upload, which come back untouched, and the floor
slots come back unchanged.  The region records are (lo, hi, count) of the
nodes that are not knocked and have floor_j > V_j, (n, -1, 0) without any."""
import copy

import numpy as np
import pytest

from finite_difference_amd import capi
from finite_difference_amd.session import Session
from test_gpu_session_knockout import REBATES, thresholds

pytestmark = pytest.mark.gpu


def regions(v, floor, knocked):
    out = []
    for vb, fb, kb in zip(v, floor, knocked):
        idx = np.nonzero(~kb & (fb > vb))[0]
        out.append((int(idx[0]), int(idx[-1]), len(idx)) if len(idx) else (v.shape[1], -1, 0))
    return np.array(out, dtype=np.int32)


def statement(v, floor, knocked, R):
    return np.where(knocked, np.maximum(floor, R[:, None]), np.maximum(v, floor))


@pytest.mark.parametrize("n", [5, 66, 257, 2049])
@pytest.mark.parametrize("B", [1, 3, 70])
def test_exercise_is_the_numpy_statement_bitwise(B, n):
    rng = np.random.default_rng(2000 * B + n)
    cases = thresholds(n)
    j = np.arange(n)
    with Session() as S:
        for shift in range(len(cases) + 1):  # the last round: no barrier at all
            barrier = shift < len(cases)
            lo = np.array([cases[(b + shift) % len(cases)][0] for b in range(B)], np.int32)
            hi = np.array([cases[(b + shift) % len(cases)][1] for b in range(B)], np.int32)
            R = np.array([REBATES[(b + shift) % len(REBATES)] for b in range(B)])
            knocked = (j[None, :] <= lo[:, None]) | (j[None, :] >= hi[:, None])
            if not barrier:
                knocked = np.zeros((B, n), dtype=bool)
            floor = rng.uniform(-2.0, 6.0, (B, n))
            floor[:, ::7] = 0.5
            rows = rng.uniform(-1.0, 5.0, (B + 2, n))  # rows 0 and B+1: sentinels
            rows[1:-1, ::5] = floor[:, ::5]            # exact ties
            fs = S.upload(floor)
            sl = S.upload(rows)
            ids = (S.exercise(sl[1:-1], n, fs, lo, hi, R) if barrier
                   else S.exercise(sl[1:-1], n, fs))
            got = S.fetch(sl, n)
            want = rows.copy()
            want[1:-1] = statement(rows[1:-1], floor, knocked, R)
            assert np.array_equal(got[0], rows[0]) and np.array_equal(got[-1], rows[-1])
            assert np.array_equal(got, want), shift
            assert np.array_equal(S.fetch(fs, n), floor)  # the floor is only read
            assert np.array_equal(S.exercise_regions(ids), regions(rows[1:-1], floor, knocked)), \
                shift
            assert np.array_equal(ids, ids[0] + np.arange(B))  # consecutive per session


def region_cases(n):
    """name -> (V, floor, ko_lo, ko_hi) of one vector; V = 1 and floor = 0
    except where the case says otherwise."""
    def base():
        return np.ones(n), np.zeros(n)
    out = {}
    out["none"] = (*base(), -1, n)
    v, f = base()
    f[:] = 2.0
    out["all"] = (v, f, -1, n)
    v, f = base()
    f[0] = 2.0
    out["node_0"] = (v, f, -1, n)
    v, f = base()
    f[n - 1] = 2.0
    out["node_last"] = (v, f, -1, n)
    v, f = base()
    f[[1 % n, n - 2]] = 2.0  # n >= 257: lanes 1 and n - 2 are in different waves
    out["first_and_last_apart"] = (v, f, -1, n)
    v, f = base()
    f[:] = 2.0               # a region interrupted by knocked nodes at both ends
    out["knocked_ends"] = (v, f, n // 4, (3 * n) // 4)
    v, f = base()
    f[:] = v                 # exact ties are not exercised
    f[n // 2] = 2.0
    out["ties"] = (v, f, -1, n)
    v, f = base()
    f[:] = 2.0
    v[[0, n // 2, n - 1]] = np.nan  # a NaN compares false: not counted, and stays NaN
    out["nan_in_v"] = (v, f, -1, n)
    return out


@pytest.mark.parametrize("n", [5, 66, 257, 2049])
def test_regions_at_their_edges(n):
    cases = region_cases(n)
    names = sorted(cases)
    V = np.array([cases[k][0] for k in names])
    F = np.array([cases[k][1] for k in names])
    lo = np.array([cases[k][2] for k in names], np.int32)
    hi = np.array([cases[k][3] for k in names], np.int32)
    R = np.full(len(names), 0.25)
    j = np.arange(n)
    knocked = (j[None, :] <= lo[:, None]) | (j[None, :] >= hi[:, None])
    want = dict(zip(names, regions(V, F, knocked)))
    assert tuple(want["none"]) == (n, -1, 0) and tuple(want["all"]) == (0, n - 1, n)
    assert tuple(want["node_0"]) == (0, 0, 1) and tuple(want["node_last"]) == (n - 1, n - 1, 1)
    assert tuple(want["ties"]) == (n // 2, n // 2, 1)
    assert tuple(want["knocked_ends"]) == (n // 4 + 1, (3 * n) // 4 - 1,
                                           (3 * n) // 4 - n // 4 - 1)
    assert want["nan_in_v"][2] == n - len({0, n // 2, n - 1})
    with Session() as S:
        fs, sl = S.upload(F), S.upload(V)
        ids = S.exercise(sl, n, fs, lo, hi, R)
        got = S.exercise_regions(ids)
        for k, name in enumerate(names):
            assert tuple(got[k]) == tuple(want[name]), name
        out = S.fetch(sl, n)
        ref = statement(V, F, knocked, R)
        ok = ~np.isnan(ref)
        assert np.array_equal(out.view(np.uint64)[ok], ref.view(np.uint64)[ok])
        assert np.array_equal(np.isnan(out), ~ok) and (~ok).sum() == len({0, n // 2, n - 1})
        # records in any order, repeated, and from two calls
        sl2 = S.upload(V[:2])
        ids2 = S.exercise(sl2, n, fs[:2])
        pick = np.array([ids2[1], ids[3], ids[0], ids2[0], ids[3]], np.int32)
        both = np.vstack([got, regions(V[:2], F[:2], np.zeros((2, n), dtype=bool))])
        m = len(names)
        assert np.array_equal(S.exercise_regions(pick), both[[m + 1, 3, 0, m, 3]])
        assert S.exercise_regions([]).shape == (0, 3)


def test_exercise_after_a_march_and_before_the_next():
    """Ordering: the event waits for the march that produced its slots, and
    the next march (another stream) waits for the event."""
    from finite_difference_amd.engine import Engine
    from plan_factory import random_solve
    rng = np.random.default_rng(78)
    n = 257
    solves = [random_solve(rng, n, 40, 2, it=False, ko=False) for _ in range(3)]
    floors = np.array([np.maximum(s.v_init, 0.0) for s in solves])
    for s in solves:
        s.tau_accumulate = True
    ref = Engine().run(solves)
    lo, hi, R = [40, -1, 10], [n, 200, 180], [0.0, 1.0, 0.5]
    j = np.arange(n)
    knocked = np.array([(j <= a) | (j >= b) for a, b in zip(lo, hi)])
    mid = statement(np.array(ref), floors, knocked, np.array(R))
    second = [copy.copy(s) for s in solves]
    for s, v in zip(second, mid):
        s.v_init = v
    want = Engine().run(second)
    with Session() as S:
        e = Engine()
        pay = S.upload(floors)
        s1 = e.march_slots(S, solves, None)
        ids = S.exercise(s1, n, pay, lo, hi, R)
        s2 = e.march_slots(S, second, list(s1))
        assert np.array_equal(S.fetch(s1, n), mid)
        assert np.array_equal(S.fetch(s2, n), np.array(want))
        assert np.array_equal(S.exercise_regions(ids), regions(np.array(ref), floors, knocked))


def test_exercise_rejects_repeated_and_aliased_slots():
    with Session() as S:
        sl = S.upload(np.zeros((4, 16)))
        with pytest.raises(capi.FdcnError, match="twice"):
            S.exercise([sl[0], sl[0]], 16, [sl[2], sl[3]])
        with pytest.raises(capi.FdcnError, match="floor slot"):
            S.exercise([sl[0], sl[1]], 16, [sl[2], sl[0]])
        with pytest.raises(capi.FdcnError, match="nodes"):
            S.exercise([sl[0]], 15, [sl[1]])
        with pytest.raises(capi.FdcnError, match="does not exist"):
            S.exercise_regions([0])
