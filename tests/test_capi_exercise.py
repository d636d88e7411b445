"""fdcn_session_exercise and fdcn_session_exercise_regions are exported, joined
the surface without a change of the ABI version, and check their arguments
before they touch a session or a device (CPU only: the calls below never get
that far)."""
import ctypes

import numpy as np
import pytest

from finite_difference_amd import capi, session

SYMBOLS = ("fdcn_session_exercise", "fdcn_session_exercise_regions")


def _lib():
    L = capi.lib()
    session._bind(L)
    return L


def test_the_symbols_are_additive_to_abi_8():
    assert _lib().fdcn_abi_version() == 8 == capi.ABI_VERSION
    header = open(capi.HEADER_PATH).read()
    assert "#define FDCN_ABI_VERSION 8" in header
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in SYMBOLS:
        assert name in capi.EXPORTED and hasattr(raw, name) and f"int {name}(" in header


def _p(a):
    return None if a is None else a.ctypes.data


def _exercise(B=2, n=9, slots=True, floor=True, lo=True, hi=True, reb=True, out=True):
    m = max(B, 1)
    sl = np.arange(m, dtype=np.int32)
    fs = sl + m
    a = np.zeros(m, np.int32)
    R = np.zeros(m)
    ids = np.zeros(m, np.int32)
    # no session (NULL): a valid argument set is stopped there, a bad one earlier
    return _lib().fdcn_session_exercise(None, B, n, _p(sl) if slots else None,
                                        _p(fs) if floor else None, _p(a) if lo else None,
                                        _p(a) if hi else None, _p(R) if reb else None,
                                        _p(ids) if out else None)


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B >= 1"), (dict(B=-3), "B >= 1"), (dict(n=0), "n_nodes >= 1"),
    (dict(slots=False), "NULL argument"), (dict(floor=False), "NULL argument"),
    (dict(out=False), "NULL argument"), (dict(lo=False), "go together"),
    (dict(hi=False, reb=False), "go together"), (dict(reb=False), "go together"),
    (dict(), "NULL session"), (dict(lo=False, hi=False, reb=False), "NULL session")])
def test_exercise_rejects_bad_arguments_without_a_device(kw, word):
    assert _exercise(**kw) == -1
    assert word in capi.lib().fdcn_last_error().decode()


def test_exercise_regions_rejects_a_null_session():
    ids = np.zeros(1, np.int32)
    out = np.zeros(3, np.int32)
    assert _lib().fdcn_session_exercise_regions(None, 1, _p(ids), _p(out)) == -1
    assert "NULL session" in capi.lib().fdcn_last_error().decode()


def test_session_binding_checks_shapes_before_the_call():
    class NoDevice(session.Session):
        def __init__(self):  # the argument checks need no session
            self._L, self._h = _lib(), None

        def __del__(self):
            pass
    S = NoDevice()
    for args in (([0, 1], 9, [2]), ([[0, 1]], 9, [2, 3]), ([0, 1], 9, [2, 3], [-1], [9, 9], [0, 0]),
                 ([0, 1], 9, [2, 3], [-1, -1], [9, 9], [0.0]),
                 ([0, 1], 9, [2, 3], [-1, -1], None, [0.0, 0.0]),
                 ([0, 1], 9, [2, 3], None, None, [0.0, 0.0])):
        with pytest.raises(ValueError, match="exercise"):
            S.exercise(*args)
    with pytest.raises(ValueError, match="exercise_regions"):
        S.exercise_regions([[0, 1]])
