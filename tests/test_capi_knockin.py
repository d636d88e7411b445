"""fdcn_session_knockin is exported, joined the surface without a change of
the ABI version, and checks its arguments before it touches a session or a
device (CPU only: the calls below never get that far)."""
import ctypes

import numpy as np
import pytest

from finite_difference_amd import capi, session


def _lib():
    L = capi.lib()
    session._bind(L)
    return L


def test_the_symbol_is_additive_to_abi_8():
    assert _lib().fdcn_abi_version() == 8 == capi.ABI_VERSION
    assert "fdcn_session_knockin" in capi.EXPORTED
    assert hasattr(ctypes.CDLL(capi.LIB_PATH), "fdcn_session_knockin")
    header = open(capi.HEADER_PATH).read()
    assert "#define FDCN_ABI_VERSION 8" in header and "int fdcn_session_knockin(" in header


def _p(a):
    return None if a is None else a.ctypes.data


def _knockin(B=2, n=9, slots=True, src=True, lo=True, hi=True):
    sl = np.arange(max(B, 1), dtype=np.int32)
    ss = sl + max(B, 1)
    a = np.zeros(max(B, 1), np.int32)
    # no session (NULL): a valid argument set is stopped there, a bad one earlier
    return _lib().fdcn_session_knockin(None, B, n, _p(sl) if slots else None,
                                       _p(ss) if src else None, _p(a) if lo else None,
                                       _p(a) if hi else None)


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B >= 1"), (dict(B=-3), "B >= 1"), (dict(n=0), "n_nodes >= 1"),
    (dict(slots=False), "NULL argument"), (dict(src=False), "NULL argument"),
    (dict(lo=False), "NULL argument"), (dict(hi=False), "NULL argument"),
    (dict(), "NULL session")])
def test_knockin_rejects_bad_arguments_without_a_device(kw, word):
    assert _knockin(**kw) == -1
    assert word in capi.lib().fdcn_last_error().decode()


def test_session_binding_checks_shapes_before_the_call():
    class NoDevice(session.Session):
        def __init__(self):  # the argument checks need no session
            self._L, self._h = _lib(), None

        def __del__(self):
            pass
    S = NoDevice()
    for args in (([0, 1], 9, [-1], [9, 9], [2, 3]), ([0, 1], 9, [-1, -1], [9], [2, 3]),
                 ([0, 1], 9, [-1, -1], [9, 9], [2]), ([[0, 1]], 9, [-1], [9], [2])):
        with pytest.raises(ValueError, match="knockin"):
            S.knockin(*args)
