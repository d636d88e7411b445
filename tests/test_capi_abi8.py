"""ABI 8: fdcn_session_upload, fdcn_session_knockout and fdcn_session_march_ps
exist, and each checks its arguments before it touches a session or a device
(CPU only: the calls below never get that far)."""
import ctypes

import numpy as np
import pytest

from finite_difference_amd import capi, session

NEW = ("fdcn_session_upload", "fdcn_session_knockout", "fdcn_session_march_ps")


def _lib():
    L = capi.lib()
    session._bind(L)
    return L


def test_abi_version_is_8_and_the_calls_are_exported():
    L = _lib()
    assert L.fdcn_abi_version() == 8 == capi.ABI_VERSION
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(raw, name), name


def _p(a):
    return None if a is None else a.ctypes.data


def _err():
    return capi.lib().fdcn_last_error().decode()


def _knockout(B=2, n=9, slots=True, lo=True, hi=True, reb=True):
    sl = np.arange(B if B > 0 else 1, dtype=np.int32)
    a = np.zeros(max(B, 1), np.int32)
    r = np.zeros(max(B, 1))
    # no session (NULL): a valid argument set is stopped there, a bad one earlier
    return _lib().fdcn_session_knockout(None, B, n, _p(sl) if slots else None,
                                        _p(a) if lo else None, _p(a) if hi else None,
                                        _p(r) if reb else None, None)


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B >= 1"), (dict(B=-3), "B >= 1"), (dict(n=0), "n_nodes >= 1"),
    (dict(slots=False), "NULL argument"), (dict(lo=False), "NULL argument"),
    (dict(hi=False), "NULL argument"), (dict(reb=False), "NULL argument"),
    (dict(), "NULL session")])
def test_knockout_rejects_bad_arguments_without_a_device(kw, word):
    assert _knockout(**kw) == -1
    assert word in _err(), _err()


def _upload(B=2, n=9, v=True, out=True):
    V = np.zeros((max(B, 1), max(n, 1)))
    o = np.zeros(max(B, 1), np.int32)
    return _lib().fdcn_session_upload(None, B, n, _p(V) if v else None, _p(o) if out else None)


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B >= 1"), (dict(n=0), "n_nodes >= 1"), (dict(v=False), "NULL argument"),
    (dict(out=False), "NULL argument"), (dict(), "NULL session")])
def test_upload_rejects_bad_arguments_without_a_device(kw, word):
    assert _upload(**kw) == -1
    assert word in _err(), _err()


def _march_ps(B=2, n=20, it=1, ps=True):
    P = np.zeros((max(B, 1), capi.NPARAM))
    P[:, capi.P_DT] = 0.01
    I = np.zeros((max(B, 1), capi.NIPARAM), np.int32)
    I[:, capi.I_KO_LO], I[:, capi.I_KO_HI] = -1, 1 << 20
    sl = np.arange(max(B, 1), dtype=np.int32)
    out = np.zeros(max(B, 1), np.int32)
    z = np.zeros(1, np.int32)
    zd = np.zeros(1)
    return _lib().fdcn_session_march_ps(None, it, B, n, 10, 2, _p(P), _p(I), None, _p(sl),
                                        _p(sl) if ps else None, 0, _p(z), _p(zd), _p(out))


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B >= 1"), (dict(n=0), "n_nodes >= 1"), (dict(ps=False), "NULL payoff_slots"),
    (dict(it=0), "IT march"), (dict(), "NULL session")])
def test_march_ps_rejects_bad_arguments_without_a_device(kw, word):
    assert _march_ps(**kw) == -1
    assert word in _err(), _err()
