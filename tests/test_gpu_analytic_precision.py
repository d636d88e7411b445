"""The closed-form kernels on the MI355X (rr_barrier_kernel,
double_barrier_kernel) against an 80-digit evaluation of the same formulas:
tests/golden/analytic_mp_cases.json, layout and bound in analytic_mp_fixture.py,
the CPU side in test_analytic_mp.py.

Bound on every non-overflow group, for price and vanilla:

    |gpu - ref| <= K_dev * 2**-53 * M + 2**-1000,    K_dev = 16 * K_host

with the fixture's condition number M.  K_host is the worst K the *host*
engines need over the same fixture (2.43 single, 1.19 double,
test_analytic_mp.py); 16 is the documented ulp bound of the device library's
pow and erfc against 1-2 ulp on the host.  `-s` prints the worst K per group.

The single-barrier rows (all groups, 576 contracts) go through one launch and
the double-barrier rows through one launch per series length m; the tests share
those results.  The module imports neither mpmath nor scipy.
"""
import math

import numpy as np
import pytest

import analytic_mp_fixture as fx
from finite_difference_amd import capi

pytestmark = pytest.mark.gpu
FIX = fx.load()
K_DEV = {e: fx.DEVICE_FACTOR * k for e, k in fx.K_HOST.items()}
CANARY = 0x7FF8C0DEC0DE0001  # a quiet NaN no kernel computes
N_CANARY = 256
SIZES = (1, 255, 256, 257, 513)


def _names(engine, overflow=False):
    return [g["group"] for g in fx.groups(FIX, engine, overflow)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pool(engine):
    """Every row of every group of one engine, overflow rows included."""
    P = np.concatenate([fx.arrays(g)[0] for g in FIX[engine]])
    F = np.concatenate([fx.arrays(g)[1] for g in FIX[engine]])
    return P, F


@pytest.fixture(scope="module")
def single_gpu():
    """{group: (price, vanilla)} from one launch over all single-barrier rows."""
    P, F = _pool("single")
    price, vanilla = capi.rr_barrier_batch(P, F)
    out, at = {}, 0
    for g in FIX["single"]:
        n = len(g["P"])
        out[g["group"]] = dict(price=price[at:at + n], vanilla=vanilla[at:at + n])
        at += n
    assert at == len(P) > 513
    return out


@pytest.fixture(scope="module")
def double_gpu():
    """{group: price}: one launch per series length m."""
    out = {}
    for m in sorted({g["m"] for g in FIX["double"]}):
        gs = [g for g in FIX["double"] if g["m"] == m]
        P = np.concatenate([fx.arrays(g)[0] for g in gs])
        F = np.concatenate([fx.arrays(g)[1] for g in gs])
        price = capi.double_barrier_batch(P, F, m)
        at = 0
        for g in gs:
            out[g["group"]] = dict(price=price[at:at + len(g["P"])])
            at += len(g["P"])
    return out


def _group(engine, name):
    return next(g for g in FIX[engine] if g["group"] == name)


def _assert_bound(engine, g, got):
    for name, refs, Ms in fx.outputs(g, engine):
        k, i = fx.worst_k(got[name], refs, Ms)
        print(f"[mp gpu] {engine} {g['group']:<10} {name:<7} worst K {k:.3f} (row {i}) "
              f"bound {K_DEV[engine]:.2f}")
        assert k <= K_DEV[engine], (g["group"], name, i, g["P"][i], g["F"][i],
                                    float(got[name][i]), refs[i], Ms[i])


@pytest.mark.parametrize("name", _names("single"))
def test_single_barrier_meets_the_bound(single_gpu, name):
    _assert_bound("single", _group("single", name), single_gpu[name])


@pytest.mark.parametrize("name", _names("double"))
def test_double_barrier_meets_the_bound(double_gpu, name):
    """Includes the series lengths: groups m0, m1 and m12 carry m = 0, 1, 12."""
    _assert_bound("double", _group("double", name), double_gpu[name])


def test_series_length_reaches_the_kernel():
    """The m = 1 contracts priced with m = 4 and with m = 0 leave the m = 1
    fixture's bound somewhere: the series length is not ignored."""
    g = _group("double", "m1")
    P, F = fx.arrays(g)
    assert g["m"] == 1
    for m in (0, 4):
        k, _ = fx.worst_k(capi.double_barrier_batch(P, F, m), g["price"], g["M"])
        assert k > K_DEV["double"], (m, k)


def test_double_barrier_zero_branches(double_gpu):
    """Call with X >= U, put with X <= L (X on and past the barrier): the
    knock-out is exactly 0.0, the knock-in is Black-Scholes within its own M."""
    g = _group("double", "x_outside")
    P, F = fx.arrays(g)
    got = double_gpu["x_outside"]["price"]
    n_out = 0
    for i, (p, f) in enumerate(zip(P, F)):
        S, X, L, U = p[:4]
        assert (X <= L) if f[0] else (X >= U)
        if f[1]:  # out
            assert g["M"][i] == 0.0 and float(g["price"][i]) == 0.0
            assert got[i] == 0.0, (i, p, f, got[i])
            n_out += 1
        else:     # in: M holds the two Black-Scholes legs only
            assert fx.k_needed(got[i], g["price"][i], g["M"][i]) <= K_DEV["double"], (i, p, f)
    assert n_out == 12 and sum(p[1] in (p[2], p[3]) for p in P) == 8  # X exactly on L or U


def test_single_barrier_zero_cells_are_exact(single_gpu):
    """Rows whose value has no term at all (M == 0: a zero table cell without
    rebate, a crossed knock-out without rebate) come back as exactly 0.0."""
    n = 0
    for g in fx.groups(FIX, "single"):
        got = single_gpu[g["group"]]["price"]
        for i, M in enumerate(g["M_price"]):
            if M == 0.0:
                assert got[i] == 0.0, (g["group"], i, g["P"][i], g["F"][i], got[i])
                n += 1
    assert n >= 8


@pytest.mark.parametrize("engine", ["single", "double"])
def test_overflow_group_is_nonfinite_or_inside_the_bound(engine, single_gpu, double_gpu):
    """sigma in [0.003, 0.04]: the formulas overflow in doubles.  A device
    result is non-finite or inside the bound, never a finite wrong number, and
    it is finite wherever the host engine's was."""
    res = single_gpu if engine == "single" else double_gpu
    for g in fx.groups(FIX, engine, overflow=True):
        got = res[g["group"]]
        seen = {}
        for i, host in enumerate(g["host"]):
            finite = True
            for name, refs, Ms in fx.outputs(g, engine):
                v = float(got[name][i])
                if math.isfinite(v):
                    k = fx.k_needed(v, refs[i], Ms[i])
                    assert k <= K_DEV[engine], (g["group"], name, i, g["P"][i], g["F"][i], v,
                                                refs[i], Ms[i], k)
                else:
                    finite = False
                    kind = "nan" if math.isnan(v) else "inf"
                    seen[(host, name, kind)] = seen.get((host, name, kind), 0) + 1
            if finite:
                seen[(host, "all", "finite")] = seen.get((host, "all", "finite"), 0) + 1
            if host == "finite":
                assert finite, (g["group"], i, g["P"][i], g["F"][i])
        print(f"[mp gpu] {engine} overflow: (host, output, device) counts {sorted(seen.items())}")


# ---------------------------------------------------------------------------
# the device-pointer entry points and the launch geometry
# ---------------------------------------------------------------------------
def _rows(engine, B):
    P, F = _pool(engine)
    idx = np.arange(B) % len(P)
    return np.ascontiguousarray(P[idx]), np.ascontiguousarray(F[idx])


def _canary_buffer(torch, n, dev):
    buf = torch.empty(n + N_CANARY, dtype=torch.float64, device=dev)
    buf.view(torch.int64).fill_(np.int64(CANARY).item())
    return buf


def _check_canary(buf, B, want):
    got = _bits(buf.cpu().numpy())
    assert np.array_equal(got[:B], _bits(want))          # bitwise, NaNs included
    assert np.all(got[B:] == np.int64(CANARY)) and len(got) == B + N_CANARY


@pytest.mark.parametrize("B", SIZES)
def test_rr_dev_entry_is_the_host_entry_bitwise(B):
    import torch
    P, F = _rows("single", B)
    want_p, want_v = capi.rr_barrier_batch(P, F)
    dev = torch.device("cuda:0")
    dP, dF = torch.from_numpy(P).to(dev), torch.from_numpy(F).to(dev)
    price, vanilla = _canary_buffer(torch, B, dev), _canary_buffer(torch, B, dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()  # the fills above ran on the default stream
    with torch.cuda.stream(stream):
        capi._check(capi.lib().fdcn_rr_barrier_batch_dev(
            B, dP.data_ptr(), dF.data_ptr(), price.data_ptr(), vanilla.data_ptr(),
            stream.cuda_stream))
    stream.synchronize()
    _check_canary(price, B, want_p)
    _check_canary(vanilla, B, want_v)


@pytest.mark.parametrize("B", SIZES)
def test_double_dev_entry_is_the_host_entry_bitwise(B):
    import torch
    P, F = _rows("double", B)
    want = capi.double_barrier_batch(P, F, 4)
    dev = torch.device("cuda:0")
    dP, dF = torch.from_numpy(P).to(dev), torch.from_numpy(F).to(dev)
    price = _canary_buffer(torch, B, dev)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        capi._check(capi.lib().fdcn_double_barrier_batch_dev(
            B, 4, dP.data_ptr(), dF.data_ptr(), price.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    _check_canary(price, B, want)


def test_dev_entries_accept_an_empty_batch():
    """B = 0 is FDCN_OK with null pointers (nothing is launched)."""
    L = capi.lib()
    assert L.fdcn_rr_barrier_batch_dev(0, None, None, None, None, None) == 0
    assert L.fdcn_double_barrier_batch_dev(0, 4, None, None, None, None) == 0
    assert L.fdcn_rr_barrier_batch(0, None, None, None, None) == 0
    assert L.fdcn_double_barrier_batch(0, 4, None, None, None) == 0
    assert L.fdcn_rr_barrier_batch_dev(-1, None, None, None, None, None) != 0
    assert L.fdcn_double_barrier_batch_dev(1, -1, None, None, None, None) != 0


@pytest.mark.parametrize("engine", ["single", "double"])
def test_result_does_not_depend_on_position_or_batch_size(engine):
    """64 contracts alone, and the same 64 at offset 200 of a batch of 513."""
    P, F = _rows(engine, 513 + 64)
    p64, f64 = P[513:], F[513:]
    Pb, Fb = P[:513].copy(), F[:513].copy()
    Pb[200:264], Fb[200:264] = p64, f64
    if engine == "single":
        alone, embedded = capi.rr_barrier_batch(p64, f64), capi.rr_barrier_batch(Pb, Fb)
    else:
        alone = (capi.double_barrier_batch(p64, f64, 4),)
        embedded = (capi.double_barrier_batch(Pb, Fb, 4),)
    for a, e in zip(alone, embedded):
        assert np.array_equal(_bits(a), _bits(e[200:264]))
    assert not np.array_equal(Pb[200:264], P[200:264])  # the 64 differ from what they replaced
