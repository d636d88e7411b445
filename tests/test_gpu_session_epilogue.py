"""greeks_kernel / read_grid and dividend_jump_kernel (csrc/fdcn_session.hip)
called directly on the MI355X, at their edges, against session_epilogue_ref.py.

Greeks: the case families of session_epilogue_ref.greeks_cases (every price
branch, both stencils at the first and last admissible node, S_dg on the
stencil's nodes, at the midpoint of a uniform stencil -- a pivot tie --, one
and fifty spacings outside, spacings in ratio 10^6, special values), vectors
of 5, 6, 66 and 2049 nodes from separate uploads in one launch, T across the
64-thread block boundary with the four kinds interleaved, `first` not
monotone and a shared readout, and every validation branch of
fdcn_session_greeks.

* every output that does not pass through the cubic fit (dg_mode 0 and 1, all
  four kinds) is bit-identical to trade_f64, NaN compared as NaN;
* every output that does is inside the rounding yardstick
  |got - exact| <= 8 max(N, 2 u scale) of session_epilogue_ref.py against
  trade_exact -- and is ALSO bit-identical to trade_f64 on the MI355X, for
  every case (the `far` and special-value families included), which is
  asserted: the kernel's LU is the restated one, operation for operation.
  Measured worst ratio error / bound on the MI355X (printed per family
  under -s): 0.125 for american, cubic, on_node, outside1 and tie (the device
  value is trade_f64, one of the realisations N is taken over), 0.080 for
  nan_unused.

Dividend jump: n in {2, 3, 4, 63, 64, 65, 257} x B in {1, 70} on a uniform
dyadic grid with D = k h (q on nodes: the searchsorted(side="right") tie), a
geometric grid and a grid with spacings in ratio 10^6; D in {0, tiny,
mid-grid, beyond the grid, negative}; strike_call in {-1, -0.0, 0.0,
mid-grid}; different data per vector.  Bit-identical to capi.dividend_jump,
inputs and sentinel rows untouched, the accuracy set inside the yardstick
against the exact natural spline (long double at n = 2049); a jump feeding a
jump feeding a Greeks readout equals the host composition bitwise.  Measured
worst ratios on the MI355X: 0.125 on the geometric and the ratio grid, 0 on
the uniform dyadic grid (every operation exact there).

Not covered: a wrong stride of the kernel's `work` rows.  With 2 n for 3 n,
vector b's c row is vector b+1's mu row; b+1 last reads mu[j] in the backward
step in which b writes c[j], so blocks that run in step (all of one launch
have the same n and the same trip counts) never see the other's value, and
all of these tests still pass.  Different data per vector shows a wrong offset
of `out`, `s`, `cash` and `strike`, not of `work`.
"""
import dataclasses

import numpy as np
import pytest

import session_epilogue_ref as R
from finite_difference_amd import capi
from finite_difference_amd.session import (GK_AMERICAN, GK_BARRIER, GK_CNLOG, GK_NPARAM,
                                           GK_READOUT, Session, readout)

pytestmark = pytest.mark.gpu


def bits_differ(a, b) -> np.ndarray:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    return ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))


def same_bits(a, b) -> bool:
    return not bool(np.any(bits_differ(a, b)))


@pytest.fixture(scope="module")
def cases():
    C = R.greeks_cases()
    want = [R.trade_f64(k, C.triples(t), P) for t, (k, _, P) in enumerate(C.trades)]
    yard = {t: R.trade_yardstick(k, C.triples(t), P)
            for t, (k, rds, P) in enumerate(C.trades) if C.accuracy[t] and R.uses_cubic((k, rds, P))}
    return C, want, yard


def upload_all(S: Session, C: R.GreeksCases) -> list:
    """One Session.upload per group of vectors; flat vector index -> slot."""
    slot = [None] * len(C.vectors)
    for ids in C.uploads:
        for i, sl in zip(ids, S.upload(np.stack([C.vectors[i] for i in ids]))):
            slot[i] = int(sl)
    return slot


def on_device(trades, slot):
    return [(k, [dataclasses.replace(r, slot=slot[r.slot]) for r in rds], P)
            for k, rds, P in trades]


def check_trades(out, idx, cases, label):
    """Rows of `out` against the references of the trades C.trades[idx]."""
    C, want, yard = cases
    worst = {}
    for row, t in zip(out, idx):
        trade = C.trades[t]
        bad = bits_differ(row, want[t])
        assert not bad.any(), (label, t, C.family[t], "cubic" if R.uses_cubic(trade) else "plain",
                               row.tolist(), want[t])
        if t in yard:
            r = max(yard[t].ratios([float(x) for x in row]))
            worst[C.family[t]] = max(worst.get(C.family[t], 0.0), r)
            assert r <= 1.0, (label, t, C.family[t], r)
    for fam in sorted(worst):
        print(f"[{label}] {fam:>12} worst ratio {worst[fam]:.3f}")


def test_every_family_in_one_launch(cases):
    C = cases[0]
    with Session() as S:
        slot = upload_all(S, C)
        assert len({len(C.vectors[ids[0]]) for ids in C.uploads}) >= 5
        out = S.greeks(on_device(C.trades, slot))
    assert out.shape == (len(C.trades), 6)
    check_trades(out, range(len(C.trades)), cases, "families")


def _interleaved(C, T):
    """T trade indices cycling through the four kinds."""
    pool = {k: [t for t, tr in enumerate(C.trades) if tr[0] == k]
            for k in (GK_BARRIER, GK_CNLOG, GK_AMERICAN, GK_READOUT)}
    assert all(pool.values())
    return [pool[i % 4][(i // 4) % len(pool[i % 4])] for i in range(T)]


@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_mixed_kinds_across_the_block_boundary(cases, T):
    C = cases[0]
    idx = _interleaved(C, T)
    with Session() as S:
        slot = upload_all(S, C)
        trades = on_device([C.trades[t] for t in idx], slot)
        if T >= 5:  # the last trade shares the readouts of the one four before it
            idx[T - 1] = idx[T - 5]
            trades[T - 1] = trades[T - 5]
        order = np.random.default_rng(T).permutation(T)
        kind, first, tp, rint, rdbl = R.flatten(trades, lambda s: s, order)
        if T >= 5:
            assert first[T - 1] == first[T - 5]
            assert np.any(np.diff(first) < 0)
        out = S.greeks_raw(kind, first, tp, rint, rdbl)
    assert out.shape == (T, 6)
    check_trades(out, idx, cases, f"T={T}")


def _raw(trade, slot):
    return R.flatten(on_device([trade], slot), lambda s: s)


def test_greeks_validation(cases):
    C, want, _ = cases
    good = next(t for t, tr in enumerate(C.trades) if tr[0] == GK_BARRIER)
    cub = next(t for t in range(len(C.trades)) if C.family[t] == "cubic")
    with Session() as S:
        slot = upload_all(S, C)

        def still_answers():
            out = S.greeks(on_device([C.trades[good]], slot))
            assert same_bits(out[0], want[good])

        def refused(match, kind, first, tp, rint, rdbl):
            with pytest.raises(capi.FdcnError, match=match):
                S.greeks_raw(kind, first, tp, rint, rdbl)
            still_answers()

        kind, first, tp, rint, rdbl = _raw(C.trades[good], slot)
        n = len(C.vectors[C.trades[good][1][0].slot])
        assert rint[0, 4] == 1
        refused("unknown kind 4", np.array([4], np.int32), first, tp, rint, rdbl)
        refused("unknown kind -1", np.array([-1], np.int32), first, tp, rint, rdbl)
        refused(r"outside R=2", kind, np.array([1], np.int32), tp, rint, rdbl)
        refused(r"outside R=2", kind, np.array([-1], np.int32), tp, rint, rdbl)

        def with_int(col, value, row=0, base=rint):
            a = base.copy()
            a[row, col] = value
            return a
        refused("node indices outside", kind, first, tp, with_int(1, 3), rdbl)       # icase 3
        a = with_int(1, 0)
        a[0, 2] = n - 1                                                              # ilo = n-1, icase 0
        refused(f"outside its {n}-node vector", kind, first, tp, a, rdbl)
        refused("node indices outside", kind, first, tp, with_int(3, 0), rdbl)       # mode 1, idx 0
        refused("node indices outside", kind, first, tp, with_int(3, n - 1), rdbl)   # mode 1, idx n-1
        refused("slot 100000 does not exist", kind, first, tp, with_int(0, 100000, row=1), rdbl)
        refused("does not exist", kind, first, tp, with_int(0, -1), rdbl)
        kc, fc, tc, ric, rdc = _raw(C.trades[cub], slot)
        nc = len(C.vectors[C.trades[cub][1][0].slot])
        assert ric[0, 4] == 2
        refused("node indices outside", kc, fc, tc, with_int(3, nc - 2, base=ric), rdc)  # mode 2
        refused("node indices outside", kc, fc, tc, with_int(3, 0, base=ric), rdc)
        empty = S.greeks_raw(np.zeros(0, np.int32), np.zeros(0, np.int32),
                             np.zeros((0, GK_NPARAM)), rint, rdbl)
        assert empty.shape == (0, 6)
        assert S.greeks([]).shape == (0, 6)
        still_answers()


# ------------------------------------------------------------ dividend jump
def _jump_on_device(S, s, v, D, K):
    """Upload v between two sentinel rows, jump the rows in between; returns
    (output vectors, the uploaded rows fetched back afterwards)."""
    B, n = v.shape
    sent = np.full((1, n), -12345.678)
    rows = np.concatenate([sent, v, 2.0 * sent])
    sl = S.upload(rows)
    out = S.dividend_jump(sl[1:-1], s, D, K)
    assert len(set(out.tolist()) | set(sl.tolist())) == 2 * B + 2
    return S.fetch(out, n), S.fetch(sl, n), rows


@pytest.mark.parametrize("B", R.JUMP_BS)
@pytest.mark.parametrize("kind", R.JUMP_GRIDS)
def test_dividend_jump_shapes(kind, B):
    worst = 0.0
    with Session() as S:
        for n in R.JUMP_NS:
            s, v, D, K = R.jump_case(kind, n, B)
            got, back, rows = _jump_on_device(S, s, v, D, K)
            assert same_bits(back, rows), (kind, n, B)  # inputs and sentinels untouched
            for b in range(B):
                want = capi.dividend_jump(s[b], v[b], D[b], K[b])
                assert same_bits(got[b], want), (kind, n, B, b, float(D[b]), float(K[b]))
            if B == 1 or n <= 65:
                for b in R.jump_accuracy_rows(B):
                    r = R.jump_yardstick(s[b], v[b], D[b], K[b]).ratio(got[b])
                    worst = max(worst, r)
                    assert r <= 1.0, (kind, n, B, b, r)
    print(f"[jump {kind} B={B}] worst ratio {worst:.3f}")


@pytest.mark.skipif(not R.HAVE_LD, reason="np.longdouble has no 64-bit mantissa here")
def test_dividend_jump_2049_against_long_double():
    cs = [R.jump_case(kind, 2049, 1) for kind in R.JUMP_GRIDS]
    s, v, D, K = (np.concatenate([c[i] for c in cs]) for i in range(4))
    with Session() as S:
        got, back, rows = _jump_on_device(S, s, v, D, K)
    assert same_bits(back, rows)
    for b, kind in enumerate(R.JUMP_GRIDS):
        assert same_bits(got[b], capi.dividend_jump(s[b], v[b], D[b], K[b])), kind
        r = R.jump_yardstick(s[b], v[b], D[b], K[b]).ratio(got[b])
        print(f"[jump {kind} n=2049] ratio {r:.3f}")
        assert r <= 1.0, (kind, r)


def test_jump_into_jump_into_greeks_equals_host_composition():
    """Three vectors from three uploads (three streams), two jumps, one
    epilogue: every consumer has to wait for its producers."""
    n = 65
    s, v, D, K = R.jump_case("geometric", n, 3)
    s[:] = s[0]
    D2 = 0.5 * D + 0.125
    h1 = np.array([capi.dividend_jump(s[b], v[b], D[b], K[b]) for b in range(3)])
    h2 = np.array([capi.dividend_jump(s[b], h1[b], D2[b], K[b]) for b in range(3)])
    grid = [float(x) for x in s[0]]
    S0 = grid[n // 2] * 1.001

    def trades(slots):
        rb = readout(slots[0], grid, S0, S0, dg_mode=1)
        ru, rd = readout(slots[1], grid, S0), readout(slots[2], grid, S0)
        rc = readout(slots[2], grid, S0, S0, dg_mode=2, idx=n // 2)
        return [(GK_CNLOG, [rb, ru, rd], (0.3, S0, 0.02, 0.05, 1e-3)),
                (GK_BARRIER, [rb, ru], (0.3, S0, 0.02, 0.01, 0.05, 1e-4)),
                (GK_READOUT, [rc], ())]
    want = [R.trade_f64(k, R.triples(rds, h2), P) for k, rds, P in trades([0, 1, 2])]
    with Session() as S:
        sl = np.concatenate([S.upload(v[b:b + 1]) for b in range(3)])
        j1 = S.dividend_jump(sl, s, D, K)
        j2 = S.dividend_jump(j1, s, D2, K)
        out = S.greeks(trades([int(x) for x in j2]))
        assert same_bits(S.fetch(j2, n), h2)
        assert same_bits(S.fetch(j1, n), h1)
    assert same_bits(out, np.array(want))


def test_dividend_jump_refusals():
    s, v, D, K = R.jump_case("geometric", 4, 2)
    with Session() as S:
        sl = S.upload(v)
        for bad in (s[:, ::-1], np.repeat(s[:, :1], 4, axis=1),
                    np.where(np.arange(4) == 2, s[:, 1:2], s)):
            with pytest.raises(capi.FdcnError, match="strictly increasing"):
                S.dividend_jump(sl, bad, D, K)
        nan = s.copy()
        nan[1, 2] = np.nan
        with pytest.raises(capi.FdcnError, match="strictly increasing"):
            S.dividend_jump(sl, nan, D, K)
        one = S.upload(v[:, :1])
        with pytest.raises(capi.FdcnError, match="n_nodes >= 2"):
            S.dividend_jump(one, s[:, :1], D, K)
        with pytest.raises(capi.FdcnError, match="holds 4 nodes, expected 3"):
            S.dividend_jump(sl, s[:, :3], D, K)
        out = np.empty(2, np.int32)
        args = [np.ascontiguousarray(sl, np.int32).ctypes.data, s.ctypes.data, D.ctypes.data,
                K.ctypes.data, out.ctypes.data]
        for k in range(5):
            a = list(args)
            a[k] = None
            with pytest.raises(capi.FdcnError, match="NULL argument"):
                capi._check(S._L.fdcn_session_dividend_jump(S._h, 2, 4, *a))
        with pytest.raises(capi.FdcnError, match="NULL session"):
            capi._check(S._L.fdcn_session_dividend_jump(None, 2, 4, *args))
        with pytest.raises(capi.FdcnError, match="B >= 0"):
            capi._check(S._L.fdcn_session_dividend_jump(S._h, -1, 4, *args))
        assert S.dividend_jump(sl[:0], s[:0], D[:0], K[:0]).shape == (0,)
        got = S.fetch(S.dividend_jump(sl, s, D, K), 4)  # and the session still answers
    for b in range(2):
        assert same_bits(got[b], capi.dividend_jump(s[b], v[b], D[b], K[b]))
