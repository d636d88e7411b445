"""CPU checks of the rounding yardstick for the spot-space per-row march
(march_precision.py on engine.VcGroup, oracle_ext.vc_batch): the REAL-typed
march against the pinned fp64 oracle (bitwise), against __float128 and against
a 50-digit restatement; the leave-one-out condition on every input
test_gpu_vc_precision.py marches (vc_cases.VC_INPUTS); the sequential
restatement of the kernels' ordering against the Thomas march in long double;
and that the bound catches what the fixed 1e-10 tolerance lets through.
"""
import dataclasses

import numpy as np
import pytest

import march_precision as mp
import vc_cases as vc
from finite_difference_amd import capi
from oracle import oracle, oracle_ext

_ys = {}


def _yardstick(key):
    y = _ys.get(key)
    if y is None:
        y = _ys[key] = mp.yardstick(vc.vc_input(key))
    return y


def _oracle(g):
    return oracle.vc_batch(g.n_nodes, g.n_time, g.n_ranna, g.diag, g.bnd, g.v_init, g.iparams,
                           g.mon_step, g.mon_rebate, 4)


def test_inputs_cover_the_groups_and_reseed_is_capped():
    keys = list(vc.VC_INPUTS)
    assert all(k.startswith(vc.GROUPS) for k in keys)
    assert len(vc.keys_of("instances")) == 3 * len(vc.KVC) == 36
    assert len(vc.keys_of("step_shapes")) == len(vc.STEP_VARIANTS) * len(vc.STEP_SHAPES)
    assert len(vc.keys_of("small_grids")) == len(vc.SMALL_N)
    assert len(vc.keys_of("gold")) == len(vc.GOLD["cases"])
    assert len(vc.keys_of("factor_scan")) == 6 and len(vc.keys_of("fuzz")) == 16
    assert len(vc.keys_of("exc_positions")) == len(vc.EXC_POSITIONS)
    assert set(vc.RESEED) <= set(keys)
    assert all(rs > 0 and reason for rs, reason in vc.RESEED.values())
    assert 10 * len(vc.RESEED) <= len(keys), "at most 10 % of the inputs may be re-drawn"
    # the never-run instance is among them, node 0 outside the slots
    g = vc.vc_input("instances_w16n16_plus1")
    assert g.n_nodes == 16385 and g.B == 4 and 40 <= g.n_time <= 70


def test_builds():
    assert oracle_ext.mant_dig("f64") == 53 and oracle_ext.mant_dig("f64fma") == 53
    assert oracle_ext.mant_dig("ld") >= 64


# --------------------------------------------------------------------------
# 1. bit equality with the pinned oracle; the mirrored plan
# --------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(vc.VC_INPUTS))
def test_f64_build_is_the_oracle_bit_for_bit(key):
    y = _yardstick(key)
    ref = _oracle(y.g)
    hi, lo = mp.march("f64", y.g)
    assert np.array_equal(hi.view(np.int64), ref.view(np.int64))
    assert not lo.any()
    # the mirrored plan, mirrored back: the Dirichlet rows carry no arithmetic
    # of the solve beyond the division by their own diagonal
    m = y.real["mirror"]
    assert np.array_equal(m[:, [0, -1]], ref[:, [0, -1]])


def test_mirror_is_an_involution():
    g = vc.vc_input("step_shapes_w1n16_65r2")
    gg = mp.mirror_group(mp.mirror_group(g))
    for f in ("diag", "bnd", "iparams", "v_init", "mon_step", "mon_rebate"):
        assert np.array_equal(getattr(gg, f), getattr(g, f)), f
    m = mp.mirror_group(g)
    assert np.array_equal(m.diag[:, :, 0], g.diag[:, :, 2, ::-1])   # sub <- sup, reversed
    assert np.array_equal(m.diag[:, :, 3], g.diag[:, :, 5, ::-1])   # a <- c
    assert np.array_equal(m.bnd[:, :, 0], g.bnd[:, :, 1])
    # an honest reordering: not the same bits as the literal march
    assert not np.array_equal(mp.realise("mirror", g), mp.realise("f64", g))


def test_series_cut_term_is_zero_for_vc_groups():
    y = _yardstick("small_grids_64")
    _, NT = y.noise()
    _, b_tail = y.bounds()
    assert np.array_equal(b_tail, mp.FACTOR * np.maximum(NT, 2.0 * mp.U * mp.TAIL_REL * y.vmax))


# --------------------------------------------------------------------------
# 2. long double against __float128 and against 50 digits
# --------------------------------------------------------------------------
QUAD_KEYS = ["long_march", "instances_w16n16_plus1", "factor_scan_a+1_s0.75",
             "step_shapes_w4n8_129r64", "small_grids_5", "gold_put_di_divs"]


@pytest.mark.parametrize("key", QUAD_KEYS)
def test_long_double_against_quad(key):
    """The reference's own error, measured in __float128, is at most 2^-9 of
    the fp64 noise N it is used to measure (direct and mirrored marches)."""
    if not oracle_ext.quad_available():
        pytest.skip("no libquadmath: liboracle_ext_quad.so cannot be built")
    y = _yardstick(key)
    qh, ql = mp.march("quad", y.g)
    N, _ = y.noise()
    for name, (h, l) in (("direct", (y.hi, y.lo)), ("mirrored", mp.march_mirrored("ld", y.g))):
        e = np.max(np.abs((h - qh) + (l - ql)), axis=1)
        print(f"[quad {key} {name}] ld error {e / (mp.U * y.vmax)} u, N {N / (mp.U * y.vmax)} u")
        assert np.all(e <= 2.0 ** -9 * N), (name, e, N)


def _mp_march(g, b):
    """vc_solve_one (oracle/fdcn_oracle.c) at 50 digits."""
    import mpmath
    mpf = mpmath.mpf
    n = g.n_nodes
    D = [[[mpf(float(x)) for x in g.diag[b, ph, k]] for k in range(6)] for ph in range(2)]
    V = [mpf(float(x)) for x in g.v_init[b]]
    I = [int(x) for x in g.iparams[b]]
    pos, end = I[capi.I_MON_START], I[capi.I_MON_START] + I[capi.I_MON_COUNT]
    for m in range(g.n_time):
        sub, mn, sup, ae, be, ce = D[0 if m < g.n_ranna else 1]
        rhs = [mpf(float(g.bnd[b, m, 0]))] + [ae[i] * V[i - 1] + be[i] * V[i] + ce[i] * V[i + 1]
                                              for i in range(1, n - 1)] + [mpf(float(g.bnd[b, m, 1]))]
        cs, ds = [sup[0] / mn[0]], [rhs[0] / mn[0]]
        for i in range(1, n):
            beta = mn[i] - sub[i] * cs[i - 1]
            cs.append(sup[i] / beta)
            ds.append((rhs[i] - sub[i] * ds[i - 1]) / beta)
        x = [mpf(0)] * n
        x[n - 1] = ds[n - 1]
        for i in range(n - 2, -1, -1):
            x[i] = ds[i] - cs[i] * x[i + 1]
        V = x
        if pos < end and int(g.mon_step[pos]) == m + 1:
            V = [mpf(float(g.mon_rebate[pos])) if j <= I[capi.I_KO_LO] or j >= I[capi.I_KO_HI]
                 else V[j] for j in range(n)]
            pos += 1
        while pos < end and int(g.mon_step[pos]) <= m + 1:
            pos += 1
    return V


def test_long_double_against_mpmath():
    """33 nodes x 20 steps: random rows in both explicit signs, an exceptional
    pair, a knock-out of both ends on three steps."""
    mpmath = pytest.importorskip("mpmath")
    g = vc.small_grids(33, m=20)
    assert (g.n_nodes, g.n_time) == (33, 20)
    hi, lo = mp.march("ld", g)
    with mpmath.workdps(50):
        for b in range(g.B):
            ref = _mp_march(g, b)
            vmax = max(abs(v) for v in ref)
            err = max(abs((mpmath.mpf(float(hi[b, j])) + mpmath.mpf(float(lo[b, j]))) - ref[j])
                      for j in range(g.n_nodes))
            assert err <= mpmath.mpf(2) ** -60 * vmax, (b, float(err / vmax))


# --------------------------------------------------------------------------
# 3. leave-one-out: each fp64 realisation against the bounds built from the other two
# --------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(vc.VC_INPUTS))
def test_leave_one_out(key):
    """The cap that keeps the factor 8 honest: on every input of the GPU file,
    each realisation passes both bounds built from the other two.  An input
    that fails is re-drawn (vc_cases.RESEED, capped at 10 %), never the factor."""
    y = _yardstick(key)
    for name in mp.REALISATIONS:
        y.check(y.real[name], f"{key} leave out {name}", exclude=name)


@pytest.mark.parametrize("key", sorted(vc.RESEED))
def test_reseeded_inputs_did_fail(key):
    """RESEED lists only inputs whose first draw does fail leave-one-out."""
    y = mp.yardstick(vc.vc_input(key, 0))
    worst = max(float(np.max(r)) for name in mp.REALISATIONS
                for r in y.ratios(y.real[name], exclude=name))
    assert worst > 1.0, worst


# --------------------------------------------------------------------------
# the kernels' ordering, restated sequentially, is the same solve
# --------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["long_march", "instances_w16n16_plus1", "instances_w1n10_ragged",
                                 "factor_scan_a-1_s0.75", "factor_scan_a+1_s0.65", "mixed_forms",
                                 "step_shapes_w4n8_129r64", "step_shapes_w1n16_20r20",
                                 "small_grids_3", "small_grids_65", "exc_positions_w1n12_700",
                                 "split_phases_w1n10_601", "gold_put_do_weekly", "fuzz_10"])
def test_kernel_order_is_the_same_solve_in_long_double(key):
    """Scaled factored rows with g folded into the explicit rows (stencil
    form) and u = x - alpha V with residual rows and shifted carry-ins
    (pointwise form), both without scans, are the Thomas march in exact
    arithmetic: in long double they agree with it to 2^-6 of the fp64 floor
    max(N, 2u vmax), so what their fp64 builds show is rounding."""
    y = _yardstick(key)
    N, _ = y.noise()
    floor = np.maximum(N, 2.0 * mp.U * y.vmax)
    for order in (oracle_ext.VC_KERNEL_STENCIL, oracle_ext.VC_KERNEL_POINTWISE):
        h, l = mp.march("ld", y.g, order)
        e = np.max(np.abs((h - y.hi) + (l - y.lo)), axis=1)
        print(f"[{key} order {order}] worst |ld restatement - ld| / floor = {np.max(e / floor):.2e}")
        assert np.all(e <= 2.0 ** -6 * floor), (order, float(np.max(e / floor)))


def test_kernel_order_leaves_the_sequential_spread_on_fuzz_10():
    """The finding behind vc_cases.KERNEL_ORDER_GROUPS, without a GPU: on
    fuzz_10 the sequential restatement of the pointwise form (x = alpha V + u
    on once-rounded scaled rows) is itself outside the tail bound of the three
    Thomas orderings, at the edge of the tail set, by the amount the pointwise
    kernel was measured at on an MI355X (0.029 u vmax) to within a factor 1.5,
    and the error grows with the step count.  The max-norm bound and the
    fixed 1e-10 see nothing."""
    g = vc.vc_input("fuzz_10")
    y = _yardstick("fuzz_10")
    uv = mp.U * y.vmax[0]

    def tail_err(gg, yy):
        e = yy.err(mp.realise(mp.KERNEL_POINTWISE, gg))
        return float(np.max(np.where(yy.tail, e, 0.0))) / (mp.U * yy.vmax[0])
    ko = mp.realise(mp.KERNEL_POINTWISE, g)
    r_max, r_tail = y.ratios(ko)
    err_u = tail_err(g, y)
    print(f"[fuzz_10] pointwise order: tail {err_u:.4f}u (MI355X 0.029u), ratios {r_max[0]:.2f} "
          f"{r_tail[0]:.2f}, max-norm {np.max(y.err(ko)) / uv:.0f}u")
    assert r_tail[0] > 1.0 and r_max[0] < 1.0
    assert 0.029 / 1.5 <= err_u <= 0.029 * 1.5
    assert mp.old_bound_ok(ko[0], y.real["f64"][0])
    short = dataclasses.replace(g, n_time=20, bnd=np.ascontiguousarray(g.bnd[:, :20]))
    assert tail_err(short, mp.yardstick(short)) < 0.25 * err_u
    y4 = mp.yardstick(g, mp.REALISATIONS + (mp.KERNEL_POINTWISE,))
    assert y4.ratios(ko)[1][0] <= 1.0 / mp.FACTOR + 1e-12


def test_kernel_order_groups_are_never_in_leave_one_out():
    assert vc.KERNEL_ORDER_GROUPS == ("fuzz_",)
    assert not set(mp.REALISATIONS) & {mp.KERNEL_STENCIL, mp.KERNEL_POINTWISE, mp.KERNEL_ORDER}
    assert vc.uses_kernel_order("fuzz_3") and not vc.uses_kernel_order("long_march")


# --------------------------------------------------------------------------
# 4. the bound catches what it should (and the fixed tolerance does not)
# --------------------------------------------------------------------------
def _knock_out_trade(opt, bt, lo, hi, n=257, m=60):
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type=opt, barrier_type=bt,
               lower_barrier=lo, upper_barrier=hi, monitoring_dates=vc.WEEKLY,
               flat_rate_nacc=0.05, num_space_nodes=n - 1, num_time_steps=m)
    return vc.make(inp, None, explicit_sign="corrected")._grid_solves()[2][0]


def _exceptional(sv, ph):
    """alpha of the phase's middle row and its exceptional rows."""
    D, n = sv.diag[ph], sv.n_nodes
    alpha = D[3, n // 2] / D[0, n // 2]
    exc = np.flatnonzero(((D[3] - alpha * D[0]) != 0.0) | ((D[5] - alpha * D[2]) != 0.0))
    return alpha, [int(i) for i in exc if 0 < i < n - 1]


def test_smooth_relative_bump_fails():
    """A relative error of 1e-12 with a smooth profile over the grid (what a
    once-rounded constant does) on every small grid: far inside the fixed
    tolerance, outside the yardstick."""
    for key in vc.keys_of("small_grids") + ["instances_w1n4_fit"]:
        y = _yardstick(key)
        ref = y.real["f64"]
        n = y.g.n_nodes
        V = ref * (1.0 + 1e-12 * np.sin(np.pi * (np.arange(n) + 0.5) / n))
        r_max, _ = y.ratios(V)
        assert np.all(r_max > 1.0), (key, r_max)
        assert all(mp.old_bound_ok(V[b], ref[b]) for b in range(y.g.B))
        y.check(ref, f"{key} unperturbed")


def _py_march(g, b, pivot_row=None, pivot_rel=0.0):
    """vc_solve_one in Python floats (bitwise the f64 build), with the pivot
    beta of one row scaled by (1 + pivot_rel) on every step."""
    n = g.n_nodes
    V = [float(x) for x in g.v_init[b]]
    I = [int(x) for x in g.iparams[b]]
    pos, end = I[capi.I_MON_START], I[capi.I_MON_START] + I[capi.I_MON_COUNT]
    for m in range(g.n_time):
        sub, mn, sup, ae, be, ce = (g.diag[b, 0 if m < g.n_ranna else 1, k].tolist()
                                    for k in range(6))
        rhs = [float(g.bnd[b, m, 0])] + [ae[i] * V[i - 1] + be[i] * V[i] + ce[i] * V[i + 1]
                                         for i in range(1, n - 1)] + [float(g.bnd[b, m, 1])]
        cs, ds = [sup[0] / mn[0]], [rhs[0] / mn[0]]
        for i in range(1, n):
            beta = mn[i] - sub[i] * cs[i - 1]
            if i == pivot_row:
                beta *= 1.0 + pivot_rel
            cs.append(sup[i] / beta if i < n - 1 else 0.0)
            ds.append((rhs[i] - sub[i] * ds[i - 1]) / beta)
        x = [0.0] * n
        x[n - 1] = ds[n - 1]
        for i in range(n - 2, -1, -1):
            x[i] = ds[i] - cs[i] * x[i + 1]
        V = x
        if pos < end and int(g.mon_step[pos]) == m + 1:
            reb = float(g.mon_rebate[pos])
            V = [reb if j <= I[capi.I_KO_LO] or j >= I[capi.I_KO_HI] else V[j] for j in range(n)]
            pos += 1
        while pos < end and int(g.mon_step[pos]) <= m + 1:
            pos += 1
    return np.asarray(V)


def test_one_perturbed_pivot_fails():
    """One pivot of the factorisation 2^-40 off (what a factor scan that lost
    13 bits on one row would store): outside the yardstick, inside 1e-10."""
    key = "instances_w1n4_plus1"  # 257 nodes, the four trades
    y = _yardstick(key)
    g, ref = y.g, y.real["f64"]
    for b in range(g.B):
        assert np.array_equal(_py_march(g, b), ref[b])  # the restatement is the f64 march
        j = np.arange(g.n_nodes)
        alive = (j > max(0, g.iparams[b, capi.I_KO_LO])) & \
            (j < min(g.n_nodes - 1, g.iparams[b, capi.I_KO_HI]))
        row = int(np.argmax(np.where(alive, np.abs(y.hi[b]), -1.0)))  # the largest live value
        V = _py_march(g, b, row, 2.0 ** -40)
        r_max, _ = y.ratios(np.where(np.arange(g.B)[:, None] == b, V[None, :], ref))
        print(f"[{key} solve {b}] pivot {row} off by 2^-40: ratio {r_max[b]:.1f}")
        assert r_max[b] > 1.0, (b, row, r_max[b])
        assert mp.old_bound_ok(V, ref[b])


DROPPED = [("call", "down-and-out", 80.0, None, 1, 5),   # rc of the second row: the tail bound
           ("put", "up-and-out", None, 300.0, 1, 3)]     # ra of the second row: the max-norm


@pytest.mark.parametrize("opt,bt,lo,hi,which,col", DROPPED, ids=["second_rc", "second_ra"])
def test_dropped_exceptional_residual_fails(opt, bt, lo, hi, which, col):
    """A knock-out trade marched with one residual coefficient of its
    barrier rows dropped (the explicit entry set to alpha times the implicit
    one, as on a uniform row): both cases pass 1e-10 max(1, vmax)."""
    sv = _knock_out_trade(opt, bt, lo, hi)
    D = sv.diag.copy()
    for ph in range(2):
        alpha, exc = _exceptional(sv, ph)
        if ph == 0 and not exc:
            continue  # theta = 1: the explicit off-diagonals are all zero, alpha = 0
        assert len(exc) == 2 and exc[1] == exc[0] + 1, exc
        assert D[ph, col, exc[which]] != alpha * D[ph, col - 3, exc[which]]
        D[ph, col, exc[which]] = alpha * D[ph, col - 3, exc[which]]
    y = mp.yardstick(vc._group([sv]))
    V = mp.march("f64", vc._group([dataclasses.replace(sv, diag=D)]))[0]
    r_max, r_tail = y.ratios(V)
    print(f"[{bt} residual dropped] ratio_max={r_max[0]:.3g} ratio_tail={r_tail[0]:.3g}")
    assert max(r_max[0], r_tail[0]) > 1.0
    assert mp.old_bound_ok(V[0], y.real["f64"][0])
    y.check(y.real["f64fma"], f"{bt} unperturbed")
