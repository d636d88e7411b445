"""DiscreteBarrierFDMPricer2: the spot-space CN with
per-row coefficients, FIS non-symmetric barrier rows and the BGK window.

CPU: the facade driven by the C oracle (sequential Thomas on the per-row
plan, oracle_vc_batch) reproduces the reference's own grids, value vectors,
prices and Greeks bit for bit (tests/golden/spot_cases.json, produced by
discrete_barrier_fdm_pricer_2.py itself -- including its wrong-sign explicit
off-diagonals, :383-385, so the values are large; they are still the
reference's values).  With explicit_sign="corrected" the same pricer
converges to Black-Scholes.

GPU: fdcn_vc_batch (csrc/fdcn_vc.hip) against the oracle on the same plans,
max|V - V_oracle| <= 1e-10 max(1, max|V_oracle|) in corrected mode; in the
reference's diverging mode the growth amplifies rounding, so there the
bound is relative to each vector's magnitude, 1e-9.
"""
import datetime as dt
import math

import numpy as np
import pytest

from backends import oracle_engine
from finite_difference_amd.engine import Engine
from vc_cases import (GOLD, V0, _random_rows, _vanilla_solve, _with_exceptional_rows,  # noqa: F401
                      exceptional_positions, factor_scan, make, mixed_forms, split_phase_rows)


@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_spot_pricer_bitwise_reference(case):
    p = make(case["inputs"], oracle_engine())
    assert p.S_nodes == case["S_nodes"]
    assert p.use_bgk_correction == case["use_bgk"]
    assert [p.bgk_lower, p.bgk_upper] == case["bgk"]
    assert [p.k_first_cont, p.k_last_cont] == case["window"]
    assert sorted(p._monitoring_step_map()) == case["monitor_map"]
    Sg, Vg, S_eff = p._solve_grid_once()
    assert Sg == case["S_shifted"] and S_eff == case["S_eff"]
    assert Vg == case["V"]
    assert p.price() == case["price"]
    assert p.greeks() == case["greeks"]


def _bs(S, K, r, sig, T, call):
    d1 = (math.log(S / K) + (r + 0.5 * sig * sig) * T) / (sig * math.sqrt(T))
    d2 = d1 - sig * math.sqrt(T)
    N = lambda x: 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))  # noqa: E731
    if call:
        return S * N(d1) - K * math.exp(-r * T) * N(d2)
    return K * math.exp(-r * T) * N(-d2) - S * N(-d1)


@pytest.mark.parametrize("opt", ["call", "put"])
def test_corrected_sign_converges_to_black_scholes(opt):
    """The reference's grid snaps K onto a node but keeps the uniform dS in
    every row, an O(dS) inconsistency at the strike: convergence is not
    monotone, so the bound is 1% on a fine grid (observed 0.1-0.2%)."""
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type=opt, barrier_type="none",
               flat_rate_nacc=0.05, num_space_nodes=1600, num_time_steps=800)
    p = make(inp, oracle_engine(), explicit_sign="corrected")
    ref = _bs(100.0, 100.0, 0.05, 0.25, p.tenor_years, opt == "call")
    assert abs(p.price() - ref) < 1e-2 * ref, (p.price(), ref)


def test_corrected_knock_out_below_vanilla():
    base = dict(spot=100.0, strike=100.0, volatility=0.25, option_type="call",
                flat_rate_nacc=0.05, num_space_nodes=300, num_time_steps=150)
    van = make(dict(base, barrier_type="none"), oracle_engine(), explicit_sign="corrected")
    weekly = [V0 + dt.timedelta(days=7 * i) for i in range(1, 27)]
    ko = make(dict(base, barrier_type="up-and-out", upper_barrier=130.0,
                   monitoring_dates=[d.isoformat() for d in weekly]), oracle_engine(),
              explicit_sign="corrected")
    assert 0.0 < ko.price() < van.price()


def test_explicit_sign_validated():
    with pytest.raises(ValueError):
        make(GOLD["cases"][0]["inputs"], None, explicit_sign="other")


def _compare_gpu(p, rel):
    Sg, S_eff, solves = p._grid_solves()
    gpu = Engine().run_vc(solves)
    ref = oracle_engine().run_vc(solves)
    for g, r in zip(gpu, ref):
        scale = max(1.0, float(np.max(np.abs(r))))
        err = float(np.max(np.abs(g - r))) / scale
        assert err <= rel, err
    return gpu


@pytest.mark.gpu
@pytest.mark.parametrize("case", GOLD["cases"], ids=lambda c: c["name"])
def test_spot_kernel_vs_oracle_reference_sign(case):
    _compare_gpu(make(case["inputs"], Engine()), 1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,opt,bt", [(200, 100, "call", "none"), (600, 300, "put", "down-and-out"),
                                        (1500, 200, "call", "up-and-out"),
                                        (5000, 60, "call", "double-out")])
def test_spot_kernel_vs_oracle_corrected(n, m, opt, bt):
    weekly = [(V0 + dt.timedelta(days=7 * i)).isoformat() for i in range(1, 27)]
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type=opt, barrier_type=bt,
               lower_barrier=80.0 if "down" in bt or "double" in bt else None,
               upper_barrier=130.0 if "up" in bt or "double" in bt else None,
               monitoring_dates=weekly, flat_rate_nacc=0.05, num_space_nodes=n,
               num_time_steps=m)
    _compare_gpu(make(inp, Engine(), explicit_sign="corrected"), 1e-10)


@pytest.mark.gpu
def test_spot_price_on_gpu_matches_black_scholes():
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type="call", barrier_type="none",
               flat_rate_nacc=0.05, num_space_nodes=1600, num_time_steps=800)
    p = make(inp, Engine(), explicit_sign="corrected")
    ref = _bs(100.0, 100.0, 0.05, 0.25, p.tenor_years, True)
    assert abs(p.price() - ref) < 1e-2 * ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", [257, 513, 1024, 1025, 1026, 2049, 4097, 4098, 8193])
@pytest.mark.parametrize("B", [1, 600])
@pytest.mark.parametrize("bt", ["down-and-out", "up-and-out", "none"])
def test_spot_kernel_grid_one_node_longer_than_the_slots(n, B, bt):
    """N + 1 nodes on N = 64 W NPT slots (1 025 = the reference's 1 024-step
    grid): node 0 stays outside the slots as a scalar (fdcn_vc pad_lo = -1).
    A down-and-out knocks node 0 out on every weekly date, so the scalar's
    projection is covered; an up-and-out and a vanilla keep node 0 at its
    Dirichlet value on every step, on every layout W = 1 / 4 / 8;
    n = slots and slots + 2 keep the padded layout."""
    from finite_difference_amd import capi
    if bt != "down-and-out" and n not in (1025, 4097, 8193):
        pytest.skip("the node-0-outside layouts only")
    weekly = [(V0 + dt.timedelta(days=7 * i)).isoformat() for i in range(1, 27)]
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type="put",
               barrier_type=bt, lower_barrier=80.0 if bt == "down-and-out" else None,
               upper_barrier=125.0 if bt == "up-and-out" else None,
               monitoring_dates=weekly if bt != "none" else [],
               flat_rate_nacc=0.05, num_space_nodes=n - 1, num_time_steps=40)
    p = make(inp, Engine(), explicit_sign="corrected")
    _, _, solves = p._grid_solves()
    sv = solves[0]
    assert sv.n_nodes == n
    if bt == "down-and-out":
        assert sv.ko_lo >= 0 and len(sv.mon_steps) > 0
    elif bt == "up-and-out":
        assert sv.ko_lo < 0 and sv.ko_hi < n and len(sv.mon_steps) > 0
    plan = capi.vc_plan(n, B=B)
    slots = 64 * plan["waves"] * plan["npt"]
    if n in (257, 513, 1025, 2049, 4097, 8193) and B == 600:
        assert slots == n - 1, plan  # the layout under test
    ref = oracle_engine().run_vc([sv])[0]
    gpu = Engine().run_vc([sv] * B)
    scale = max(1.0, float(np.max(np.abs(ref))))
    for g in (gpu[0], gpu[-1]):
        assert float(np.max(np.abs(g - ref))) / scale <= 1e-10
        assert g[0] == ref[0]  # node 0 (the scalar) exactly its Dirichlet / rebate value
    assert all(np.array_equal(g, gpu[0]) for g in gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1025, 600])
def test_spot_dev_entry_skips_repeated_monitor_steps(n):
    """fdcn_vc_batch_dev does not validate the monitor
    runs; a repeated or out-of-order step is skipped (the oracle's `while`)
    instead of stalling every later projection of that scenario."""
    import dataclasses

    import torch
    from finite_difference_amd import capi
    from finite_difference_amd.engine import pack_vc
    from oracle import oracle
    inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type="call",
               barrier_type="double-out", lower_barrier=85.0, upper_barrier=120.0,
               monitoring_dates=[], flat_rate_nacc=0.05, num_space_nodes=n - 1,
               num_time_steps=60)
    p = make(inp, Engine(), explicit_sign="corrected")
    sv = p._grid_solves()[2][0]
    sv.ko_lo, sv.ko_hi = p._ko_nodes(p._grid_solves()[0], 85.0, 120.0)
    runs = [[3, 3, 8, 5, 12, 12, 12, 30, 60], [7, 2, 7, 40, 41, 41, 60]]
    solves = []
    for r in runs:
        solves.append(dataclasses.replace(sv, mon_steps=r,
                                          mon_rebates=[0.25 * (k + 1) for k in range(len(r))]))
    g = pack_vc(solves, [0, 1])
    dev = torch.device("cuda", 0)
    T = {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).to(dev)
         for k in ("diag", "bnd", "v_init", "iparams", "mon_step", "mon_rebate")}
    out = torch.empty_like(T["v_init"])
    wsb = capi.vc_plan(g.n_nodes, B=g.B)["ws_bytes_per_scen"] * g.B
    ws = torch.empty(wsb // 8 + 1, dtype=torch.float64, device=dev)
    capi.vc_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, T["diag"].data_ptr(),
                      T["bnd"].data_ptr(), T["v_init"].data_ptr(), T["iparams"].data_ptr(),
                      len(g.mon_step), T["mon_step"].data_ptr(), T["mon_rebate"].data_ptr(),
                      out.data_ptr(), ws.data_ptr(), wsb, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = oracle.vc_batch(g.n_nodes, g.n_time, g.n_ranna, g.diag, g.bnd, g.v_init, g.iparams,
                          g.mon_step, g.mon_rebate)
    for b in range(2):
        scale = max(1.0, float(np.max(np.abs(ref[b]))))
        assert float(np.max(np.abs(got[b] - ref[b]))) / scale <= 1e-10, b
    # the last projection of each run took effect: knocked-out nodes hold its rebate
    assert got[0][0] == 0.25 * 9 and got[1][-1] == 0.25 * 7


@pytest.mark.gpu
@pytest.mark.parametrize("w,npt,n", [(1, 16, 1025), (1, 8, 513), (1, 4, 257), (4, 16, 4097),
                                     (4, 8, 2049), (16, 4, 4096), (1, 16, 1000), (1, 10, 601),
                                     (1, 10, 641), (1, 12, 769), (1, 12, 700)])
def test_pointwise_exceptional_rows_at_every_slot_position(w, npt, n):
    """The pointwise form's exceptional rows (csrc/fdcn_vc.hip) at slot 0,
    1, NPT-2 and NPT-1 of a lane, across a lane and a wave boundary, next to
    both Dirichlet rows, in the N + 1 layout (node 0 outside the slots) and
    a padded one, every compiled width: one launch of all positions on the
    pinned variant, each scenario classified pointwise (asserted) and equal
    to the oracle; the same launch forced onto the stencil form too."""
    from finite_difference_amd import capi
    pos, solves = exceptional_positions(w, npt, n)
    from finite_difference_amd.engine import pack_vc
    g = pack_vc(solves, list(range(len(solves))))
    assert np.all(capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag) == 1)
    ref = oracle_engine().run_vc(solves)
    try:
        for stencil in (False, True):
            capi.vc_force_variant(w, npt, stencil)
            assert capi.vc_variant_name(n, B=len(solves)) == f"fdcn_vc_march<{w},{npt}>"
            got = Engine().run_vc(solves)
            for i, (a, b) in zip(pos + [-1], zip(got, ref)):
                err = float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
                assert err <= 1e-10, (stencil, i, err)
    finally:
        capi.vc_force_variant(0, 0, False)


@pytest.mark.gpu
def test_mixed_forms_in_one_launch():
    """One launch whose scenarios take different forms: both march kernels
    run, each on the scenarios the factor kernel gave it -- a corrected
    Pricer2 knock-out (pointwise, two exceptional rows), a vanilla
    (pointwise, none), the reference's explicit sign (pointwise, alpha = +1)
    and a scenario with three scattered exceptional rows (stencil)."""
    import dataclasses
    from finite_difference_amd import capi
    from finite_difference_amd.engine import pack_vc
    solves = mixed_forms()
    g = pack_vc(solves, list(range(4)))
    assert capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag).tolist() == [1, 1, 1, 0]
    got = Engine().run_vc(solves)
    ref = oracle_engine().run_vc(solves)
    for k, (a, b) in enumerate(zip(got, ref)):
        scale = max(1.0, float(np.max(np.abs(b))))
        assert float(np.max(np.abs(a - b))) / scale <= (1e-9 if k == 2 else 1e-10), k


def test_vc_forms_classify_the_reference_rows_pointwise():
    """fdcn_vc_forms (the factor kernel's classification, run on the host):
    every reference spot-space case (its own explicit sign, BGK window,
    dividends) and corrected-sign knock-outs take the pointwise form; two
    perturbed adjacent rows still do; three scattered rows, or a perturbed
    Rannacher row far from them, take the stencil form."""
    import dataclasses
    from finite_difference_amd import capi
    from finite_difference_amd.engine import pack_vc

    def forms(solves):
        g = pack_vc(solves, list(range(len(solves))))
        return capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag).tolist()
    for case in GOLD["cases"]:
        _, _, solves = make(case["inputs"], None)._grid_solves()
        assert all(f == 1 for f in forms(solves)), case["name"]
    weekly = [(V0 + dt.timedelta(days=7 * i)).isoformat() for i in range(1, 27)]
    for bt, lo, hi in (("down-and-out", 85.0, None), ("up-and-out", None, 120.0),
                       ("double-out", 80.0, 125.0), ("up-and-in", None, 125.0)):
        inp = dict(spot=100.0, strike=100.0, volatility=0.25, option_type="put", barrier_type=bt,
                   lower_barrier=lo, upper_barrier=hi, monitoring_dates=weekly,
                   flat_rate_nacc=0.05, num_space_nodes=400, num_time_steps=50)
        _, _, solves = make(inp, None, explicit_sign="corrected")._grid_solves()
        assert all(f == 1 for f in forms(solves)), bt
    base = _vanilla_solve(301, 20)
    assert forms([base, _with_exceptional_rows(base, 150)]) == [1, 1]
    D = base.diag.copy()
    for i in (50, 150, 250):
        D[1, 3, i] *= 1.001
    D2 = base.diag.copy()
    D2[1, 3, 40] *= 1.001
    D2[0, 3, 200] = 0.25 * D2[0, 0, 200]  # the Rannacher phase's row 200 as well
    assert forms([dataclasses.replace(base, diag=D), dataclasses.replace(base, diag=D2)]) == [0, 0]
    capi.vc_force_variant(0, 0, True)
    try:
        assert forms([base]) == [0]
    finally:
        capi.vc_force_variant(0, 0, False)


def _serial_pivots(diag_phase):
    """The reference's serial sweep (_solve_tridiagonal,
    discrete_barrier_fdm_pricer_2.py:282-290): pivots beta_i and the
    contraction |sub_i sup_{i-1}| / beta_i^2 of the c* recurrence."""
    sub, m, sup = diag_phase[0], diag_phase[1], diag_phase[2]
    beta = np.empty_like(m)
    c = 0.0
    worst = 0.0
    for i in range(len(m)):
        beta[i] = m[i] - (sub[i] * c if i else 0.0)
        if i:
            worst = max(worst, abs(sub[i] * sup[i - 1]) / beta[i] ** 2)
        c = sup[i] / beta[i]
    return beta, worst


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [-1.0, 1.0], ids=["corrected", "reference_sign"])
@pytest.mark.parametrize("spread", [0.45, 0.65, 0.75])
def test_factor_scan_matches_serial_sweep_on_non_dominant_rows(alpha, spread):
    """fdcn_vc_factor finds the Thomas pivots by a parallel scan
    over 2x2 matrix products, which equals the reference's serial sweep only
    to rounding while the recurrence contracts.  Random implicit rows:
    spread 0.45 all diagonally dominant; 0.65 11 % of rows not dominant,
    the c* recurrence locally expanding (|sub_i sup_(i-1)| / beta_i^2 up to
    2.5), pivots >= 0.4; 0.75 23 % not dominant, pivots down to 0.04 (local
    expansion ~650).  The explicit rows in the reference's sign (alpha = +1)
    and the corrected one; every scenario of the launch against the serial
    oracle, in the pointwise form and forced onto the stencil form."""
    from finite_difference_amd import capi
    from finite_difference_amd.engine import pack_vc
    solves = factor_scan(alpha, spread)
    contraction = []
    for sv in solves:
        for ph in range(2):
            beta, worst = _serial_pivots(sv.diag[ph])
            contraction.append(worst)
            if spread <= 0.65:
                assert np.min(np.abs(beta)) > 0.3
    nondom = np.mean([np.mean(np.abs(sv.diag[1, 0]) + np.abs(sv.diag[1, 2])
                              > np.abs(sv.diag[1, 1])) for sv in solves])
    assert (nondom > 0.05 and max(contraction) > 1.0) if spread > 0.6 else nondom < 0.01
    g = pack_vc(solves, list(range(len(solves))))
    assert np.all(capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag) == 1)
    ref = oracle_engine().run_vc(solves)
    w, npt = (lambda p: (p["waves"], p["npt"]))(capi.vc_plan(1025, B=len(solves)))
    try:
        for stencil in (False, True):
            capi.vc_force_variant(w, npt, stencil)
            got = Engine().run_vc(solves)
            for k, (a, b) in enumerate(zip(got, ref)):
                err = float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
                assert err <= 1e-10, (stencil, k, err)
    finally:
        capi.vc_force_variant(0, 0, False)


@pytest.mark.gpu
@pytest.mark.parametrize("w,npt,n", [(1, 16, 1025), (1, 10, 601), (4, 8, 2049)])
def test_exceptional_rows_split_over_both_phases(w, npt, n):
    """the one-pass path maps each phase's exceptional rows into
    the pair (i1, i1 + 1) (csrc/fdcn_vc.hip, xi[ph][j] - i1).  Here the
    Rannacher phase's only exceptional row is i1 + 1 and the CN phase's is
    i1, so i1 comes from the other phase than the row it pairs with: the
    scenario still classifies pointwise and both forms match the oracle."""
    import dataclasses
    from finite_difference_amd import capi
    from finite_difference_amd.engine import pack_vc
    solves = split_phase_rows(w, npt, n)
    g = pack_vc(solves, list(range(len(solves))))
    assert np.all(capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag) == 1)
    ref = oracle_engine().run_vc(solves)
    try:
        for stencil in (False, True):
            capi.vc_force_variant(w, npt, stencil)
            got = Engine().run_vc(solves)
            for k, (a, b) in enumerate(zip(got, ref)):
                err = float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(b))))
                assert err <= 1e-10, (stencil, k, err)
    finally:
        capi.vc_force_variant(0, 0, False)
