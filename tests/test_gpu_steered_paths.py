"""The two Monte Carlo path kernels (bgk_path_kernel in csrc/fdcn_mc_bgk.hip,
mc_path_kernel in csrc/fdcn_mc.hip) on steered paths: normals solved for so
that spots land in the smoothed bands, on their edges, next to the exact-mode
levels, on the spot floor and on either side of a threshold across a dividend
(tests/steered_paths.py; the reference's per-path values on them recorded by
tests/golden/make_golden_steered.py).  Every launch is a few hundred paths of
seven or eight steps with valid arguments."""
import dataclasses

import numpy as np
import pytest

import bgk_fixture
import mc_fixture
import steered_paths as sp
from finite_difference_amd import bgk_barrier, capi, mc_barrier
from finite_difference_amd.bgk_barrier import DiscreteBarrierBGKPricer, run_paths

pytestmark = pytest.mark.gpu

CASES = sp.load_cases()
ARRAYS = sp.load_arrays()
TRADES = CASES["bgk"]["trades"]
MC_CASES = CASES["mc"]["cases"]


def _pricer(trade):
    return DiscreteBarrierBGKPricer(engine="hip", **bgk_fixture.kwargs_for(trade["inputs"]))


def _trade(name):
    return next(t for t in TRADES if t["name"] == name)


def _both_signs(plan, z):
    return np.concatenate([z, -z], axis=0) if plan.antithetic else z


def _bitwise(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def _labels(trade, plan):
    labels = CASES["bgk"]["labels"][trade["menu"]]
    return labels + ["mirror of " + lb for lb in labels] if plan.antithetic else labels


def _bounds(plan, zf, x_ref):
    """bgk_fixture.path_bounds; with a rebate at expiry x carries the term
    R * (1 - alive) as well, whose error is path_bounds' rebate bound (R times
    the movement of alive), so the two add."""
    bound_x, bound_r = bgk_fixture.path_bounds(plan, zf, x_ref)
    if plan.rebate_mode == 1 and plan.params[capi.BGK_P_EPS_BARRIER] > 0.0:
        bound_x = bound_x + bound_r
    return bound_x, bound_r


def _contract(case):
    return mc_barrier.plan_contract(**mc_fixture.kwargs_for(case["inputs"], mc_barrier))


# ---------------------------------------------------------------------------
# BGK: per-path values against the reference's
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("trade", TRADES, ids=lambda t: t["name"])
def test_bgk_values_on_steered_paths(trade):
    """Per path |gpu - ref| <= bgk_fixture.path_bounds: on the ramps the steep
    n_mon * intrinsic / (2 eps_b) term is what a 1-ulp spot difference needs.
    In exact mode (eps_b = 0) the decisions are equal: rebate_pv is exact."""
    plan = _pricer(trade)._job().plan
    z = ARRAYS[trade["normals"]]
    zf = _both_signs(plan, z)
    x_ref = ARRAYS["x_" + trade["name"]]
    r_ref = ARRAYS.get("rebate_" + trade["name"], np.zeros_like(x_ref))
    bound_x, bound_r = _bounds(plan, zf, x_ref)
    stats, pay = run_paths([[plan]], engine="hip", z=z, want_payoffs=True)
    assert pay.shape == (1, 1, 2, trade["n_sim"])
    err_x = np.abs(pay[0, 0, 0] - x_ref)
    err_r = np.abs(pay[0, 0, 1] - r_ref)
    labels = _labels(trade, plan)
    for group in sorted({sp.group_of(lb) for lb in labels}):
        rows = [i for i, lb in enumerate(labels) if sp.group_of(lb) == group]
        ratio_r = np.max(err_r[rows] / np.where(bound_r[rows] > 0.0, bound_r[rows], np.inf))
        print(f"{trade['name']} {group}: worst x error / bound "
              f"{np.max(err_x[rows] / bound_x[rows]):.2e}, rebate_pv {ratio_r:.2e}")
    assert np.all(err_x <= bound_x), labels[int(np.argmax(err_x / bound_x))]
    assert np.all(err_r <= bound_r), labels[int(np.argmax(err_r - bound_r))]
    # the four raw sums are those of the per-path values
    x, r = pay[0, 0, 0], pay[0, 0, 1]
    assert abs(stats[0, 0, 0] - np.sum(x)) <= 1e-12 * np.sum(np.abs(x))
    assert abs(stats[0, 0, 1] - np.sum(x * x)) <= 1e-12 * np.sum(x * x)
    assert abs(stats[0, 0, 2] - np.sum(r)) <= 1e-12 * np.sum(np.abs(r)) + 1e-300
    # sum (1 - alive): alive moves by at most n_mon breach amounts, each by a
    # spot's 4 * 2^-51 * S_max over the ramp's width 2 eps_b; exact for eps_b = 0
    _, _, alive = bgk_barrier.host_paths(plan, zf)
    eps_b = float(plan.params[capi.BGK_P_EPS_BARRIER])
    tol = 0.0
    if eps_b > 0.0:
        spots = sp.landing(plan.params[0], plan.step[:, 0], plan.step[:, 1], zf)
        n_mon = int(np.count_nonzero(plan.step[:, capi.BGK_S_MONITOR]))
        tol = float(np.sum(4.0 * 2.0 ** -51 * spots.max(axis=1) * n_mon / (2.0 * eps_b)))
    assert abs(stats[0, 0, 3] - np.sum(1.0 - alive)) <= tol + 1e-12 * np.sum(1.0 - alive)


# ---------------------------------------------------------------------------
# BGK: grouping and batching on paths that take the ramps (bitwise)
# ---------------------------------------------------------------------------
def test_bgk_grouping_on_steered_paths():
    """The base scenario alone, as slot 0 of its Greeks ladder and as slot 7
    of a G = 8 group: per-path values and the four sums bit for bit.  The
    bumped scenarios (spots 0.023 off the base's: outside the bands) against
    the host engine."""
    trade = _trade("dbl_call_smooth_hit")
    p = _pricer(trade)
    up, dn, base, upv, dnv = (j.plan for j in p._bumped_jobs(1e-4 * p.spot_price, 1e-4))
    z = ARRAYS[trade["normals"]]
    kw = dict(engine="hip", z=z, want_payoffs=True)
    alone = run_paths([[base]], **kw)
    ladder = run_paths([[base, up, dn, upv, dnv]], **kw)
    eight = run_paths([[up, dn, upv, dnv, up, dn, upv, base]], **kw)
    assert _bitwise(alone[0][0, 0], ladder[0][0, 0]) and _bitwise(alone[1][0, 0], ladder[1][0, 0])
    assert _bitwise(alone[0][0, 0], eight[0][0, 7]) and _bitwise(alone[1][0, 0], eight[1][0, 7])
    assert _bitwise(ladder[1][0, 1], eight[1][0, 0])
    assert np.array_equal(alone[1][0, 0, 0], run_paths([[base]], **kw)[1][0, 0, 0])
    zf = _both_signs(base, z)
    for g, plan in enumerate((base, up, dn, upv, dnv)):
        x, rebate, _ = bgk_barrier.host_paths(plan, zf)
        bound_x, bound_r = _bounds(plan, zf, x)
        err_x = np.abs(ladder[1][0, g, 0] - x)
        err_r = np.abs(ladder[1][0, g, 1] - rebate)
        print(f"ladder slot {g}: worst x error / bound {np.max(err_x / bound_x):.2e}, "
              f"rebate_pv {np.max(err_r / bound_r):.2e}")
        assert np.all(err_x <= bound_x) and np.all(err_r <= bound_r), g
    assert len({tuple(ladder[0][0, g]) for g in range(5)}) == 5


@pytest.mark.parametrize("antithetic", [True, False])
def test_bgk_batch_on_steered_paths(antithetic):
    """The 18 smoothed out-trades (sides x rebate modes x call / put) share one
    set of normals: as one launch of B = 18 each gives bit for bit what it
    gives alone."""
    trades = [t for t in TRADES if t["menu"] == "smooth" and "_in_" not in t["name"]]
    assert len(trades) == 18
    plans = [dataclasses.replace(_pricer(t)._job().plan, antithetic=antithetic) for t in trades]
    assert len({(int(p.flags[0]), int(p.flags[1]), int(p.flags[2])) for p in plans}) == 18
    z = ARRAYS[trades[0]["normals"]]
    assert all(t["normals"] == trades[0]["normals"] for t in trades)
    kw = dict(engine="hip", z=z, n_obs=z.shape[0], want_payoffs=True)
    stats, pay = run_paths([[p] for p in plans], **kw)
    for b, plan in enumerate(plans):
        one_stats, one_pay = run_paths([[plan]], **kw)
        assert _bitwise(one_stats[0], stats[b]) and _bitwise(one_pay[0], pay[b]), trades[b]["name"]
    assert len({tuple(stats[b, 0]) for b in range(18)}) >= 12


# ---------------------------------------------------------------------------
# single barrier
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", MC_CASES, ids=lambda c: c["name"])
def test_single_barrier_payoffs_on_steered_paths(case):
    """|gpu - ref| <= 1e-11 |ref| + 1e-12 spot per observation, the bound of
    test_gpu_mc.test_payoff_parity_on_the_references_normals.  A decision that
    differed would move a payoff by far more (a vanilla against a rebate, one
    hit date's discount factor against another's, a clamped spot against an
    unclamped one): within the bound every decision is the reference's."""
    c = _contract(case)
    z = ARRAYS[case["normals"]]
    anti = case["inputs"]["cfg"]["antithetic"]
    sums, pay = mc_barrier.simulate([c], z.shape[0], anti, engine="hip", z=z, want_payoffs=True)
    ref = ARRAYS[case["payoffs"]]
    spot = case["inputs"]["spot"]
    err = np.abs(pay[0] - ref)
    bound = 1e-11 * np.abs(ref) + 1e-12 * spot
    for group in sorted({sp.group_of(lb) for lb in case["labels"]}):
        rows = [i for i, lb in enumerate(case["labels"]) if sp.group_of(lb) == group]
        print(f"{case['name']} {group}: worst payoff error / bound "
              f"{np.max(err[rows] / bound[rows]):.2e}")
    assert np.all(err <= bound), case["labels"][int(np.argmax(err / bound))]
    assert abs(sums[0, 0] - np.sum(pay[0])) <= 1e-12 * np.sum(np.abs(pay[0])) + 1e-300


@pytest.mark.parametrize("name", ["do_call_floor_div_first", "do_call_floor_div_last",
                                  "ui_call_straddle_div_first", "di_call_straddle_div_last"])
def test_single_barrier_antithetic_launch_of_the_same_normals(name):
    """The floor and jump-order rows once more with their mirrored paths,
    against the host engine (the mirrors are off the decision edges too)."""
    case = next(c for c in MC_CASES if c["name"] == name)
    assert not case["inputs"]["cfg"]["antithetic"]
    c = _contract(case)
    z = ARRAYS[case["normals"]]
    assert sp.mc_edge_gap(c, np.concatenate([z, -z])) > sp.EDGE
    want = mc_barrier._host_observations(c, z, True)
    _, pay = mc_barrier.simulate([c], z.shape[0], True, engine="hip", z=z, want_payoffs=True)
    err = np.abs(pay[0] - want)
    bound = 1e-11 * np.abs(want) + 1e-12 * case["inputs"]["spot"]
    print(f"{name} antithetic: worst payoff error / bound {np.max(err / bound):.2e}")
    assert np.all(err <= bound)
