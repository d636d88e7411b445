"""The least-squares Monte Carlo contract (include/fdcn.h) against its mpmath
restatement (lsm_reference.py) at the decision edges of lsm_edge_cases.py, on
the CPU: the reference against facts that owe nothing to this project, the
branch census and the margin conditions of the fixture
(golden/make_golden_lsm_edges.py), an exact regeneration of two small cases,
and the NumPy host engine against every case under the derived bounds of
DESIGN.md 13.1.  The device runs the same comparison in test_gpu_lsm_edges.py.
"""
import math

import mpmath as mp
import numpy as np
import pytest

import lsm_edge_cases as ec
import lsm_reference as lr
from conftest import GOLDEN, load_golden
from finite_difference_amd import capi, mc_american

FIX = load_golden("lsm_edges.json")
ARRAYS = dict(np.load(GOLDEN + "/lsm_edges.npz"))
CASES = FIX["cases"]
N = capi.LSM_SUBRUN


def stored(name):
    return ec.load_case(name, CASES[name], ARRAYS)


def floats(v):
    return np.array([float(x) for x in v])


# ---------------------------------------------------------------------------
# 1. the reference against facts that owe nothing to this project
# ---------------------------------------------------------------------------
def test_the_menu_and_the_fixture_name_the_same_cases():
    assert sorted(CASES) == sorted(ec.MENU)


def test_one_step_is_the_discounted_mean_payoff():
    c = ec.contract("none", "call", times=[0.5], strike=95.0)
    r = lr.reference_subrun(c, 0, False, 5, 9)
    z = lr.subrun_normals(1, False, 5, 2 * 9 + 1, 0)[:, 0]
    s = 100.0 * np.exp((0.03 - 0.045) * 0.5 + 0.3 * math.sqrt(0.5) * z)
    want = float(np.mean(np.maximum(s - 95.0, 0.0)) * math.exp(-0.05 * 0.5))
    assert float(r["price_mean"]) == pytest.approx(want, rel=1e-13)
    assert r["invalid"] == 0 and mp.isinf(r["min_margin"])


def test_the_path_to_observation_mapping():
    """Antithetic: slots 2 j and 2 j + 1 of a thread are +z and -z of one
    observation; sub-run g continues the stream of sub-run g - 1."""
    z = lr.subrun_normals(3, True, 7, 4, 0)
    assert np.array_equal(z[0:256], -z[256:512]) and np.array_equal(z[3584:3840], -z[3840:])
    assert not np.array_equal(np.abs(z[0:256]), np.abs(z[512:768]))
    both = mc_american.philox_normals(4096, 3, 7, 4, 0)
    assert np.array_equal(z[512:768], both[256:512])
    nxt = lr.subrun_normals(3, True, 7, 4, 2048)
    assert np.array_equal(nxt[0:256], both[2048:2304])
    plain = lr.subrun_normals(3, False, 7, 4, 4096)
    assert np.array_equal(plain, mc_american.philox_normals(4096, 3, 7, 4, 4096))


def test_european_knock_in_plus_knock_out_is_vanilla_path_by_path():
    """Zero rebate, no exercise date, and a barrier on the out-of-the-money
    side: the contract's knock-out pays max(phi, rebate) at the hit (the FD
    pricers' exercise floor), which is zero only where the breach is out of
    the money."""
    t = [0.1, 0.3, 0.5]
    kw = dict(times=t, monitor=(0, 1, 2), exercise=(), upper=106.0)
    parts = [lr.reference_subrun(ec.contract(k, "put", **kw), 0, True, 3, 2)
             for k in ("up-and-in", "up-and-out", "none")]
    ki, ko, va = (p["values"] for p in parts)
    with mp.workdps(lr.DPS):
        assert max(abs(a + b - v) for a, b, v in zip(ki, ko, va)) < mp.mpf("1e-45")
        assert abs(parts[0]["fit_mean"] + parts[1]["fit_mean"] - parts[2]["fit_mean"]) < 1e-45
    assert sum(1 for v in ki if v > 0) > 100 and sum(1 for v in ko if v > 0) > 100


def test_an_unreachable_double_knock_out_is_kind_none():
    t = [0.2, 0.35, 0.5]
    a = lr.reference_subrun(ec.contract("double-out", "put", times=t, monitor=(0, 1, 2),
                                        lower=1e-3, upper=1e6, rebate=3.0), 0, False, 4, 1)
    b = lr.reference_subrun(ec.contract("none", "put", times=t), 0, False, 4, 1)
    assert a["values"] == b["values"] and a["coef"] == b["coef"] and a["stops"] == b["stops"]
    assert a["valid"] == [True, True, False]


def test_the_fit_agrees_with_lstsq_on_the_centred_design():
    """One fit by another route: numpy's SVD least squares on the float64
    design centred at the mean regressor, against the reference's normal
    equations; lstsq's own accuracy is eps * cond of that design."""
    c = ec.contract("none", "put")
    r = lr.reference_subrun(c, 0, False, 6, 3)
    m = 5
    u = floats(r["fit_u"][m])
    y = floats(r["fit_cf"][m])
    mu = float(u.mean())
    V = np.vander(u - mu, 4, increasing=True)
    sol, _, rank, sv = np.linalg.lstsq(V, y, rcond=None)
    assert rank == 4
    with mp.workdps(lr.DPS):
        want = floats(lr.cubic(r["coef"][m - 1], mp.mpf(float(v))) for v in u)
    got = V @ sol
    tol = 100.0 * ec.EPS * (sv[0] / sv[-1]) * np.max(np.abs(y))
    assert np.max(np.abs(got - want)) <= tol
    assert tol < 1e-9


# ---------------------------------------------------------------------------
# 2. the census and the conditions on the fixture
# ---------------------------------------------------------------------------
def test_every_branch_of_the_contract_is_taken():
    """Each path branch by at least 16 paths of one set of one sub-run of one
    case; each step branch by at least one step."""
    best = {k: 0 for k in lr.CENSUS_PATH_KEYS + lr.CENSUS_STEP_KEYS}
    for doc in CASES.values():
        for item in doc["items"]:
            for run in item["runs"]:
                for k, v in run["census"].items():
                    best[k] = max(best[k], max(v) if isinstance(v, list) else v)
    print(best)
    for k in lr.CENSUS_PATH_KEYS:
        assert best[k] >= 16, (k, best[k])
    for k in lr.CENSUS_STEP_KEYS:
        assert best[k] >= 1, k
    assert best == FIX["census_max"]


def test_margins_and_exclusion_caps():
    """Every decision of the reference is at least 100 bounds from its fit, or
    the case leaves out at most 1 % of its decisions; the excluded price paths
    are stored."""
    assert FIX["margin_factor"] == ec.MARGIN_FACTOR and FIX["exclusion_cap"] == ec.EXCLUSION_CAP
    for name, doc in CASES.items():
        for item, st in zip(doc["items"], stored(name)):
            assert 0 <= item["stream_id"] < ec.MAX_STREAM
            assert item["n_low_margin"] <= ec.EXCLUSION_CAP * max(1, item["n_decisions"]), name
            if item["n_low_margin"] == 0:
                assert item["n_decisions"] == 0 or item["worst_margin_ratio"] >= ec.MARGIN_FACTOR
                assert not any(r.excluded.any() for r in st.runs), name
            assert sum(int(r.excluded.sum()) for r in st.runs) <= item["n_low_margin"]


def test_the_steered_counts_and_pivots():
    for name in ("minfit_put", "minfit_put_anti", "minfit_call", "minfit_call_anti",
                 "minfit_knock_in", "minfit_knock_out"):
        a, b = (it["runs"][0] for it in CASES[name]["items"])
        k = ec.EDGE_STEP - 1
        assert (a["count"][k], a["valid"][k]) == (64, True), name
        assert (b["count"][k], b["valid"][k]) == (63, False), name
    run = CASES["pivot_equal_u"]["items"][0]["runs"][0]
    assert run["count"][0] == N and run["ratios"][0][1] == 0.0 and not run["valid"][0]
    run = CASES["pivot_singular"]["items"][0]["runs"][0]
    k = ec.PIVOT_STEP - 1
    assert run["count"][k] >= 64 and not run["valid"][k]
    assert min(v for v in run["ratios"][k] if v is not None) <= 1e-14
    assert all(run["valid"][j] for j in range(7) if j != k)
    run = CASES["pivot_ill"]["items"][0]["runs"][0]
    assert run["valid"][k] and 1e-10 <= min(run["ratios"][k]) <= 1e-4
    st = stored("pivot_singular")[0]
    assert not (st.runs[0].stops == ec.PIVOT_STEP).any()


def test_the_singular_pivot_is_singular_in_float64_too():
    """(b): the host engine's arithmetic on the fit of the shifted step gives a
    first pivot ratio of at most 1e-13, a decade under the rule's 1e-12: the
    step is invalid on both sides of any summation-order noise."""
    st = stored("pivot_singular")[0]
    c, doc = st.contract, CASES["pivot_singular"]
    x = ec.float_walk(c, 0, doc["antithetic"], doc["seed"], 2 * st.stream_id)
    strike = c.params[capi.LSM_P_STRIKE]
    u = ec.float_regressor(c, x, ec.PIVOT_STEP)[np.exp(x[:, ec.PIVOT_STEP - 1]) < strike]
    assert u.size == doc["items"][0]["runs"][0]["count"][ec.PIVOT_STEP - 1]
    s0, s1, s2 = float(u.size), float(np.sum(u)), float(np.sum(u * u))
    l10 = s1 / math.sqrt(s0)
    assert (s2 - l10 * l10) / s2 <= 1e-13


@pytest.mark.parametrize("name", ec.REGENERATED)
def test_regenerating_a_case_gives_the_fixture_exactly(name):
    arrays = {}
    doc = ec.case_to_fixture(ec.build_case(name), arrays)
    assert doc == CASES[name]
    assert sorted(arrays) == sorted(k for k in ARRAYS if k.startswith(name + "/"))
    for k, v in arrays.items():
        assert np.array_equal(v, ARRAYS[k]), k


# ---------------------------------------------------------------------------
# 3. the host engine against every case
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.MENU))
def test_host_engine_against_the_reference(name):
    """Flags, invalid_fit_steps, every fit within fit_bound(u) on its fit
    paths, every price-set value within 1e-11 |ref| + 1e-12 spot (the paths of
    stored low-margin decisions left out), in-sample mean, smallest margin.
    Worst error-to-bound ratios per family: DESIGN.md 13.1."""
    doc = CASES[name]
    for k, st in enumerate(stored(name)):
        h = mc_american.host_subruns(st.contract, doc["subruns"], doc["antithetic"], doc["seed"],
                                     st.stream_id)
        worst = ec.check_engine(doc, st, h["coef"], h["values"], h["invalid"].sum(),
                                float(h["margin"].min()), fit_means=h["fit_mean"])
        print(f"{name}[{k}] ({doc['family']}): worst error / bound: fit {worst['fit']:.3g}, "
              f"value {worst['value']:.3g}, margin {worst['margin']:.3g}")


def test_no_exercise_at_an_invalid_step_and_its_neighbours_stand():
    """(a), (b): invalid_fit_steps counts the step, no path of either set
    exercises there voluntarily (host engine: no value equals an exercise
    there), the other steps' fits are those of the unedited contract."""
    st = stored("pivot_singular")[0]
    doc = CASES["pivot_singular"]
    c, m = st.contract, ec.PIVOT_STEP
    h = mc_american.host_subruns(c, [0], False, doc["seed"], st.stream_id)
    assert h["invalid"][0] == 1 and h["coef"][0, m - 1, 4] == 0.0
    x = ec.float_walk(c, 0, False, doc["seed"], 2 * st.stream_id + 1)
    paid_there = np.maximum(c.params[capi.LSM_P_STRIKE] - np.exp(x[:, m - 1]), 0.0) \
        * c.step[m - 1, capi.LSM_S_DF_END]
    itm = paid_there > 0.0
    assert not np.any(np.abs(h["values"][0][itm] - paid_there[itm]) <= 1e-9)
    plain = ec.contract("none", "put")
    r = lr.reference_subrun(plain, 0, False, doc["seed"], st.stream_id)
    later = np.array([[float(v) for v in row] for row in r["coef"][m:]])
    assert np.array_equal(later, st.runs[0].coef[m:])  # steps after it: the same fits
    st = stored("pivot_equal_u")[0]
    doc = CASES["pivot_equal_u"]
    h = mc_american.host_subruns(st.contract, [0], False, doc["seed"], st.stream_id,
                                 want_fit=True)
    assert h["invalid"][0] == 1 and not h["coef"][0, 0].any()
    assert (st.runs[0].stops == 2).all()


# ---------------------------------------------------------------------------
# 4. the finalize formulas
# ---------------------------------------------------------------------------
def test_finalize_on_nearly_equal_means():
    """Sub-run means equal to about 1e-9: the one-pass stderr of the engines'
    finalize against the reference's two-pass value, within the cancellation
    bound of DESIGN.md 13.1."""
    st = stored("finalize")[0]
    means = [mp.mpf(r.doc["price_mean"]) for r in st.runs]
    G = len(means)
    with mp.workdps(lr.DPS):
        mean = mp.fsum(means) / G
        want = float(mp.sqrt(mp.fsum((v - mean) ** 2 for v in means) / (G - 1) / G))
        spread = float(max(means) - min(means)) / float(mean)
    assert G == 4 and 1e-11 < spread < 1e-8
    got = mc_american._finalize(floats(means), floats(means), 0, math.inf)
    bound = ec.stderr_bound(means)
    print(f"finalize: two-pass stderr {want:.3e}, one-pass {got[capi.LSM_O_STDERR]:.3e}, "
          f"bound {bound:.3e}")
    assert abs(got[capi.LSM_O_STDERR] - want) <= bound
    assert want < bound  # the truth is below the one-pass formula's noise here
