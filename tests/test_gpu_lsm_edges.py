"""The least-squares Monte Carlo kernel (csrc/fdcn_mc_lsm.hip) against the
mpmath restatement of its contract at the decision edges: the fixture of
golden/make_golden_lsm_edges.py (lsm_reference.py evaluated on the menu of
lsm_edge_cases.py) under the derived bounds of DESIGN.md 13.1 -- the same
comparison test_lsm_edges_host.py runs on the NumPy host engine.  The 511- and
512-step launches go against the host engine only.  Every launch has valid
arguments."""
import mpmath as mp
import numpy as np
import pytest

import lsm_edge_cases as ec
import lsm_fixture as lf
import lsm_reference as lr
from conftest import GOLDEN, load_golden
from finite_difference_amd import capi, mc_american

pytestmark = pytest.mark.gpu

FIX = load_golden("lsm_edges.json")
ARRAYS = dict(np.load(GOLDEN + "/lsm_edges.npz"))
CASES = FIX["cases"]
N = capi.LSM_SUBRUN


@pytest.fixture(scope="module")
def launches():
    """Per case, once: the stored items and the device launch with both dumps
    (the contracts of a case share n_steps, antithetic, seed and sub-runs)."""
    out = {}
    for name, doc in CASES.items():
        items = ec.load_case(name, doc, ARRAYS)
        dev = mc_american.simulate_lsm(
            [it.contract for it in items], len(doc["subruns"]), doc["antithetic"], engine="hip",
            seed=doc["seed"], stream_ids=[it.stream_id for it in items],
            subrun_first=doc["subruns"][0], want_values=True, want_coef=True)
        out[name] = (items, dev)
    return out


@pytest.mark.parametrize("name", list(ec.MENU))
def test_device_against_the_reference(launches, name):
    """Flags and invalid_fit_steps equal; every valid fit within fit_bound(u)
    on its fit paths; every price-set value within 1e-11 |ref| + 1e-12 spot
    (a path stopped at another step is paid another amount; the paths of the
    stored low-margin decisions are left out); price, in-sample value and
    min_margin.  The printed worst error-to-bound ratios are results, recorded
    in DESIGN.md 13.1, not inputs to any tolerance."""
    doc = CASES[name]
    items, dev = launches[name]
    G = len(doc["subruns"])
    for b, st in enumerate(items):
        stats = dev["stats"][b]
        spot = float(st.contract.params[capi.LSM_P_SPOT])
        worst = ec.check_engine(doc, st, dev["coef"][b], dev["values"][b].reshape(G, N),
                                stats[capi.LSM_O_INVALID], float(stats[capi.LSM_O_MIN_MARGIN]))
        print(f"{name}[{b}] ({doc['family']}): worst error / bound: fit {worst['fit']:.3g}, "
              f"value {worst['value']:.3g}, margin {worst['margin']:.3g}")
        if st.doc["n_low_margin"] == 0:
            for key, col in (("price_mean", capi.LSM_O_PRICE), ("fit_mean", capi.LSM_O_FIT_VALUE)):
                want = sum(r.doc[key] for r in st.runs) / G
                assert abs(stats[col] - want) <= ec.value_bound(want, spot), (name, b, key)


def test_the_sharded_launch_is_sub_runs_five_to_seven(launches):
    """G = 3, antithetic, obs_first = 5 sub-runs' worth of observations: the
    merging sums are those of the reference's sub-runs 5, 6 and 7."""
    doc = CASES["sharded"]
    items, dev = launches["sharded"]
    assert doc["subruns"] == [5, 6, 7] and doc["antithetic"]
    st, stats = items[0], dev["stats"][0]
    means = np.array([r.doc["price_mean"] for r in st.runs])
    spot = float(st.contract.params[capi.LSM_P_SPOT])
    assert abs(stats[capi.LSM_O_SUM] - means.sum()) <= 3 * ec.value_bound(means.mean(), spot)
    assert abs(stats[capi.LSM_O_SUM2] - (means ** 2).sum()) \
        <= 2.0 * means.max() * 3 * ec.value_bound(means.mean(), spot)
    got = dev["values"][0].reshape(3, N).sum(axis=1) / N
    assert np.all(np.abs(got - means) <= ec.value_bound(means, spot))
    assert not np.allclose(got[0], got[1], rtol=1e-6)  # three different sub-runs


def test_finalize_on_nearly_equal_means(launches):
    """lsm_finalize_kernel's one-pass stderr where the sub-run means agree to
    about 1e-9 relative, against the reference's two-pass value: within the
    cancellation bound of DESIGN.md 13.1 plus the means' own tolerance."""
    items, dev = launches["finalize"]
    st, stats = items[0], dev["stats"][0]
    means = [mp.mpf(r.doc["price_mean"]) for r in st.runs]
    G = len(means)
    with mp.workdps(lr.DPS):
        mean = mp.fsum(means) / G
        want = float(mp.sqrt(mp.fsum((v - mean) ** 2 for v in means) / (G - 1) / G))
    spot = float(st.contract.params[capi.LSM_P_SPOT])
    bound = ec.stderr_bound(means) + 2.0 * float(ec.value_bound(float(mean), spot))
    got = float(stats[capi.LSM_O_STDERR])
    print(f"finalize: device stderr {got:.3e}, two-pass reference {want:.3e}, bound {bound:.3e}, "
          f"price {stats[capi.LSM_O_PRICE]:.15g}")
    assert abs(got - want) <= bound
    assert abs(stats[capi.LSM_O_PRICE] - float(mean)) <= ec.value_bound(float(mean), spot)


@pytest.mark.parametrize("M", [511, 512])
def test_the_longest_launches_against_the_host_engine(M):
    """n_steps = FDCN_LSM_MAX_STEPS (the whole coefficient table in LDS) and
    its odd neighbour (the last normal pair half used), exercise every 64th
    step, two monitored dates, G = 1: path for path against host_subruns under
    test_gpu_mc_american.py's tolerances.  The event rules were settled against
    the reference at eight steps."""
    plans = ec.long_contracts(M)
    ids = FIX["long"][str(M)]["stream_ids"]
    dev = mc_american.simulate_lsm(plans, 1, False, engine="hip", seed=ec.LONG_SEED,
                                   stream_ids=ids, want_values=True, want_coef=True)
    for b, (c, sid) in enumerate(zip(plans, ids)):
        h = mc_american.host_subruns(c, [0], False, ec.LONG_SEED, sid, want_fit=True)
        spot, strike = float(c.params[capi.LSM_P_SPOT]), float(c.params[capi.LSM_P_STRIKE])
        tau_c = lf.TAU_C_REL * strike
        assert float(h["margin"].min()) >= 100.0 * tau_c, (M, b)
        n_valid = int(h["coef"][0, :, 4].sum())  # seven fitted steps, 64 .. 448
        assert n_valid >= 1 and n_valid + int(h["invalid"][0]) == 7, (M, b)
        assert np.array_equal(dev["coef"][b][..., 4], h["coef"][..., 4]), (M, b)
        assert int(dev["stats"][b, capi.LSM_O_INVALID]) == int(h["invalid"].sum()), (M, b)
        gap = np.abs(lf.cubic(dev["coef"][b], h["fit_u"]) - lf.cubic(h["coef"], h["fit_u"]))
        assert float(np.nanmax(gap)) <= tau_c, (M, b, float(np.nanmax(gap)))
        ref = h["values"].reshape(-1)
        err = np.abs(dev["values"][b] - ref)
        assert np.all(err <= ec.value_bound(ref, spot)), (M, b, float(err.max()))
        price = float(ref.sum() / N)
        assert abs(dev["stats"][b, capi.LSM_O_PRICE] - price) <= ec.value_bound(price, spot)
        dm = float(dev["stats"][b, capi.LSM_O_MIN_MARGIN])
        assert abs(dm - float(h["margin"].min())) <= 2.0 * tau_c, (M, b)
        print(f"n_steps {M}[{b}] {c.barrier_type}: worst fit difference "
              f"{float(np.nanmax(gap)) / strike:.3e} x strike, worst value error "
              f"{float(np.max(err / ec.value_bound(ref, spot))):.3e} of its bound")
