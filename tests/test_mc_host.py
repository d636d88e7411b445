"""Monte Carlo discrete-barrier pricer, CPU side: the façade's host engine on
the reference's normals against the reference's recorded numbers
(tests/golden/mc_cases.json, written by make_golden_mc.py), the errors it
raises, the Philox contract's known answers, the merge of sharded statistics,
and the C ABI's argument validation (which happens before any device call)."""
import ctypes
import datetime as dt

import numpy as np
import pytest

import mc_fixture as fx
from finite_difference_amd import capi, mc_barrier
from finite_difference_amd.mc_barrier import (BarrierSpec, MCConfig, RebateSpec,
                                              price_discrete_barrier_mc)

CASES = fx.load_cases()
ARRAYS = fx.load_arrays()
REL = 1e-13


def _close(got, ref, rel=REL):
    assert abs(got - ref) <= rel * abs(ref), (got, ref)


@pytest.mark.parametrize("case", CASES["small"] + CASES["large"], ids=lambda c: c["name"])
def test_host_engine_reproduces_the_reference(case):
    """Same normals (default_rng(seed), chunk by chunk), same arithmetic in
    the same order: price and stderr to 1e-13 relative, every other field
    equal."""
    out = price_discrete_barrier_mc(engine="host", rng="numpy",
                                    **fx.kwargs_for(case["inputs"], mc_barrier))
    ref = case["result"]
    assert sorted(out) == sorted(ref)
    _close(out["price"], ref["price"])
    _close(out["stderr"], ref["stderr"])
    for lo, hi in zip(out["ci_95"], ref["ci_95"]):
        assert abs(lo - hi) <= REL * abs(ref["price"])
    for key in ("n_observations", "antithetic", "grid_points", "steps", "barrier_type",
                "barrier_level", "barrier_band", "dividend_before_monitor"):
        assert out[key] == ref[key], key


@pytest.mark.parametrize("case", CASES["small"], ids=lambda c: c["name"])
def test_host_payoffs_and_step_arrays_match_the_fixture(case):
    plan = mc_barrier.plan_contract(**fx.kwargs_for(case["inputs"], mc_barrier))
    assert plan.step.tolist() == case["step"]
    assert plan.params.tolist() == case["params"] and plan.flags.tolist() == case["flags"]
    z = ARRAYS[case["normals"]]
    _, pay = mc_barrier.simulate([plan], z.shape[0], case["inputs"]["cfg"]["antithetic"],
                                 engine="host", z=z, want_payoffs=True)
    ref = ARRAYS[case["payoffs"]]
    assert np.all(np.abs(pay[0] - ref) <= REL * np.abs(ref))


def test_fixtures_cover_what_they_must():
    small = [c["inputs"] for c in CASES["small"]]
    assert {c["barrier"]["type"] for c in small} == set(capi.MC_KIND)
    assert {c["option_type"] for c in small} == {"call", "put"}
    assert {CASES["small"][k]["result"]["steps"] for k in range(len(small))} == {1, 3, 8}
    assert any(c["barrier"]["tol_bps"] == 1.0 for c in small)
    for at_hit in (True, False):
        assert any(c["rebate"]["at_hit"] is at_hit and c["rebate"]["amount"] != 0.0
                   and c["barrier"]["type"].endswith("out") for c in small)
    for flag in (True, False):
        assert any(c["cfg"]["dividend_before_monitor"] is flag for c in small)
        assert any(c["cfg"]["antithetic"] is flag for c in small)
    assert any(not c["include_maturity_monitor"] for c in small)
    # the dividend date is monitored where the ordering flag is exercised
    assert any(d in c["monitor_dates"] for c in small for d, _ in c["dividends"])


def _base():
    return fx.kwargs_for(CASES["small"][2]["inputs"], mc_barrier)  # up-and-out call


@pytest.mark.parametrize("change,match", [
    (dict(spot=0.0), "spot and strike"),
    (dict(strike=-1.0), "spot and strike"),
    (dict(vol=-0.1), "vol"),
    (dict(maturity=dt.date(2025, 7, 28)), "maturity"),
    (dict(barrier=BarrierSpec("up-and-out", None)), "barrier.level"),
    (dict(barrier=BarrierSpec("down-and-in", 0.0)), "barrier.level"),
    (dict(cfg=MCConfig(n_paths=0)), "n_paths"),
    (dict(cfg=MCConfig(n_paths=1, antithetic=True)), "n_paths >= 2"),
    (dict(maturity=dt.date(2026, 1, 5)), "NACA not found"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_raises_on_the_references_bad_inputs(change, match):
    kw = {**_base(), **change}
    with pytest.raises(ValueError, match=match):
        price_discrete_barrier_mc(engine="host", **kw)


def test_curve_rejects_bad_frames():
    import pandas as pd
    val = dt.date(2025, 7, 28)
    with pytest.raises(ValueError, match="columns"):
        mc_barrier.NacaCurve(pd.DataFrame({"Day": ["2025-07-28"], "NACA": [0.07]}), val)
    with pytest.raises(ValueError, match="non-numeric"):
        mc_barrier.NacaCurve(pd.DataFrame({"Date": ["2025-07-28"], "NACA": ["x"]}), val)
    c = fx.flat_curve(mc_barrier, 0.073086, val)
    d0, d1 = dt.date(2025, 8, 4), dt.date(2025, 8, 28)
    assert c.year_fraction(d0, d1) == 24 / 365.0 and c.year_fraction(d1, d0) == 0.0
    assert c.get_discount_factor(d1) == 1.073086 ** (-(31 / 365.0))
    fwd = c.get_forward_nacc_rate(d0, d1)
    assert abs(fwd - np.log(1.073086)) < 1e-12


def test_unknown_engine_or_rng_is_an_error():
    with pytest.raises(ValueError, match="engine"):
        price_discrete_barrier_mc(engine="cuda", **_base())
    with pytest.raises(ValueError, match="rng"):
        price_discrete_barrier_mc(engine="host", rng="mt", **_base())


def test_package_exports_the_reference_names():
    import finite_difference_amd as pkg
    for name in ("NacaCurve", "BarrierSpec", "RebateSpec", "MCConfig",
                 "price_discrete_barrier_mc", "mc_barrier_batch", "merge_mc_stats"):
        assert getattr(pkg, name) is getattr(mc_barrier, name)


# ---------------------------------------------------------------------------
# Philox
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    """The Random123 known-answer vectors, on the tests' restatement and on the
    package's host generator."""
    assert tuple(int(x) for x in fx.philox(*ctr, *key)) == want
    got = mc_barrier.philox4x32_10(np.array([ctr], dtype=np.uint64), key)
    assert tuple(int(x) for x in got[0]) == want


@pytest.mark.parametrize("n_steps", [1, 2, 3, 8])
def test_host_generator_is_the_documented_mapping(n_steps):
    for seed, stream, first in [(7, 0, 0), (2 ** 63 + 11, 5, 2 ** 32 - 100)]:
        got = mc_barrier.philox_normals(200, n_steps, seed, stream, first)
        assert np.array_equal(got, fx.expected_normals(200, n_steps, seed, stream, first))


# ---------------------------------------------------------------------------
# merging shards
# ---------------------------------------------------------------------------
def test_merge_of_two_halves_equals_the_whole():
    kw = {k: v for k, v in _base().items() if k != "cfg"}
    cfg = MCConfig(n_paths=6000, seed=3, antithetic=True, chunk_size=1000)
    whole = mc_barrier.mc_barrier_batch([kw], cfg, engine="host", rng="philox")[0]
    parts = [mc_barrier.mc_barrier_batch([kw], cfg, engine="host", rng="philox", obs_range=r)[0]
             for r in (range(0, 1300), range(1300, 3000))]
    merged = mc_barrier.merge_mc_stats(parts)
    assert merged["n_observations"] == whole["n_observations"] == 3000
    _close(merged["price"], whole["price"], 1e-14)
    _close(merged["stderr"], whole["stderr"], 1e-12)
    again = mc_barrier.merge_mc_stats([(p["n_observations"], p["sum_p"], p["sum_p2"])
                                       for p in parts])
    assert again["price"] == merged["price"] and again["stderr"] == merged["stderr"]
    with pytest.raises(ValueError):
        mc_barrier.merge_mc_stats([])


def test_batch_groups_by_step_count_and_keeps_the_order():
    cfg = MCConfig(n_paths=512, seed=5, antithetic=False, chunk_size=512)
    kws = [{k: v for k, v in fx.kwargs_for(c["inputs"], mc_barrier).items() if k != "cfg"}
           for c in CASES["small"]]
    out = mc_barrier.mc_barrier_batch(kws, cfg, engine="host", rng="numpy")
    assert [o["steps"] for o in out] == [c["result"]["steps"] for c in CASES["small"]]
    for kw, o in zip(kws, out):
        one = price_discrete_barrier_mc(engine="host", rng="numpy", cfg=cfg, **kw)
        assert o["price"] == one["price"] and o["stderr"] == one["stderr"]


# ---------------------------------------------------------------------------
# C ABI: validation happens before any device is touched
# ---------------------------------------------------------------------------
def _raw(B=1, n_steps=2, n_obs=8, antithetic=1, params=None, flags=None, null=()):
    P = np.ascontiguousarray(params if params is not None
                             else [[100.0, 100.0, 0.99, 90.0, 1.0, 1e-12]] * max(B, 1))
    F = np.ascontiguousarray(flags if flags is not None else [[0, 1, 0, 1, 0]] * max(B, 1),
                             dtype=np.int32)
    S = np.zeros((max(B, 1), max(n_steps, 1), capi.MC_NSTEP))
    S[..., capi.MC_S_DIFF] = 0.1
    S[..., capi.MC_S_MONITOR] = 1.0
    S[..., capi.MC_S_DF_END] = 0.99
    stats = np.zeros((max(B, 1), capi.MC_NSTAT))
    ptr = {"params": P.ctypes.data, "flags": F.ctypes.data, "step": S.ctypes.data,
           "stats": stats.ctypes.data}
    for name in null:
        ptr[name] = None
    L = capi.lib()
    rc = L.fdcn_mc_barrier_batch(B, n_steps, n_obs, antithetic, ptr["params"], ptr["flags"],
                                 ptr["step"], None, 7, 0, ptr["stats"], None)
    return rc, L.fdcn_last_error().decode(), stats


@pytest.mark.parametrize("kw,word", [
    (dict(B=0), "B"), (dict(n_steps=0), "n_steps"), (dict(n_obs=0), "n_obs"),
    (dict(antithetic=2), "antithetic"),
    (dict(flags=[[2, 1, 0, 1, 0]]), "put"), (dict(flags=[[0, 5, 0, 1, 0]]), "kind"),
    (dict(flags=[[0, -1, 0, 1, 0]]), "kind"), (dict(flags=[[0, 1, 2, 1, 0]]), "rebate_at_hit"),
    (dict(flags=[[0, 1, 0, -1, 0]]), "dividend_before_monitor"),
    (dict(flags=[[0, 1, 0, 1, -3]]), "stream"),
    (dict(params=[[0.0, 100.0, 0.99, 90.0, 1.0, 1e-12]]), "spot"),
    (dict(params=[[100.0, -5.0, 0.99, 90.0, 1.0, 1e-12]]), "strike"),
    (dict(params=[[100.0, 100.0, 0.99, 0.0, 1.0, 1e-12]]), "threshold"),
    (dict(null=("params",)), "params"), (dict(null=("flags",)), "flags"),
    (dict(null=("step",)), "step"), (dict(null=("stats",)), "stats"),
], ids=lambda v: v if isinstance(v, str) else "")
def test_host_entry_rejects_bad_arguments(kw, word):
    rc, msg, _ = _raw(**kw)
    assert rc == -1 and word in msg, (rc, msg)


def test_second_contract_is_validated_too():
    rc, msg, _ = _raw(B=2, flags=[[0, 1, 0, 1, 0], [0, 9, 0, 1, 1]])
    assert rc == -1 and "contract 1" in msg and "kind" in msg, (rc, msg)


def test_threshold_is_not_required_without_a_barrier():
    rc, msg, _ = _raw(params=[[100.0, 100.0, 0.99, 0.0, 0.0, 1e-12]], flags=[[1, 0, 0, 1, 0]])
    assert rc in (0, -3), (rc, msg)


def test_host_entry_accepts_a_valid_plan_until_the_device():
    rc, msg, stats = _raw()
    assert rc in (0, -3), (rc, msg)
    if rc == 0:
        assert np.isfinite(stats).all() and stats[0, 0] >= 0.0


def test_dev_entry_rejects_a_short_workspace_before_the_device():
    """The pointers are never dereferenced: the sizes are checked first."""
    need = capi.mc_plan(5000)["ws_bytes_per_contract"] * 3
    buf = np.zeros(8)
    p = buf.ctypes.data
    L = capi.lib()
    rc = L.fdcn_mc_barrier_batch_dev(3, 2, 5000, 1, p, p, p, None, 7, 0, p, None, p, need - 1, None)
    assert rc == -1 and "workspace" in L.fdcn_last_error().decode()
    rc = L.fdcn_mc_barrier_batch_dev(3, 2, 5000, 1, p, p, None, None, 7, 0, p, None, p, need, None)
    assert rc == -1 and "step" in L.fdcn_last_error().decode()
    rc = L.fdcn_mc_normals(0, 2, 7, 0, 0, p)
    assert rc == -1 and "n_obs" in L.fdcn_last_error().decode()


def test_mc_plan_runs_without_a_gpu():
    per = capi.mc_plan(1)["obs_per_block"]
    assert per >= 256 and per % 256 == 0
    for n in (1, per - 1, per, per + 1, 10 * per + 7, 4_000_000):
        p = capi.mc_plan(n)
        assert p["obs_per_block"] == per  # the chunk depends on nothing
        assert p["blocks_per_contract"] == -(-n // per)
        assert p["ws_bytes_per_contract"] == 16 * p["blocks_per_contract"]
    with pytest.raises(capi.FdcnError):
        capi.mc_plan(0)
    assert isinstance(ctypes.c_int64(capi.mc_plan(2 ** 33)["ws_bytes_per_contract"]).value, int)
