"""Device-resident sessions (csrc/fdcn_session.hip, session.py) on the MI355X.

* a march in a session gives the host-array ABI's vectors bitwise (same
  kernel); chained marches (v_init from slots) equal the oracle's segments;
* the device dividend jump is bit-identical to fdcn_dividend_jump (the host C
  restatement of fd_american_equity.py:479-553, :732-772, itself bitwise the
  NumPy/reference spline);
* the device Greeks epilogue equals the host epilogue of the facades on the
  same GPU value vectors: bitwise for the barrier (…pricer.py:883-904) and
  CN-log (_cn.py:429-466) kinds, whose formulas are plain arithmetic in the
  reference's order; to 1e-12 relative (Delta/Gamma/theta 1.6e-12, eight
  times the measured worst) for the American kind, whose 4x4 cubic fit is a
  different LU than numpy's LAPACK;
* the American trades with one and two discrete dividends (device jumps)
  match the reference's golden numbers (tolerances of test_gpu_pricers).
"""
import numpy as np
import pytest

from finite_difference_amd import capi, scenarios
from finite_difference_amd.engine import Engine, HipBackend, group_solves, pack
from finite_difference_amd.session import Session
from plan_factory import random_solve

pytestmark = pytest.mark.gpu


class HipHostEpilogue:
    """The HIP march with the value vectors copied back and the facades'
    host epilogue (Engine.on_device is False for this backend)."""
    name = "hip-host-epilogue"

    def run_group(self, g):
        return HipBackend().run_group(g)


def host_engine():
    return Engine(HipHostEpilogue())


def test_session_march_and_fetch_equal_host_abi():
    rng = np.random.default_rng(31)
    solves = ([random_solve(rng, 2049, 64, 2, it=True) for _ in range(3)] +
              [random_solve(rng, 1024, 80, 2, it=False) for _ in range(4)])
    ref = Engine().run(solves)
    with Session() as S:
        slots = Engine().march_slots(S, solves)
        assert S.slots() == len(solves)
        for s, sl, r in zip(solves, slots, ref):
            got = S.fetch([sl], s.n_nodes)[0]
            assert np.array_equal(got, r)


def test_chained_marches_equal_two_oracle_segments():
    """Two IT launches of n/2 steps, the second starting from the first's
    slots (no Rannacher restart, tau0 carried on, accumulated tau), equal the
    oracle marching the same two segments (the multiplier restarts at 0 at
    each segment, as _solve_segment's does)."""
    rng = np.random.default_rng(8)
    n_time = 60
    full = [random_solve(rng, 513, n_time, 2, it=True) for _ in range(3)]
    for s in full:
        s.tau_accumulate = True
    ref = Engine().run(full)
    import copy
    first = [copy.copy(s) for s in full]
    second = [copy.copy(s) for s in full]
    for a, b in zip(first, second):
        a.n_time = b.n_time = n_time // 2
        b.n_ranna = 0
        b.tau0 = capi.tau_sequence(a.tau0, a.dt, a.n_time)[-1]
    with Session() as S:
        e = Engine()
        s1 = e.march_slots(S, first)
        s2 = e.march_slots(S, second, list(s1))
        got = S.fetch(s2, full[0].n_nodes)
    # the split march restarts the IT multiplier at the segment boundary
    # (lambda = 0 at every _solve_segment start, fd_american_equity.py:661),
    # so compare with the oracle doing the same two segments
    from backends import oracle_engine
    o = oracle_engine()
    mid = o.run(first)
    for b, v in zip(second, mid):
        b.v_init = v
    want = o.run(second)
    for g, w in zip(got, want):
        assert np.max(np.abs(g - w)) <= 1e-10 * max(1.0, np.max(np.abs(w)))


def test_device_dividend_jump_is_bitwise_host():
    rng = np.random.default_rng(12)
    n = 2049
    B = 6
    s = np.sort(rng.uniform(20.0, 400.0, (B, n)), axis=1)
    v = np.maximum(160.0 - s, 0.0) + rng.uniform(0.0, 0.5, (B, n))
    cash = rng.uniform(0.2, 4.0, B)
    strike = np.where(np.arange(B) % 2 == 0, -1.0, 150.0)
    ref = np.array([capi.dividend_jump(s[b], v[b], cash[b], strike[b]) for b in range(B)])
    solves = []
    for b in range(B):  # put the vectors into slots through a zero-step march
        sv = random_solve(rng, n, 0, 0, it=False, ko=False)
        sv.v_init = v[b].copy()
        solves.append(sv)
    with Session() as S:
        sl = Engine().march_slots(S, solves)
        assert np.array_equal(S.fetch(sl, n), v)
        out = S.dividend_jump(sl, s, cash, strike)
        got = S.fetch(out, n)
    assert np.array_equal(got, ref)


def test_session_rejects_bad_slots():
    rng = np.random.default_rng(3)
    sv = random_solve(rng, 300, 10, 2, it=False)
    with Session() as S:
        with pytest.raises(capi.FdcnError, match="slot"):
            S.fetch([0], 300)
        sl = Engine().march_slots(S, [sv])
        with pytest.raises(capi.FdcnError, match="nodes"):
            S.fetch(sl, 299)


def _barrier_cases():
    from conftest import load_golden
    return load_golden("barrier_cases.json")["cases"]


def test_barrier_device_epilogue_is_bitwise_host_epilogue():
    from test_barrier_host import make
    for case in _barrier_cases():
        dev = make(case["inputs"], Engine())
        host = make(case["inputs"], host_engine())
        assert dev.price_log2() == host.price_log2(), case["name"]
        assert dev.greeks_log2() == host.greeks_log2(), case["name"]


def test_batched_runner_device_epilogue_is_bitwise_host():
    from test_barrier_host import _mixed_rows
    base = scenarios.runner_base_params("put", 64)
    base.update(num_time_steps=40, grid_mode="explicit")
    rows = _mixed_rows(25, 5)
    a = scenarios.run_rows_batched(rows, base, Engine())
    b = scenarios.run_rows_batched(rows, base, host_engine())
    for ra, rb in zip(a, b):
        for k in ("model_price", "model_delta", "model_gamma", "model_vega"):
            assert ra[k] == rb[k] or (np.isnan(ra[k]) and np.isnan(rb[k])), (k, ra, rb)


def test_cn_log_device_epilogue_is_bitwise_host():
    import test_cn_log_host as T
    from conftest import load_golden
    for case in load_golden("cn_log_cases.json"):
        inp = case["inputs"]
        if not inp["bt"].endswith("out"):
            continue
        dev, host = T.make(inp, Engine()), T.make(inp, host_engine())
        assert dev.price() == host.price()
        assert dev.greeks() == host.greeks()


AMERICAN_FIT_TOL = 8 * 1.94e-13


@pytest.mark.parametrize("which", ["american", "black76"])
def test_american_device_epilogue_matches_host(which):
    """The kernel's cubic fit is its own LU, numpy's is LAPACK's: not the
    same bits, but two orderings of one 4x4 solve.  Measured on the MI355X
    over these eight contracts, |device - host| / max(1, |host|) is at most
    2.2e-15 for Delta, 3.3e-15 for Gamma and 1.94e-13 for theta (price and
    vega: 0); AMERICAN_FIT_TOL is that worst figure times the factor 8 of
    the rounding yardsticks (it was 1e-7).  test_gpu_session_epilogue.py
    holds the kernel's fit to the exact solve, case by case."""
    if which == "american":
        import test_american_host as T
    else:
        import test_black76_host as T
    for case in T.CASES:
        dev, host = T.make(case, Engine()), T.make(case, host_engine())
        pd_, ph = dev.price_log2(), host.price_log2()
        assert abs(pd_ - ph) <= 1e-12 * max(1.0, abs(ph)), (case["name"], pd_, ph)
        gd, gh = dev.greeks_log2(), host.greeks_log2()
        assert abs(gd["price"] - gh["price"]) <= 1e-12 * max(1.0, abs(gh["price"]))
        assert abs(gd["vega"] - gh["vega"]) <= 1e-12 * max(1.0, abs(gh["vega"]))
        for k in ("delta", "gamma", "theta"):
            assert abs(gd[k] - gh[k]) <= AMERICAN_FIT_TOL * max(1.0, abs(gh[k])), (
                case["name"], k, gd, gh)


def test_american_dividend_trades_on_device_match_reference():
    """put_1div / call_2div: segments in lock-step launches, the spline jumps
    on the device in between (no host round trip), Richardson epilogue on
    the device; against the reference's own numbers."""
    import test_american_host as T
    from test_gpu_pricers import check_greeks, close
    divs = [c for c in T.CASES if c["inputs"]["divs"]]
    assert {c["name"] for c in divs} == {"put_1div", "call_2div"}
    for case in divs:
        p = T.make(case, Engine())
        assert close("price", p.price_log2(), case["price_log2"])
        check_greeks(p.greeks_log2(), case["greeks_log2"], "device " + case["name"])


def test_prefetch_many_device_matches_single_trades():
    import test_american_host as T
    from finite_difference_amd.american import prefetch_many
    batch = [T.make(c, Engine()) for c in T.CASES]
    prefetch_many(batch)
    for p, c in zip(batch, T.CASES):
        one = T.make(c, Engine())
        assert p.price_log2() == one.price_log2()
        assert p.greeks_log2() == one.greeks_log2()


@pytest.mark.parametrize("opt", ["put", "call"])
@pytest.mark.parametrize("chunk_rows", [2048, 3], ids=["one_chunk", "two_chunks"])
def test_vectorized_scenario_file_equals_batched_runner(opt, chunk_rows, monkeypatch):
    """scenario_batch (native plan, device epilogue; with two_chunks the
    rows planned and marched in two pipelined chunks) against
    run_rows_batched on the same GPU: the same 2R solves, so bitwise; and the
    host epilogue over the same vectors, bitwise."""
    import math
    import test_scenario_batch as T
    from finite_difference_amd import scenario_batch
    monkeypatch.setattr(scenario_batch, "CHUNK_ROWS", chunk_rows)
    base = scenarios.runner_base_params(opt, 64)
    base.update(num_time_steps=40, grid_mode="explicit", rebate_amount=0.5)
    rows = T._rows(40, 9)
    a = scenarios.run_rows_batched(rows, base, Engine())
    b = scenario_batch.run_rows_vectorized(rows, base, Engine())
    c = scenario_batch.run_rows_vectorized(rows, base, host_engine())
    for ra, rb, rc in zip(a, b, c):
        for k in ra:
            for x in (rb, rc):
                same = ra[k] == x[k] or (isinstance(ra[k], float) and math.isnan(ra[k])
                                         and math.isnan(x[k]))
                assert same, (ra["scenario_name"], k, ra[k], x[k])


def test_run_all_scenarios_file_on_device(tmp_path):
    """run_all_scenarios takes the vectorised path for a whole CSV and writes
    the per-row runner's numbers (oracle engine) to within the kernel's
    tolerance."""
    import pandas as pd
    import test_scenario_batch as T
    from backends import oracle_engine
    rows = T._rows(25, 4)
    cfg = tmp_path / "cfg.csv"
    pd.DataFrame(rows).to_csv(cfg, index=False)
    base = scenarios.runner_base_params("put", 64)
    base.update(num_time_steps=40, grid_mode="explicit")
    df = scenarios.run_all_scenarios(str(cfg), str(tmp_path / "out.csv"), base, Engine(),
                                     verbose=False)
    ref = scenarios.run_rows(rows, base, oracle_engine())
    assert len(df) == len(ref)
    for i, r in enumerate(ref):
        for k in ("model_price", "model_delta", "model_gamma", "model_vega"):
            assert abs(df[k].iloc[i] - r[k]) <= 1e-9 * max(1.0, abs(r[k])), (i, k)


@pytest.mark.parametrize("divs", [None, [(__import__("datetime").date(2025, 8, 11), 1.5)]],
                         ids=["nodiv", "div1"])
@pytest.mark.parametrize("chunk_rows", [500, 5], ids=["one_chunk", "two_chunks"])
def test_vectorized_american_file_equals_per_row_device(divs, chunk_rows, monkeypatch):
    """american_batch (native plan, lock-step segment launches, device jumps
    and epilogue; with two_chunks the rows planned and launched in two
    pipelined chunks) against the per-row façades' device path (greeks_many)
    on the same GPU: the same grids, so bitwise."""
    import test_american_batch as T
    from finite_difference_amd import american_batch
    from finite_difference_amd.american import prefetch_many
    monkeypatch.setattr(american_batch, "CHUNK_ROWS", chunk_rows)
    for opt in ("put", "call"):
        base = T._base(opt, divs, n=128, m=96)
        rows = T._rows(12, 4)
        ps = [scenarios.make_american_pricer(r["S0"], r["K"], r["sigma"], r["rate"],
                                             engine=Engine(), **base) for r in rows]
        prefetch_many(ps)
        cols = {k: [r[k] for r in rows] for k in american_batch.ROW_KEYS}
        res = american_batch.price_columns(cols, base, Engine())
        for i, p in enumerate(ps):
            assert res["price_log2"][i] == p.price_log2(), (opt, i)
            g = p.greeks_log2()
            for k in ("price", "delta", "gamma", "vega", "theta"):
                assert res[k][i] == g[k], (opt, i, k, res[k][i], g[k])


def test_destroy_drains_cross_stream_consumers_before_freeing():
    """ADVICE r2 (medium) / VERDICT r3 item 6: a slot produced on one session
    stream and read by a launch on another.  The session's fifth and sixth
    calls round-robin onto streams 0 and 1: the consumer march (v_init from
    the producer's slots, stream 1) is queued behind a long independent march
    (stream 1), while the producer's block was allocated on stream 0.
    fdcn_session_destroy must drain every stream before its stream-ordered
    frees (else the producer's block returns to the pool while the consumer
    has not read it yet): destroy takes at least the long march's time.  A
    new session on the same thread then allocates (from the same pool) and
    re-runs producer + consumer; its output equals the oracle's two chained
    segments."""
    import copy
    import time
    from backends import oracle_engine
    rng = np.random.default_rng(77)
    n, steps = 1024, 60
    prod = [random_solve(rng, n, steps, 2, it=False) for _ in range(8)]
    cons = [copy.copy(s) for s in prod]
    for c in cons:
        c.n_ranna = 0
    small = [random_solve(rng, 513, 20, 2, it=False) for _ in range(4)]
    long_one = random_solve(rng, 2049, 32768, 2, it=True)  # ~45 ms
    longs = [long_one] * 2048
    e = Engine()
    with Session() as S:  # the long march alone, fetched (its own time)
        t0 = time.perf_counter()
        sl = e.march_slots(S, longs)
        S.fetch(sl[:1], 2049)
        t_long = time.perf_counter() - t0
    S = Session()
    a = e.march_slots(S, prod)          # call 1: stream 0 (producer)
    e.march_slots(S, longs)             # call 2: stream 1 (long)
    e.march_slots(S, small[:2])         # call 3: stream 2
    e.march_slots(S, small[2:])         # call 4: stream 3
    e.march_slots(S, small[:1])         # call 5: stream 0
    e.march_slots(S, cons, list(a))     # call 6: stream 1, behind the long march
    t0 = time.perf_counter()
    S.close()
    t_destroy = time.perf_counter() - t0
    assert t_destroy >= 0.4 * t_long, (t_destroy, t_long)
    with Session() as S2:
        a2 = e.march_slots(S2, prod)
        b2 = e.march_slots(S2, cons, list(a2))
        got = S2.fetch(b2, n)
    o = oracle_engine()
    mid = o.run(prod)
    for c, v in zip(cons, mid):
        c.v_init = v
    want = o.run(cons)
    for g, w in zip(got, want):
        assert np.max(np.abs(g - w)) <= 1e-10 * max(1.0, np.max(np.abs(w)))


@pytest.mark.parametrize("where", ["v_direct", "payoff_is_v_direct", "payoff_direct_v_staged",
                                   "both_direct"])
def test_host_buffer_inputs_march_bitwise_as_staged(where):
    """fdcn_session_host_buffer: a payoff / v_init written into the session's
    pinned memory is copied to the device from there (no staging), in every
    combination the march's upload handles -- the CN march with v_init direct,
    the IT march with its payoff direct and v_init staged, v_init == payoff
    direct, both direct -- and the outputs equal the all-staged march bit for bit."""
    rng = np.random.default_rng(77)
    it = where != "v_direct"
    solves = [random_solve(rng, 1025, 48, 2, it=it) for _ in range(6)]
    g = pack(solves, list(range(len(solves))))
    if where == "payoff_is_v_direct":
        g.v_init = g.payoff  # the first segment of an American grid
    with Session() as S:
        ref = S.fetch(S.march(g), g.n_nodes)

        def pinned(a):
            buf = S.host_buffer(a.size).reshape(a.shape)
            buf[...] = a
            return buf
        import dataclasses
        h = dataclasses.replace(g)
        if where in ("v_direct", "both_direct"):
            h.v_init = pinned(g.v_init)
        if where in ("payoff_direct_v_staged", "both_direct"):
            h.payoff = pinned(g.payoff)
        if where == "payoff_is_v_direct":
            h.payoff = pinned(g.payoff)
            h.v_init = h.payoff
        got = S.fetch(S.march(h), g.n_nodes)
        del h
    assert np.array_equal(got, ref)
