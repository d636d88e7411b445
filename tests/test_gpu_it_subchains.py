"""The one-wave IT variant at 32 nodes per lane, fdcn_march<1,1,32,0>, on two
sub-chains of M = 16 nodes (it ran four of 8): what the 257/258-node grids of
test_gpu_it_tables.py cannot reach.  Nothing below depends on the sub-chain
count, so the cases hold for an A/B library built with another one.

Rule of test_gpu_kernels.py: B = 3 solves forced to the variant, every node of
v_out against the C oracle (oracle/fdcn_oracle.c),
max_j |V_gpu - V_oracle| <= 1e-10 * max(1, max_j |V_oracle|) per solve.  The
batches are those of test_gpu_it_tables.py: a put with the sum-form lower
Dirichlet value, a call, and a put with the product form.

* full wave: 2049 nodes are 64 active lanes with one short lane (lane 63
  receives no backward carry; the short lane's D'' sits on the last sub-chain,
  whose table has M = 16 entries), 2050 nodes the same with no short lane;
* fold across lanes: at 2049 nodes the Sherman-Morrison extent
  (capi.sm_extent) exceeds 64 nodes, so fold rows lie on more than two lanes;
  a high (0.48) and a low (0.18) volatility;
* phase switch: no Rannacher step / two of them over 131 steps (the table
  registers are reloaded at step 2; the last 64-step block is ragged);
* accumulated tau (FDCN_I_TAU_MODE = 1) from tau0 = 0.037 on 257 nodes.
"""
import math

import numpy as np
import pytest

from finite_difference_amd import capi
from finite_difference_amd.engine import (FORM_PROD, FORM_SUM, Boundary, Engine, Solve,
                                          operator_coefficients, pack)

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_kernels.py
NPT = 32
KINDS = ("put", "call", "put_prod")


def american(n_nodes, n_time, sigma, kind, n_ranna=2, tau_acc=False, tau0=0.0):
    """One American solve on a log grid; kind: 'put', 'call' or 'put_prod'."""
    r, b, T, K = 0.05, 0.03, 0.5, 100.0
    x_min, x_max = math.log(40.0), math.log(250.0)
    dx = (x_max - x_min) / (n_nodes - 1)
    s = np.array([math.exp(x_min + i * dx) for i in range(n_nodes)])
    a, c, bc = operator_coefficients(sigma, b, 0.0, r, dx)
    if kind == "call":
        pay = np.maximum(s - K, 0.0)
        lower = Boundary(FORM_SUM, 0.0, 0.0, 0.0, 0.0)
        upper = Boundary(FORM_SUM, float(s[-1]), b - r, -K, -r)
    else:
        pay = np.maximum(K - s, 0.0)
        upper = Boundary()
        if kind == "put_prod":
            lower = Boundary(FORM_PROD, K, -r, float(s[0]), b - r)
        else:
            lower = Boundary(FORM_SUM, K, -r, 0.0, 0.0)
    return Solve(it=True, n_time=n_time, n_ranna=n_ranna, dt=T / n_time, coeffs=(a, c, bc),
                 v_init=pay.copy(), lower=lower, upper=upper, tau0=tau0, tau_accumulate=tau_acc,
                 payoff=pay.copy())


def batch(n_nodes, n_time, sigmas=(0.25, 0.30, 0.35), **kw):
    return [american(n_nodes, n_time, sg, kind, **kw) for sg, kind in zip(sigmas, KINDS)]


class OracleBackend:
    name = "oracle"

    def run_group(self, g):
        from oracle import oracle
        return oracle.it_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                               g.payoff, 4)


def extent(solves):
    g = pack(solves, list(range(len(solves))))
    return capi.sm_extent(g.n_nodes, g.n_time, g.n_ranna, g.params)


def check(solves, label, force_variant):
    n_nodes, B = solves[0].n_nodes, len(solves)
    k_cap = extent(solves)
    force_variant(1, NPT, 0)
    assert capi.variant_name(n_nodes, True, k_cap, B=B) == f"fdcn_march<1,1,{NPT},0>"
    gpu = Engine().run(solves)
    ref = Engine(OracleBackend()).run(solves)
    worst = 0.0
    for g, r in zip(gpu, ref):
        assert g.shape == r.shape == (n_nodes,)
        assert np.all(np.isfinite(g)), f"{label}: non-finite GPU output"
        worst = max(worst, float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r)))))
    print(f"[{label}] sm_extent={k_cap} worst_rel_err={worst:.3e}")
    assert worst <= TOL, f"{label}: {worst:.3e} > {TOL}"


@pytest.mark.parametrize("n_nodes", [2049, 2050])
def test_full_wave(n_nodes, force_variant):
    n_int = n_nodes - 2
    lanes = -(-n_int // NPT)
    assert lanes == 64 and lanes * NPT - n_int == (1 if n_nodes == 2049 else 0)
    check(batch(n_nodes, 64), f"it NPT=32 n={n_nodes} m=64", force_variant)


@pytest.mark.parametrize("sigma", [0.48, 0.18])
def test_fold_across_lanes(sigma, force_variant):
    solves = batch(2049, 64, sigmas=(sigma,) * 3)
    k = extent(solves)
    print(f"[fold sigma={sigma}] sm_extent={k} nodes = {-(-k // NPT)} lanes of {NPT}")
    if k <= 64:
        pytest.skip(f"SKIPPED, NOTHING CHECKED: sm_extent {k} <= 64 at sigma={sigma}: "
                    "the fold rows do not span several lanes; choose other parameters")
    assert k > 64
    check(solves, f"it NPT=32 n=2049 m=64 sigma={sigma}", force_variant)


@pytest.mark.parametrize("n_ranna", [0, 2])
def test_phase_switch(n_ranna, force_variant):
    check(batch(2049, 131, n_ranna=n_ranna), f"it NPT=32 n=2049 m=131 n_ranna={n_ranna}",
          force_variant)


def test_accumulated_tau(force_variant):
    solves = batch(257, 131, tau_acc=True, tau0=0.037)
    check(solves, "it NPT=32 n=257 m=131 accumulated tau", force_variant)
