"""The one-wave IT two-pass variants: homogeneous tables as DPP-broadcast
registers, boundary terms through the scalar unit.

Every forced variant fdcn_march<1,1,NPT,0> marches tiny American batches
(B = 3) and every node of v_out is compared with the C oracle
(oracle/fdcn_oracle.c) under the rule of test_gpu_kernels.py:
max_j |V_gpu - V_oracle| <= 1e-10 * max(1, max_j |V_oracle|) per solve.

Grids: each chunk length once with no short lane and once with one (the
short lane's phantom slot and its own table entry P'_0 - fm^(M-1) bm^(M-1)):

  NPT 32   258 / 257 nodes   S = 4, M = 8: one table register
  NPT 40   162 / 161         S = 1, M = 40: three table registers
  NPT 64   194 / 193         S = 2, M = 32: two table registers
  NPT 24    98 /  97         S = 1, M = 24: two table registers
  NPT  8    66 /  65         S = 1, one table register
  NPT  2     5               the planner's smallest grid (3 interior nodes):
                             the node-by-node update

Steps: 64, 128 and 131 with two Rannacher steps -- the boundary table is
padded to 64-step blocks, so the running scalar-load offset meets a table of
exactly one block, an exact block edge and a ragged tail, and the table
registers are reloaded at the phase switch (step 2).

Each batch holds a put with the sum-form lower Dirichlet value, a call (the
non-constant value at the upper end) and a put with the product form.  The
258-node grid also runs at a low (0.18) and a high (0.48) volatility (no
carry-scan stage / two of them in the Crank-Nicolson phase), and one batch
runs on accumulated tau (FDCN_I_TAU_MODE = 1, the American default) from a
non-zero tau0.
"""
import math

import numpy as np
import pytest

from finite_difference_amd import capi
from finite_difference_amd.engine import (FORM_PROD, FORM_SUM, Boundary, Engine, Solve,
                                          operator_coefficients)

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_kernels.py
N_RANNA = 2


def american(n_nodes, n_time, sigma, kind, tau_acc=False, tau0=0.0):
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
    return Solve(it=True, n_time=n_time, n_ranna=N_RANNA, dt=T / n_time, coeffs=(a, c, bc),
                 v_init=pay.copy(), lower=lower, upper=upper, tau0=tau0, tau_accumulate=tau_acc,
                 payoff=pay.copy())


class OracleBackend:
    name = "oracle"

    def run_group(self, g):
        from oracle import oracle
        return oracle.it_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                               g.payoff, 4)


def check(npt, solves, label, force_variant):
    n_nodes, B = solves[0].n_nodes, len(solves)
    force_variant(1, npt, 0)
    assert capi.variant_name(n_nodes, True, B=B) == f"fdcn_march<1,1,{npt},0>"
    gpu = Engine().run(solves)
    ref = Engine(OracleBackend()).run(solves)
    worst = 0.0
    for g, r in zip(gpu, ref):
        assert g.shape == r.shape == (n_nodes,)
        assert np.all(np.isfinite(g)), f"{label}: non-finite GPU output"
        worst = max(worst, float(np.max(np.abs(g - r))) / max(1.0, float(np.max(np.abs(r)))))
    print(f"[{label}] worst_rel_err={worst:.3e}")
    assert worst <= TOL, f"{label}: {worst:.3e} > {TOL}"


def batch(n_nodes, n_time, sigmas=(0.25, 0.30, 0.35), **kw):
    return [american(n_nodes, n_time, sg, kind, **kw)
            for sg, kind in zip(sigmas, ("put", "call", "put_prod"))]


# (NPT, n_nodes): no short lane, then one short lane
GRIDS = [(32, 258), (32, 257), (40, 162), (40, 161), (64, 194), (64, 193), (24, 98), (24, 97),
         (8, 66), (8, 65), (2, 5)]
N_TIMES = [64, 128, 131]


@pytest.mark.parametrize("n_time", N_TIMES)
@pytest.mark.parametrize("npt,n_nodes", GRIDS, ids=[f"npt{p}_n{n}" for p, n in GRIDS])
def test_forced_it_variant_vs_oracle(npt, n_nodes, n_time, force_variant):
    n_int = n_nodes - 2
    lanes = -(-n_int // npt)
    assert lanes * npt - n_int == (0 if n_nodes % 2 == 0 else 1)  # short lanes of this grid
    check(npt, batch(n_nodes, n_time), f"it NPT={npt} n={n_nodes} m={n_time}", force_variant)


@pytest.mark.parametrize("sigma", [0.18, 0.48])
def test_low_and_high_volatility(sigma, force_variant):
    check(32, batch(258, 131, sigmas=(sigma,) * 3), f"it NPT=32 n=258 sigma={sigma}",
          force_variant)


def test_accumulated_tau(force_variant):
    solves = batch(257, 131, tau_acc=True, tau0=0.037)
    check(32, solves, "it NPT=32 n=257 m=131 accumulated tau", force_variant)
