"""The one-wave IT variant at 32 nodes per lane, fdcn_march<1,1,32,0>, with the
forward carry section (sub-chain join, scan stages, the carry from the lane
below, the CC[j]) issued among the links of backward pass 1: the same
instructions on the same operands in another order, so every bit of v_out is
what the kernel gave before the reordering.

Every case pins the variant (capi.force_variant), launches through
fdcn_it_batch_dev with v_out and the workspace between canary regions
(test_gpu_guard.py), B = 3 solves (a put with the sum-form lower Dirichlet
value, a call, a put with the product form), and asserts

  (a) max_j |V_gpu - V_oracle| <= 1e-10 * max(1, max_j |V_oracle|) per solve
      against the C oracle (the TOL of test_gpu_kernels.py),
  (b) both bounds of march_precision.Yardstick (the long-double march and
      its three fp64 realisations),
  (c) sha256(v_out) == tests/golden/it_carry_overlap.json, recorded from the
      parent commit's library on an MI355X by
      tests/golden/make_golden_it_carry_overlap.py.

Cases, chosen for what the fused region can break:

* 2049 nodes (64 lanes, one short: bw1l = 0 starts the last sub-chain's
  backward links) and 2050 nodes (none);
* 543 and 1405 nodes: 17 and 44 active lanes (fm_act / fmM_act drop the carry
  into the first inactive lane -- the two multipliers of the interleaved
  carry instructions);
* 130 steps with two Rannacher steps: the phase switch reloads the scan
  weights and tables at step 2, and 64-step block boundaries fall inside the
  march;
* accumulated tau from tau0 = 0.037;
* a coarse-time group (10 steps on 2049 nodes): |fm| is 0.92 to 0.97, so the
  forward scan needs 4 to 6 stages and the ds_bpermute branch between the two
  interleaved halves runs (scan_stages() below restates setup_scan's
  criterion on the CPU and the test asserts nst >= 3 for every solve; the
  Sherman-Morrison extent, which grows with the same |fm|, is printed);
* the single-trade flavour (fdcn_march<1,1,32,2>, four sub-chains, the
  plain two-sweep solve) on 2049 nodes.
"""
import hashlib
import math

import numpy as np
import pytest
import torch

import march_precision as mp
from conftest import load_golden
from finite_difference_amd import capi
from finite_difference_amd.engine import pack
from test_gpu_guard import Guarded
from test_gpu_it_subchains import batch

pytestmark = pytest.mark.gpu

TOL = 1e-10  # tests/test_gpu_kernels.py
NPT = 32
GOLDEN = "it_carry_overlap.json"

# name -> (n_nodes, n_time, flavour, sigmas, keyword arguments of american())
CASES = {
    "short_lane_2049": (2049, 64, 0, (0.25, 0.30, 0.35), {}),
    "full_lanes_2050": (2050, 64, 0, (0.25, 0.30, 0.35), {}),
    "lanes_17": (543, 64, 0, (0.25, 0.30, 0.35), {}),
    "lanes_44": (1405, 64, 0, (0.25, 0.30, 0.35), {}),
    "phase_switch_130": (2049, 130, 0, (0.25, 0.30, 0.35), dict(n_ranna=2)),
    "accumulated_tau": (257, 130, 0, (0.25, 0.30, 0.35), dict(tau_acc=True, tau0=0.037)),
    "deep_scan": (2049, 40, 0, (0.072, 0.124, 0.226, 0.44, 0.30, 0.16), {}),
    "single_trade": (2049, 64, 1, (0.25, 0.30, 0.35), {}),
}


def group(name):
    n_nodes, n_time, _, sigmas, kw = CASES[name]
    solves = []
    for i in range(0, len(sigmas), 3):  # batch(): one solve per kind
        solves += batch(n_nodes, n_time, sigmas=sigmas[i:i + 3], **kw)
    return pack(solves, list(range(len(solves))))


def scan_stages(P, theta):
    """(nst_f, nst_b) of one scenario's parameter row at `theta`: the scan
    stages whose weight exceeds 1e-18 (setup_scan in fdcn_kernels.hip), from
    fm = -A_L / r and bm = -A_U / r of the converged factors (make_phase)."""
    dt, a, c, bc = (float(P[i]) for i in (capi.P_DT, capi.P_A, capi.P_C, capi.P_BC))
    AL, AC, AU = -theta * dt * a, 1.0 - theta * dt * bc, -theta * dt * c
    r = 0.5 * (AC + math.sqrt(AC * AC - 4.0 * AL * AU))
    out = []
    for mult in (-AL / r, -AU / r):
        q, n = abs(mult) ** (NPT - 1), 0
        while n < 6 and q > 1e-18:
            q *= q
            n += 1
        out.append(n)
    return tuple(out)


def launch(g, flavour):
    """v_out [B, n_nodes] of the pinned variant through the _dev entry, the
    two buffers the march writes between canaries."""
    k_cap = capi.sm_extent(g.n_nodes, g.n_time, g.n_ranna, g.params)
    capi.force_variant(1, NPT, flavour)
    try:
        name = capi.variant_name(g.n_nodes, True, k_cap, B=g.B)
        assert name == f"fdcn_march<1,1,{NPT},{2 * flavour}>", name
        p = capi.plan(g.n_nodes, True, k_cap, n_time=g.n_time, B=g.B)
        dev = torch.device("cuda", 0)
        P = torch.from_numpy(g.params).to(dev)
        I = torch.from_numpy(g.iparams).to(dev)
        V0 = torch.from_numpy(g.v_init).to(dev)
        F = torch.from_numpy(g.payoff).to(dev)
        out = Guarded(g.B * g.n_nodes, dev)
        ws_bytes = p["ws_bytes_per_scen"] * g.B
        assert ws_bytes % 8 == 0
        ws = Guarded(ws_bytes // 8, dev)
        capi.it_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, P.data_ptr(), I.data_ptr(),
                          V0.data_ptr(), F.data_ptr(), out.ptr, k_cap, ws.ptr, ws_bytes,
                          torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        capi.force_variant(0)
    assert out.guards_intact(), "a store left v_out"
    assert ws.guards_intact(), "a store left the workspace"
    return np.ascontiguousarray(out.values().reshape(g.B, g.n_nodes)), k_cap


def digest(v):
    return hashlib.sha256(np.ascontiguousarray(v, dtype="<f8").tobytes()).hexdigest()


def test_deep_scan_group_needs_three_to_six_stages():
    g = group("deep_scan")
    nst = [scan_stages(P, 0.5) for P in g.params]
    print(f"[deep_scan] (nst_f, nst_b) per solve at theta = 1/2: {nst}")
    assert all(3 <= nf <= 6 and 3 <= nb <= 6 for nf, nb in nst), nst
    assert len({nf for nf, _ in nst}) > 1, nst  # more than one depth of the branch


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    from oracle import oracle
    g = group(name)
    assert g.B <= 8 and g.n_time <= 200
    n_int = g.n_nodes - 2
    lanes = -(-n_int // NPT)
    if name in ("lanes_17", "lanes_44"):
        assert lanes == int(name.split("_")[1])
    if name == "short_lane_2049":
        assert lanes * NPT - n_int == 1
    if name == "full_lanes_2050":
        assert lanes * NPT - n_int == 0
    V, k_cap = launch(g, CASES[name][2])
    assert np.all(np.isfinite(V)), f"{name}: non-finite GPU output"
    # (a) the C oracle
    ref = oracle.it_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                          g.payoff, 4)
    rel = np.max(np.abs(V - ref), axis=1) / np.maximum(1.0, np.max(np.abs(ref), axis=1))
    print(f"[{name}] n={g.n_nodes} m={g.n_time} lanes={lanes} sm_extent={k_cap} "
          f"worst_rel_err={rel.max():.3e} sha256={digest(V)}")
    assert rel.max() <= TOL, rel
    # (b) the rounding yardstick
    mp.yardstick(g).check(V, name)
    # (c) the bits of the parent commit's kernel
    want = load_golden(GOLDEN)["cases"][name]
    assert want["shape"] == list(V.shape)
    assert digest(V) == want["sha256"], f"{name}: v_out is not bit-identical to the golden"
