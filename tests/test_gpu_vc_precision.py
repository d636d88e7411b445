"""The spot-space per-row march kernels (csrc/fdcn_vc.hip) against a
long-double march of the same plan, under the rounding yardstick of
march_precision.py (max-norm and out-of-the-money tail, per solve) in place of
the fixed 1e-10 of test_spot_barrier.py / test_gpu_fuzz.py.

Inputs: vc_cases.VC_INPUTS, each of which test_vc_precision.py holds to the
leave-one-out condition on the CPU.  "pointwise" launches let the factor
kernel choose the form, "stencil" forces the stencil form on every scenario;
the variant is pinned (asserted through vc_variant_name) wherever the input
names one.  `-s` prints every launch's worst ratio = error / bound.

Measured on an MI355X (463 solves per form): worst ratios 0.75 (max-norm,
instances stencil, 13 107 nodes) and 0.85 (tail, instances pointwise, 640
nodes) against the three Thomas orderings; the fuzz group takes the sequential
restatement of the kernels' ordering as a fourth realisation (fuzz_10
pointwise: tail 1.27 without it, 0.14 with; vc_cases.KERNEL_ORDER_GROUPS).
Before the factor kernel's Newton step 33 of these 46 tests
failed, ratios up to 43.

Every launch also checks what must be exact: the Dirichlet nodes equal the
literal march's bit for bit (rows with a unit diagonal: x_0 = g_0 lo, no
arithmetic of the solve), and on a scenario whose last step is a monitor the
knocked-out nodes equal the rebate.
"""
import dataclasses

import numpy as np
import pytest
import torch

import march_precision as mp
import vc_cases as vc
from finite_difference_amd import capi

pytestmark = pytest.mark.gpu

GUARD = 8192  # doubles = 64 KiB each side
CANARY = np.int64(0x7FF4DEADBEEF5A5A)  # a signalling-NaN bit pattern no march produces


@pytest.fixture(autouse=True)
def _unpin():
    yield
    capi.vc_force_variant(0, 0, False)


def _pin(g, pin, form):
    stencil = form == "stencil"
    if pin is None:
        capi.vc_force_variant(0, 0, stencil)
    else:
        capi.vc_force_variant(pin[0], pin[1], stencil)
        assert capi.vc_variant_name(g.n_nodes, B=g.B) == f"fdcn_vc_march<{pin[0]},{pin[1]}>"
    forms = capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag)
    assert not stencil or not forms.any()
    return forms


def _host_launch(g):
    return capi.vc_batch(g.n_nodes, g.n_time, g.n_ranna, g.diag, g.bnd, g.v_init, g.iparams,
                         g.mon_step, g.mon_rebate)


def _yardstick(key, forms):
    names = mp.REALISATIONS
    if vc.uses_kernel_order(key):
        names += tuple(nm for nm, f in ((mp.KERNEL_POINTWISE, 1), (mp.KERNEL_STENCIL, 0))
                       if np.any(forms == f))
    return mp.yardstick(vc.vc_input(key), names)


def _exact_parts(g, V, ref, label):
    """Dirichlet nodes and knocked-out nodes carry no rounding."""
    unit = np.all(g.diag[:, :, 1, [0, -1]] == 1.0, axis=(1, 2))
    assert np.array_equal(V[unit][:, [0, -1]], ref[unit][:, [0, -1]]), label
    j = np.arange(g.n_nodes)
    n_ko = 0
    for b in range(g.B):
        start, cnt = g.iparams[b, capi.I_MON_START], g.iparams[b, capi.I_MON_COUNT]
        if cnt == 0 or g.n_time == 0 or g.mon_step[start + cnt - 1] != g.n_time:
            continue
        ko = (j <= g.iparams[b, capi.I_KO_LO]) | (j >= g.iparams[b, capi.I_KO_HI])
        assert np.all(V[b, ko] == g.mon_rebate[start + cnt - 1]), (label, b)
        n_ko += int(ko.sum())
    return int(unit.sum()), n_ko


def _check(key, form, launch=None):
    g = vc.vc_input(key)
    forms = _pin(g, vc.VC_INPUTS[key][1], form)
    V = (launch or _host_launch)(g)
    y = _yardstick(key, forms)
    label = f"{key} {form} forms={''.join(str(int(f)) for f in forms)} [{len(y.real)} realisations]"
    n_unit, n_ko = _exact_parts(g, V, y.real["f64"], label)
    try:
        worst = y.check(V, label)
    except AssertionError as e:  # every launch of the test is measured and printed first
        r_max, r_tail = y.ratios(V)
        worst = (float(np.max(r_max)), float(np.max(r_tail)))
        _outside.append(str(e))
    return worst, n_unit, n_ko


_outside = []


@pytest.fixture(autouse=True)
def _fresh():
    _outside.clear()


def _assert_inside():
    """After a test's last launch: no solve of any of them was outside."""
    bad = list(_outside)
    _outside.clear()
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------
# every compiled instance, pinned, between canaries
# --------------------------------------------------------------------------
class Guarded:
    """n doubles between two guard regions on the device."""

    def __init__(self, n, dev):
        self.n = n
        self.buf = torch.full((GUARD + max(n, 1) + GUARD,), int(CANARY), dtype=torch.int64,
                              device=dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD * 8

    def guards_intact(self):
        b = self.buf.cpu().numpy()
        return bool(np.all(b[:GUARD] == CANARY) and np.all(b[GUARD + max(self.n, 1):] == CANARY))

    def values(self):
        return self.buf.cpu().numpy()[GUARD:GUARD + self.n].view(np.float64)


def _guarded_launch(g):
    """fdcn_vc_batch_dev on a side stream; v_out and the workspace exactly as
    vc_plan sizes them, each between two canary regions."""
    dev = torch.device("cuda", 0)
    T = {k: torch.from_numpy(np.ascontiguousarray(getattr(g, k))).to(dev)
         for k in ("diag", "bnd", "v_init", "iparams")}
    MS = torch.from_numpy(g.mon_step if len(g.mon_step) else np.zeros(1, np.int32)).to(dev)
    MR = torch.from_numpy(g.mon_rebate if len(g.mon_rebate) else np.zeros(1)).to(dev)
    p = capi.vc_plan(g.n_nodes, B=g.B)
    ws_bytes = p["ws_bytes_per_scen"] * g.B
    assert ws_bytes == 8 * (2 * 5 * 64 * p["waves"] * p["npt"] + 20) * g.B
    out, ws = Guarded(g.B * g.n_nodes, dev), Guarded(ws_bytes // 8, dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    capi.vc_batch_dev(g.B, g.n_nodes, g.n_time, g.n_ranna, T["diag"].data_ptr(),
                      T["bnd"].data_ptr(), T["v_init"].data_ptr(), T["iparams"].data_ptr(),
                      len(g.mon_step), MS.data_ptr(), MR.data_ptr(), out.ptr, ws.ptr, ws_bytes,
                      side.cuda_stream)
    side.synchronize()
    assert out.guards_intact(), "a store left v_out"
    assert ws.guards_intact(), "a store left the workspace"
    return out.values().reshape(g.B, g.n_nodes).copy()


@pytest.mark.parametrize("form", vc.FORMS)
@pytest.mark.parametrize("w,npt", vc.KVC, ids=[f"w{w}n{n}" for w, n in vc.KVC])
def test_every_instance_between_canaries(w, npt, form):
    """All 24 instances (12 of kVc, two forms), each on n = slots + 1 (node 0
    outside the slots), n = slots and a ragged n near 0.8 slots, through
    fdcn_vc_batch_dev on a side stream: the canaries around v_out and around
    the exactly sized workspace stay bit-for-bit intact, and every node is
    inside the yardstick.  <16,16> (8 194 to 16 385 nodes) ran nowhere before:
    from the gfx950 build, stencil / pointwise: 128 / 128 VGPRs, 0 AGPRs, 784 /
    640 B a lane of scratch, 115 472 B of LDS a block (of 160 KiB), 4 waves a SIMD.
    Its global accesses: coef[k slots + 16 t + j], k < 10, t < 1 024, j < 16, so
    < 10 slots, then scal[0..19]: the 2 kNC slots + kNS doubles vc_plan sizes;
    v_init / v_out at j = 16 t + k - pad_lo only where 0 <= j < n; bnd[m + lane]
    only where < n_time; the factor kernel's slot s = i + pad_lo skipped where < 0."""
    seen = 0
    for size in ("plus1", "fit", "ragged"):
        key = f"instances_w{w}n{npt}_{size}"
        g = vc.vc_input(key)
        assert g.n_nodes == vc.instance_sizes(w, npt)[size] and 40 <= g.n_time <= 70
        _, n_unit, _ = _check(key, form, _guarded_launch)
        seen += n_unit
    assert seen == 12  # every scenario's Dirichlet nodes were compared exactly
    _assert_inside()


# --------------------------------------------------------------------------
# the other groups: one test per group and form
# --------------------------------------------------------------------------
GROUP_TESTS = ["step_shapes_w1n16", "step_shapes_w4n8", "small_grids", "long_march", "gold",
               "factor_scan", "exc_positions", "split_phases", "mixed_forms", "fuzz"]


GROUP_FORMS = [(grp, form) for grp in GROUP_TESTS for form in vc.FORMS
               if any(form in vc.VC_INPUTS[k][2] for k in vc.keys_of(grp))]


@pytest.mark.parametrize("group,form", GROUP_FORMS, ids=[f"{g}-{f}" for g, f in GROUP_FORMS])
def test_group_inside_the_yardstick(group, form):
    keys = [k for k in vc.keys_of(group) if form in vc.VC_INPUTS[k][2]]
    # fdcn_vc_batch takes the CN plan checks (n_nodes >= 5): the 3- and 4-node
    # grids go through fdcn_vc_batch_dev, which the kernels' own n >= 3 bounds
    launch = _guarded_launch if group == "small_grids" else None
    worst, n_ko = (0.0, 0.0), 0
    for key in keys:
        (w_max, w_tail), _, k = _check(key, form, launch)
        worst = (max(worst[0], w_max), max(worst[1], w_tail))
        n_ko += k
    print(f"[group {group} {form}] launches={len(keys)} worst ratio_max={worst[0]:.3f} "
          f"ratio_tail={worst[1]:.3f} knocked-out nodes compared exactly={n_ko}")
    if group.startswith(("step_shapes", "small_grids")):
        assert n_ko > 0
    _assert_inside()


def test_inputs_are_all_marched():
    marched = set(vc.keys_of("instances"))
    for group in GROUP_TESTS:
        marched |= set(vc.keys_of(group))
    assert marched == set(vc.VC_INPUTS)


# --------------------------------------------------------------------------
# independence of a scenario from its launch
# --------------------------------------------------------------------------
@pytest.mark.parametrize("w,npt,n", [(1, 16, 1025), (4, 8, 2049), (8, 16, 8193)])
def test_scenario_is_independent_of_its_launch(w, npt, n):
    """With the variant pinned, a scenario gives bitwise the same vector
    alone, first and last in a mixed-form batch of 7, and in a repeat launch
    -- a pointwise one (double-out, knocked out on every step) and a stencil
    one (three scattered exceptional rows), on the N + 1 layout."""
    g = vc.step_shapes(w, npt, n, 65, 2)
    D = g.diag.copy()
    for b in (2, 5):
        for i in (n // 8, n // 2 + 5, n - 20):
            D[b, 1, 3, i] *= 1.001
    g = dataclasses.replace(g, diag=D)
    capi.vc_force_variant(w, npt, False)
    assert capi.vc_variant_name(n, B=7) == capi.vc_variant_name(n, B=1) == f"fdcn_vc_march<{w},{npt}>"
    forms = capi.vc_forms(g.n_nodes, g.n_time, g.n_ranna, g.diag).tolist()
    assert forms == [1, 1, 0, 1, 1, 0, 1]
    for subject in (4, 2):
        others = [b for b in range(7) if b != subject]
        alone = _host_launch(vc.take(g, [subject]))[0]
        first = _host_launch(vc.take(g, [subject] + others))[0]
        last = _host_launch(vc.take(g, others + [subject]))[-1]
        again = _host_launch(vc.take(g, [subject]))[0]
        for name, v in (("first of 7", first), ("last of 7", last), ("repeat", again)):
            assert np.array_equal(alone.view(np.int64), v.view(np.int64)), (subject, name)
        # node 0 (outside the slots) and node n-1: the rebate where the last
        # step knocks them out, else the last Dirichlet value, exactly
        ko_lo, ko_hi = g.iparams[subject, capi.I_KO_LO], g.iparams[subject, capi.I_KO_HI]
        assert alone[0] == (0.5 if ko_lo >= 0 else g.bnd[subject, -1, 0])
        assert alone[-1] == (0.5 if ko_hi <= n - 1 else g.bnd[subject, -1, 1])
