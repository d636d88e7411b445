"""Paths whose normals are solved for, shared by the steered-path tests and
tests/golden/make_golden_steered.py.

Random draws almost never reach the ramps of the smoothed barrier test, the
quadratic of the smoothed payoff, the spot floor or a decision edge.  A row of
normals that puts a step's spot on a chosen target does: the log-spot at the
end of step k is log_s0 + sum_j (drift_j + diff_j z_j), so

    z_k = (ln target_k - log_s0 - c_{k-1} - drift_k) / diff_k,

with c carried by the engine's own separately rounded multiply and add.  The
single-barrier engine multiplies spots instead (and subtracts dividends), so
there z_k = (ln(target_k / s_{k-1}) - drift_k) / diff_k with s carried by the
engine's operations, and a target is the spot before the step's dividend.

The menus below are lists of (label, targets) rows; a label's first word is
its group: "ramp", "frac", "payoff", "all" for the smoothed menu, "edge",
"strike", "rebreach" for the exact one, "floor", "straddle" for the
single-barrier extras.  The census functions recount, under the host engines'
own arithmetic, which branch every monitored and terminal spot takes.
"""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F7 = (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5)
EDGE_OFFSET = 1e-8   # exact-mode landings sit at level * (1 +- this)
EDGE = 1e-9          # and every exact decision stays off its edge by more than this


def load_cases():
    with open(os.path.join(GOLDEN, "steered_cases.json"), encoding="utf-8") as f:
        return json.load(f)


def load_arrays():
    with np.load(os.path.join(GOLDEN, "steered_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def group_of(label):
    return label.split(" ", 1)[0]


# ---------------------------------------------------------------------------
# BGK engine: log-spot as a running sum
# ---------------------------------------------------------------------------
def steer(log_s0, drift, diff, targets):
    """One row of normals: step k ends on targets[k]; None gives z = 0."""
    z = np.zeros(len(targets))
    c = 0.0
    for k, target in enumerate(targets):
        if target is not None:
            z[k] = (math.log(target) - log_s0 - c - float(drift[k])) / float(diff[k])
        c = c + (float(drift[k]) + float(diff[k]) * float(z[k]))
    return z


def landing(log_s0, drift, diff, Z):
    """Spots [n, n_steps] at each step's end as the fp64 engines see them."""
    Z = np.atleast_2d(Z)
    return np.exp(log_s0 + np.cumsum(np.asarray(drift)[None, :] + np.asarray(diff)[None, :] * Z,
                                     axis=1))


def steer_rows(log_s0, drift, diff, rows):
    return np.stack([steer(log_s0, drift, diff, t) for _, t in rows])


class _Rows:
    """Rows of targets on a grid whose monitored steps default to `mid`."""

    def __init__(self, monitor, mid):
        self.monitor = [bool(m) for m in monitor]
        self.n = len(self.monitor)
        # landings go on monitored steps before the last one: the last step
        # carries the terminal target
        self.mon = [k for k in range(self.n - 1) if self.monitor[k]]
        assert len(self.mon) >= 5, "the menus need five monitored steps before the last"
        self.mid = mid
        self.rows = []

    def add(self, label, landings, terminal):
        t = [self.mid if self.monitor[k] else None for k in range(self.n)]
        for k, s in landings.items():
            t[k] = s
        t[-1] = terminal
        self.rows.append((label, t))


def _mid(Hu, Hd, K):
    if Hu is not None and Hd is not None:
        return 0.5 * (Hu + Hd)
    return Hu - 20.0 if Hu is not None else Hd + 20.0


def _itm(K, put):
    return K - 6.0 if put else K + 12.0


def bgk_menu(Hu, Hd, K, eps_b, eps_p, monitor, put):
    """Smoothed menu.  A side's breach amount a in (0, 1) is the landing
    Hu + (2a - 1) eps_b (up) or Hd - (2a - 1) eps_b (down); "full" is one unit
    beyond the level."""
    R = _Rows(monitor, _mid(Hu, Hd, K))
    m = R.mon
    itm = _itm(K, put)
    sides = [(n, H, sg) for n, H, sg in (("up", Hu, 1.0), ("down", Hd, -1.0)) if H is not None]

    def part(H, sg, a):
        return H + sg * (2.0 * a - 1.0) * eps_b

    for name, H, sg in sides:
        for where, k in (("first", m[0]), ("last", m[-1])):
            for f in F7:
                R.add(f"ramp {name} {where} f={f:+.1f}", {k: H + f * eps_b}, itm)
    for name, H, sg in sides:
        full = H + sg * 1.0
        R.add(f"frac {name} 0.25+0.5", {m[0]: part(H, sg, 0.25), m[2]: part(H, sg, 0.5)}, itm)
        R.add(f"frac {name} 0.25+0.5+0.5 clamp",
              {m[0]: part(H, sg, 0.25), m[2]: part(H, sg, 0.5), m[4]: part(H, sg, 0.5)}, itm)
        R.add(f"frac {name} 0.5+full", {m[1]: part(H, sg, 0.5), m[3]: full}, itm)
        R.add(f"frac {name} full+0.5", {m[1]: full, m[3]: part(H, sg, 0.5)}, itm)
        R.add(f"frac {name} 0.75+0.75 clamp",
              {m[0]: part(H, sg, 0.75), m[4]: part(H, sg, 0.75)}, itm)
    if len(sides) == 2:
        R.add("frac both up 0.25 down 0.5",
              {m[1]: part(Hu, 1.0, 0.25), m[3]: part(Hd, -1.0, 0.5)}, itm)
    sgn = -1.0 if put else 1.0
    for f in F7:
        R.add(f"payoff alive=1 f={f:+.1f}", {}, K + sgn * f * eps_p)
        for name, H, sg in sides:
            R.add(f"payoff alive=0.5 {name} f={f:+.1f}", {m[2]: part(H, sg, 0.5)},
                  K + sgn * f * eps_p)
    if len(sides) == 2:
        for f in F7:
            R.add(f"all f={f:+.1f}", {m[1]: Hu + f * eps_b, m[3]: Hd - f * eps_b},
                  K + sgn * f * eps_p)
    return R.rows


def exact_menu(levels, K, monitor, put, mid=None):
    """Exact-mode menu.  levels: (name, H, sign) with sign +1 for a level
    breached from below (up) and -1 for one breached from above (down)."""
    names = {n: H for n, H, _ in levels}
    R = _Rows(monitor, mid if mid is not None else _mid(names.get("up"), names.get("down"), K))
    m = R.mon
    itm = _itm(K, put)
    for name, H, sg in levels:
        for where, k in (("first", m[0]), ("middle", m[len(m) // 2]), ("last", m[-1])):
            for side in (-1.0, 1.0):
                R.add(f"edge {name} {where} {side:+.0f}", {k: H * (1.0 + side * EDGE_OFFSET)}, itm)
    for side in (-1.0, 1.0):
        R.add(f"strike {side:+.0f}", {}, K * (1.0 + side * EDGE_OFFSET))
    for name, H, sg in levels:
        R.add(f"rebreach {name}", {m[0]: H + sg * 1.0, m[3]: H + sg * 2.0}, itm)
        R.add(f"rebreach {name} late first", {m[2]: H + sg * 1.0, m[4]: H + sg * 2.0}, itm)
    if len(levels) == 2:
        (_, Ha, sa), (_, Hb, sb) = levels
        R.add("rebreach up then down", {m[1]: Ha + sa * 1.0, m[4]: Hb + sb * 1.0}, itm)
    return R.rows


def targets_of(rows):
    """(row, step, target) of every steered step."""
    return [(r, k, t) for r, (_, tg) in enumerate(rows) for k, t in enumerate(tg) if t is not None]


def bgk_census(plan, Z):
    """Branch counts of the rows Z [n, n_steps] (both signs already stacked)
    under the host engine's arithmetic (bgk_barrier.host_paths)."""
    from finite_difference_amd import capi
    P, S = plan.params, plan.step
    Hu, Hd, K = (float(P[k]) for k in (capi.BGK_P_UPPER, capi.BGK_P_LOWER, capi.BGK_P_STRIKE))
    eb, ep = float(P[capi.BGK_P_EPS_BARRIER]), float(P[capi.BGK_P_EPS_PAYOFF])
    R = float(P[capi.BGK_P_REBATE])
    sides = int(plan.flags[capi.BGK_F_SIDES])
    mode = int(plan.flags[capi.BGK_F_REBATE_MODE])
    spots = landing(P[capi.BGK_P_LOG_SPOT], S[:, capi.BGK_S_DRIFT], S[:, capi.BGK_S_DIFF], Z)
    n = spots.shape[0]
    out = {}
    # f = +-1 rows land within 1e-13 of a band edge: a band of half-width
    # 0.99 e leaves them out of "inside" and 1.01 e out of "below" / "above"
    inner, outer = 0.99, 1.01
    breached = np.zeros(n)
    rebate_pv = np.zeros(n)
    newly = dict(frac_first=np.zeros(n, bool), partial_after=np.zeros(n, bool),
                 full_after=np.zeros(n, bool))
    for name, bit, H in (("up", 1, Hu), ("down", 2, Hd)):
        if sides & bit:
            out[name] = dict(below=0, inside=0, above=0)
    for k in np.nonzero(S[:, capi.BGK_S_MONITOR])[0]:
        s = spots[:, k]
        event = np.zeros(n)
        for name, bit, H in (("up", 1, Hu), ("down", 2, Hd)):
            if not sides & bit:
                continue
            out[name]["below"] += int(np.count_nonzero(s < H - outer * eb))
            out[name]["inside"] += int(np.count_nonzero(np.abs(s - H) < inner * eb))
            out[name]["above"] += int(np.count_nonzero(s > H + outer * eb))
            if name == "up":
                e = np.where(s < H - eb, 0.0, np.where(s > H + eb, 1.0,
                                                        0.5 + (s - H) / (2.0 * eb)))
            else:
                e = np.where(s < H - eb, 1.0, np.where(s > H + eb, 0.0,
                                                        0.5 + (H - s) / (2.0 * eb)))
            event = np.maximum(event, e)
        if mode == 2:
            had = rebate_pv > 0.0
            newly["frac_first"] |= (event > 0.0) & (event < 1.0) & ~had
            newly["partial_after"] |= (event > 0.0) & (event < 1.0) & had
            newly["full_after"] |= (event == 1.0) & had
            rebate_pv += np.maximum(0.0, event - had) * R * float(S[k, capi.BGK_S_DF_END])
        breached += event
    alive = np.clip(1.0 - breached, 0.0, 1.0)
    out["alive_1"] = int(np.count_nonzero(alive == 1.0))
    out["alive_frac"] = int(np.count_nonzero((alive > 0.0) & (alive < 1.0)))
    out["alive_0_clamped"] = int(np.count_nonzero((breached > 1.0) & (breached < 2.0)))
    d = spots[:, -1] - K
    d = -d if plan.flags[capi.BGK_F_PUT] else d
    out["payoff_below"] = int(np.count_nonzero(d < -outer * ep))
    out["payoff_inside"] = int(np.count_nonzero(np.abs(d) < inner * ep))
    out["payoff_above"] = int(np.count_nonzero(d > outer * ep))
    if mode == 2:
        out["newly"] = {k: int(np.count_nonzero(v)) for k, v in newly.items()}
    return out


def bgk_edge_gap(plan, Z):
    """Smallest relative distance of an exact-mode decision from its edge."""
    from finite_difference_amd import capi
    P, S = plan.params, plan.step
    spots = landing(P[capi.BGK_P_LOG_SPOT], S[:, capi.BGK_S_DRIFT], S[:, capi.BGK_S_DIFF], Z)
    sides = int(plan.flags[capi.BGK_F_SIDES])
    gap = np.inf
    if P[capi.BGK_P_EPS_BARRIER] == 0.0:
        for k in np.nonzero(S[:, capi.BGK_S_MONITOR])[0]:
            for bit, lv in ((1, P[capi.BGK_P_UPPER]), (2, P[capi.BGK_P_LOWER])):
                if sides & bit:
                    gap = min(gap, float(np.min(np.abs(spots[:, k] - lv))) / lv)
    if P[capi.BGK_P_EPS_PAYOFF] == 0.0:
        K = P[capi.BGK_P_STRIKE]
        gap = min(gap, float(np.min(np.abs(spots[:, -1] - K))) / K)
    return gap


# ---------------------------------------------------------------------------
# single-barrier engine: a product of exponentials, cash dividends, a floor
# ---------------------------------------------------------------------------
def mc_walk(contract, Z):
    """The host engine's spots, step by step: pre [n, n_steps] after the
    exponential, tested (the spot the monitor sees), post (after the step's
    dividend), clamped (the floor was the larger argument)."""
    from finite_difference_amd import capi
    P, F, S = contract.params, contract.flags, contract.step
    Z = np.atleast_2d(Z)
    n, n_steps = Z.shape
    floor = float(P[capi.MC_P_FLOOR])
    div_first = bool(F[capi.MC_F_DIV_FIRST])
    s = np.full(n, float(P[capi.MC_P_SPOT]))
    pre, tested, post = (np.empty((n, n_steps)) for _ in range(3))
    clamped = np.zeros((n, n_steps), bool)
    for i in range(n_steps):
        s = s * np.exp(S[i, capi.MC_S_DRIFT] + S[i, capi.MC_S_DIFF] * Z[:, i])
        pre[:, i] = s
        div = float(S[i, capi.MC_S_DIV])
        if div != 0.0:
            clamped[:, i] = s - div < floor
            after = np.maximum(s - div, floor)
        else:
            after = s
        tested[:, i] = after if div_first else s
        s = after
        post[:, i] = s
    return pre, tested, post, clamped


def steer_mc(contract, targets):
    """One row of normals for the single-barrier engine: targets[k] is the
    spot after step k's exponential and before its dividend."""
    from finite_difference_amd import capi
    P, S = contract.params, contract.step
    floor = float(P[capi.MC_P_FLOOR])
    s = float(P[capi.MC_P_SPOT])
    z = np.zeros(len(targets))
    for k, target in enumerate(targets):
        drift, diff, div = (float(S[k, j]) for j in (capi.MC_S_DRIFT, capi.MC_S_DIFF,
                                                     capi.MC_S_DIV))
        if target is not None:
            z[k] = (math.log(target / s) - drift) / diff
        s = s * float(np.exp(drift + diff * z[k]))
        if div != 0.0:
            s = max(s - div, floor)
    return z


def steer_mc_rows(contract, rows):
    return np.stack([steer_mc(contract, t) for _, t in rows])


def mc_extras_menu(contract, kind_menu):
    """Rows of the single-barrier extras on the contract's own grid.
    kind_menu "floor": the spot before the dividend D at floor + 1.0 and at
    floor + D + 0.1 (with D = 1.5 and floor 225: 226.0, clamped to 225, and
    226.6, left at 225.1), each to three terminal spots, and four rows that
    run on z = 0 after the jump, so that the clamped spot itself is carried to
    the payoff.  Where the contract has a down threshold between the floor
    and floor + 0.1 the clamped spot is breached on the same step and the
    unclamped one is not.  "straddle": the spot before a monitored dividend at
    threshold + D/4, D/2, 3D/4, so that the spots before and after the jump
    sit on either side of the threshold, and two rows on which both orders
    agree."""
    from finite_difference_amd import capi
    P, S = contract.params, contract.step
    n = contract.n_steps
    divs = [k for k in range(n) if S[k, capi.MC_S_DIV] != 0.0]
    assert len(divs) == 1
    kd = divs[0]
    D = float(S[kd, capi.MC_S_DIV])
    thr, floor = float(P[capi.MC_P_THRESHOLD]), float(P[capi.MC_P_FLOOR])
    K = float(P[capi.MC_P_STRIKE])
    rows = []

    def add(label, pre_div, terminal, before=230.0):
        t = [before if S[k, capi.MC_S_MONITOR] != 0.0 else None for k in range(n)]
        t[kd] = pre_div
        t[-1] = terminal
        rows.append((label, t))

    if kind_menu == "floor":
        for term in (K + 12.0, K + 3.0, K - 6.0):
            add(f"floor active pre={floor + 1.0:.1f} T={term:.0f}", floor + 1.0, term)
            add(f"floor inactive pre={floor + D + 0.1:.1f} T={term:.0f}", floor + D + 0.1, term)
        # z = 0 to the end: the terminal spot is the clamped one carried forward
        for pre_div in (floor + 1.0, floor + 0.2, floor + D + 0.1, floor + D + 1.0):
            t = [230.0 if S[k, capi.MC_S_MONITOR] != 0.0 and k < kd else None for k in range(n)]
            t[kd] = pre_div
            rows.append((f"floor carried pre={pre_div:.1f}", t))
    elif kind_menu == "straddle":
        for off in (0.25 * D, 0.5 * D, 0.75 * D):
            for term in (K + 12.0, K - 6.0):
                add(f"straddle pre=thr+{off:.3f} T={term:.0f}", thr + off, term,
                    before=thr + 8.0 if contract.flags[capi.MC_F_KIND] in (1, 3) else thr - 8.0)
        for off in (-0.5, D + 0.5):     # both orders agree: breached / not, both sides
            add(f"straddle agree pre=thr{off:+.1f}", thr + off, K + 12.0,
                before=thr + 8.0 if contract.flags[capi.MC_F_KIND] in (1, 3) else thr - 8.0)
    else:
        raise ValueError(kind_menu)
    return rows


def mc_census(contract, Z):
    """Branch counts of the rows Z for the single-barrier engine."""
    from finite_difference_amd import capi
    P, F, S = contract.params, contract.flags, contract.step
    pre, tested, post, clamped = mc_walk(contract, Z)
    kind = int(F[capi.MC_F_KIND])
    thr = float(P[capi.MC_P_THRESHOLD])
    has_div = S[:, capi.MC_S_DIV] != 0.0
    mon = S[:, capi.MC_S_MONITOR] != 0.0
    out = dict(floor_active=int(np.count_nonzero(clamped.any(axis=1))),
               floor_inactive=int(np.count_nonzero((~clamped[:, has_div]).any(axis=1)))
               if has_div.any() else 0, order_changes=0, rebreach=0)
    if kind == 0:
        return out

    def hit(s):
        return s <= thr if kind in (1, 3) else s >= thr
    both = has_div & mon
    if both.any():
        k = int(np.nonzero(both)[0][0])
        earlier = (hit(tested) & mon[None, :])[:, :k].any(axis=1)
        out["order_changes"] = int(np.count_nonzero((hit(pre[:, k]) != hit(post[:, k]))
                                                    & ~earlier))
    h = hit(tested[:, mon])
    for row in h:
        idx = np.nonzero(row)[0]
        if len(idx) >= 2 and not row[idx[0]:idx[-1]].all():
            out["rebreach"] += 1
    return out


def mc_edge_gap(contract, Z):
    """Smallest relative distance of a tested spot from the threshold and of a
    terminal spot from the strike."""
    from finite_difference_amd import capi
    P, F, S = contract.params, contract.flags, contract.step
    _, tested, post, _ = mc_walk(contract, Z)
    K = float(P[capi.MC_P_STRIKE])
    gap = float(np.min(np.abs(post[:, -1] - K))) / K
    if int(F[capi.MC_F_KIND]) != 0:
        thr = float(P[capi.MC_P_THRESHOLD])
        mon = S[:, capi.MC_S_MONITOR] != 0.0
        gap = min(gap, float(np.min(np.abs(tested[:, mon] - thr))) / thr)
    return gap
