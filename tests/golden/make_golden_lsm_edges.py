#!/usr/bin/env python3
"""Writes tests/golden/lsm_edges.json and lsm_edges.npz: the edge-case menu of
tests/lsm_edge_cases.py evaluated by the mpmath reference of
tests/lsm_reference.py (CPU only, several minutes; reads nothing outside the
repository).

json  per case: family, n_steps, antithetic, seed, sub-runs; per contract the
      stream id found by the builder, the decision count, the number of
      decisions below 100 x their bound (the exclusions), the worst
      margin-to-bound ratio; per sub-run the valid flags, fit-path counts,
      pivot ratios, invalid-step count, smallest margin, means, the fit
      bounds' coefficients (dc, du_abs) and the branch census.  Also the
      stream ids of the 511 / 512-step launches (host-engine margin at least
      lsm_fixture.MIN_MARGIN, as golden/make_golden_lsm.py does) and the
      census maxima over the menu.
npz   per contract the engine inputs (params, flags, step, times); per
      sub-run the reference coefficients rounded to float64, the price-set
      values and stopping steps per path, the fit membership of every valid
      fit and the excluded price paths as bit masks.  fit_bound(u) is a closed
      form in u (lsm_edge_cases.FitBound), so the tests evaluate it on the fit
      paths instead of reading it per path.

Usage: python tests/golden/make_golden_lsm_edges.py [case ...]
(cases not named are kept from the existing files).
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import lsm_edge_cases as ec  # noqa: E402
import lsm_fixture as lf  # noqa: E402
import lsm_reference as lr  # noqa: E402
from finite_difference_amd import mc_american  # noqa: E402

OUT_JSON = os.path.join(HERE, "lsm_edges.json")
OUT_NPZ = os.path.join(HERE, "lsm_edges.npz")
LIMIT = 1 << 20


def long_stream_ids():
    out = {}
    for M in (511, 512):
        ids, margins = [], []
        for b, c in enumerate(ec.long_contracts(M)):
            for sid in range(b, ec.MAX_STREAM, 4):
                m = float(mc_american.host_subruns(c, [0], False, ec.LONG_SEED, sid)
                          ["margin"].min())
                if m >= lf.MIN_MARGIN:
                    break
            assert m >= lf.MIN_MARGIN, (M, b, m)
            ids.append(sid)
            margins.append(lf.finite(m))
        out[str(M)] = dict(stream_ids=ids, host_min_margin=margins)
        print("long", M, out[str(M)], flush=True)
    return out


def census_maxima(cases):
    best = {k: 0 for k in lr.CENSUS_PATH_KEYS + lr.CENSUS_STEP_KEYS}
    for doc in cases.values():
        for item in doc["items"]:
            for run in item["runs"]:
                for k, v in run["census"].items():
                    best[k] = max(best[k], max(v) if isinstance(v, list) else v)
    return best


def main():
    names = sys.argv[1:] or list(ec.MENU)
    doc = json.load(open(OUT_JSON)) if os.path.exists(OUT_JSON) else {"cases": {}}
    arrays = dict(np.load(OUT_NPZ)) if os.path.exists(OUT_NPZ) else {}
    for name in names:
        t = time.time()
        case = ec.build_case(name)
        for k in [k for k in arrays if k.startswith(name + "/")]:
            del arrays[k]
        doc["cases"][name] = ec.case_to_fixture(case, arrays)
        for it in case.items:
            print(f"{name}: stream {it.stream_id}, {it.n_decisions} decisions, "
                  f"{it.n_low_margin} below {ec.MARGIN_FACTOR:g} bounds, worst margin / bound "
                  f"{it.worst_margin_ratio:.3g}, counts {it.refs[0]['count']}, valid "
                  f"{[int(v) for v in it.refs[0]['valid']]} {it.note}", flush=True)
        print(f"{name}: {time.time() - t:.0f} s", flush=True)
    doc["cases"] = {k: doc["cases"][k] for k in ec.MENU if k in doc["cases"]}
    if not sys.argv[1:] or "long" not in doc:
        doc["long"] = long_stream_ids()
    doc["census_max"] = census_maxima(doc["cases"])
    doc["margin_factor"] = ec.MARGIN_FACTOR
    doc["exclusion_cap"] = ec.EXCLUSION_CAP
    with open(OUT_JSON, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    np.savez_compressed(OUT_NPZ, **arrays)
    for p in (OUT_JSON, OUT_NPZ):
        assert os.path.getsize(p) < LIMIT, (p, os.path.getsize(p))
        print(p, os.path.getsize(p), "bytes")
    print("census maxima:", doc["census_max"])


if __name__ == "__main__":
    main()
