"""Record the sha256 of v_out for every case of test_gpu_it_carry_overlap.py.

Runs on an MI355X, against a build of libfdcn.so from the commit BEFORE the
forward carry section moved into backward pass 1 (tools/build_ab.sh TAG REV
builds one into ab/TAG/):

  python tests/golden/make_golden_it_carry_overlap.py --lib ab/TAG/libfdcn.so

The cases, the pinning and the launch (the _dev entry between canaries) are
the test's own (imported from it), so the test compares like with like.
Each case is also held to the C oracle under the test's TOL before its digest
is written, so a broken library cannot become the golden.  Writes
it_carry_overlap.json next to this file: per case the shape of v_out and the
sha256 of its little-endian float64 bytes, plus the library's sha256.
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                     # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))    # repository root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="the parent commit's libfdcn.so")
    ap.add_argument("--out", default=os.path.join(HERE, "it_carry_overlap.json"))
    args = ap.parse_args()
    from finite_difference_amd import capi
    capi.LIB_PATH = os.path.abspath(args.lib)
    import test_gpu_it_carry_overlap as t
    from oracle import oracle
    capi.require_device()
    cases = {}
    for name in t.CASES:
        g = t.group(name)
        V, k_cap = t.launch(g, t.CASES[name][2])
        ref = oracle.it_batch(g.n_nodes, g.n_time, g.n_ranna, g.params, g.iparams, g.v_init,
                              g.payoff, 4)
        rel = np.max(np.abs(V - ref), axis=1) / np.maximum(1.0, np.max(np.abs(ref), axis=1))
        assert np.all(np.isfinite(V)) and rel.max() <= t.TOL, (name, rel)
        V2, _ = t.launch(g, t.CASES[name][2])
        assert np.array_equal(V, V2), f"{name}: two launches of one library differ"
        cases[name] = {"shape": list(V.shape), "sha256": t.digest(V)}
        print(f"{name}: sm_extent={k_cap} rel_err={rel.max():.3e} {cases[name]['sha256']}")
    with open(capi.LIB_PATH, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()
    with open(args.out, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_it_carry_overlap.py",
                   "library_sha256": lib_sha, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
