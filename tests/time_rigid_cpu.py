"""tests/time_rigid_cpu.py -- CPU cost of the literal restatement of Rigid_cost_function (tests/rigid_literal.py): one evaluation in the literal
mode (per-vertex Neighbourhood, sparse similarity map) and in the fast mode, and a whole run in the fast mode, bounded in size and iterations.
A script, run by hand (it lives under tests/ because it uses the oracle):

    python tests/time_rigid_cpu.py [order [iters]]  ->  one JSON line (defaults: ico4, 5 iterations per loop)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import rigid_literal as RL  # noqa: E402
from newmsm_amd import synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    order = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    iters = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    xyz, tri = O.icosphere(order)
    ref = synthetic.features(xyz, 1, 7)
    src = synthetic.features(synthetic.known_warp(xyz, seed=9, rot_deg=4.0, amp=1.0), 1, 7)
    out = dict(order=order, V=len(xyz), iters=iters)
    for fast in (False, True):
        t0 = time.perf_counter()
        r = RL.RigidLiteral(xyz, tri, src, ref, 2, fast=fast).initialise()
        t1 = time.perf_counter()
        r.rigid_cost_mesh(0.0, 0.0, 0.0)
        t2 = time.perf_counter()
        key = "fast" if fast else "literal"
        out[key + "_initialise_s"] = t1 - t0
        out[key + "_evaluation_s"] = t2 - t1
    r = RL.RigidLiteral(xyz, tri, src, ref, 2, fast=True).initialise()
    t0 = time.perf_counter()
    _, trace, summary = r.run(iters, float(np.float32(0.01)), 0.5)
    out.update(fast_run_s=time.perf_counter() - t0, evaluations=summary["evaluations"], iterations=len(trace))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
