"""tests/time_strains_cpu.py -- CPU cost of the restatement of calculate_strains (tests/strains_literal.py) on the inputs of tools/time_strains.py: the
fast mode at the given orders and, where it stays short, the literal O(V^2)-per-step mode.  Process CPU time, meant for one core (run it under
`taskset -c 0` with OMP_NUM_THREADS=OPENBLAS_NUM_THREADS=1).  A script, run by hand (it lives under tests/ because it uses the oracle):

    python tests/time_strains_cpu.py [order ...]  ->  one JSON line per order (defaults: ico4 ico6 ico7)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import strains_literal as SL  # noqa: E402
from newmsm_amd import synthetic  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    orders = [int(a) for a in sys.argv[1:]] or [4, 6, 7]
    for order in orders:
        xyz, tri = O.icosphere(order)
        orig = synthetic.anatomy(xyz, seed=1)
        final = synthetic.anatomy(synthetic.known_warp(xyz, seed=6, rot_deg=2.0, amp=1.5), seed=1)
        out = dict(order=order, V=len(orig), fast_cpu_s=SL.cpu_seconds(orig, tri, final))
        if order <= 4:
            t0 = time.process_time()
            SL.calculate_strains(orig, tri, final, literal=True)
            out["literal_cpu_s"] = time.process_time() - t0
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
