#!/usr/bin/env python
"""Records the unary tables of tests/unary_rows_cases.py, as the loaded library computes them on GPU 0 behind the ray sampler, into an .npz -- the fixture
tests/golden/unary_rows_parent.npz when MSM_LIB_PATH names the library of the commit before k_unary_reduce_rows:

    MSM_LIB_PATH=/path/to/parent/libmsmhip.so python tools/record_unary_tables.py tests/golden/unary_rows_parent.npz

With a second .npz it then compares what it recorded with that file and exits 1 on the first table that differs in a bit."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ.setdefault("MSMHIP_RAYTABLE", "sync")  # as tests/conftest.py: the direction table on first use


def main(argv):
    if len(argv) not in (2, 3):
        print(__doc__)
        return 2
    import newmsm_amd as M
    import unary_rows_cases as R

    ctx = M.Context(0)
    tables = {}
    for name, sim, weighting in R.all_tables():
        cf = R.product(ctx, name, sim, weighting)
        U = cf.computeUnaryCosts().copy()
        assert cf.unary_launch()["sampler"] == "rays" and np.isfinite(U).all()
        tables[R.key(name, sim, weighting)] = U
        print("%-20s %s form %s" % (R.key(name, sim, weighting), U.shape, cf.routes()["unary_form"]))
    np.savez_compressed(argv[1], **tables)
    print("wrote %s: %d tables, %d bytes" % (argv[1], len(tables), os.path.getsize(argv[1])))
    if len(argv) == 3:
        with np.load(argv[2]) as z:
            for k, U in tables.items():
                if not np.array_equal(U, z[k]):
                    print("DIFFERS: %s, max |difference| %.3e" % (k, np.max(np.abs(U - z[k]))))
                    return 1
        print("bit-equal to %s" % argv[2])
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
