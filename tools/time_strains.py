"""tools/time_strains.py [--orders 6 7] [--repeats N] -- the strain map of an aMSM run (msm_calculate_strains) on the MI355X (GPU only): a synthetic
anatomy (newmsm_amd/synthetic.py) on icosphere(order) against the same anatomy after a known warp of the sphere, fit radius 2 as newmsm uses it.
Prints one JSON line per order: the mesh upload, the first call and the warm calls (a host clock around each call, which returns complete), the
neighbourhood sizes and the final radii.  The per-kernel times come from the same run under `rocprofv3 --kernel-trace --stats`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import newmsm_amd as M  # noqa: E402
from newmsm_amd import synthetic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--orders", type=int, nargs="+", default=[6, 7])
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    ctx = M.Context(0)
    for order in a.orders:
        xyz, tri = M.make_mesh_from_icosa(order)
        orig = synthetic.anatomy(xyz, seed=1)
        final = synthetic.anatomy(synthetic.known_warp(xyz, seed=6, rot_deg=2.0, amp=1.5), seed=1)
        ctx.synchronize()
        t0 = time.perf_counter()
        mesh = M.Mesh(ctx, orig, tri)
        t1 = time.perf_counter()
        strains, kept, radius = M.calculate_strains(mesh, final, 2.0, with_neighbourhoods=True)
        t2 = time.perf_counter()
        warm = []
        for _ in range(a.repeats):
            ctx.synchronize()
            s0 = time.perf_counter()
            M.calculate_strains(mesh, final, 2.0)
            warm.append((time.perf_counter() - s0) * 1e3)
        mesh.close()
        print(json.dumps(dict(order=order, V=len(orig), T=len(tri), mesh_create_ms=(t1 - t0) * 1e3, first_call_ms=(t2 - t1) * 1e3,
                              warm_call_ms_median=statistics.median(warm), warm_call_ms_min=min(warm), warm_call_ms_all=[round(w, 3) for w in warm],
                              kept_mean=float(kept.mean()), kept_max=int(kept.max()), radius_max=float(radius.max()),
                              radius_grown=int(np.count_nonzero(radius > 2.0)), max_stretch=float(strains[0].max()), min_stretch=float(strains[1].min()))),
              flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
