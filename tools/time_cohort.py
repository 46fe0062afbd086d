"""Times a cohort registered to one template (newmsm_amd/cohort.py) in one process and one session:

    (a) the way without it: S run_multiresolution calls one after another on one context, no reference cache;
    (b) run_cohort with one worker (the reference side of the feature preparation prepared once);
    (c) run_cohort with 2, 4 and 8 workers (each its own context and stream).

    python tools/time_cohort.py [--subjects 16] [--runs 3] [--workers 1,2,4,8] [--commit ID] [--out profiles/cohort_time.json]

S synthetic subjects on ico6 with D = 2 against one ico6 reference, the MSMSulc-shaped schedule of tools/time_registration.py (data grids ico4/5/6,
control grids ico2/3/4, sigma 4/2/1, three iterations, the Monte Carlo optimiser).  After one registration that warms the process the legs run in turn,
--runs rounds of them; the fastest run of a leg is its warm figure, all runs are listed.  A cohort leg includes the creation of its workers' contexts.
Reported per leg: wall time, wall time per subject, and the digest of every subject's sphere.reg and transformed data -- the legs computed the same
bits or the figures mean nothing.  The reference-side preparation (level_features of the reference data at the three levels) is timed on its own,
warm, and given as a share of leg (a)'s time per subject.

It also times, as they stand: msm_abs_summary over the S2 x 2 x V values of S2 = 64 distortion maps beside dedrift.distortion_summary (numpy on the
host) on the same maps, and msm_surface_distortion for those 64 copies in one call beside the only route to the same maps there was before it
(Dedrift.accumulate / finish / correct, which also warps and resamples: the whole calls are timed, not the distortion kernel inside them).
Prints one JSON line; --out also writes it to a file."""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import cohort, dedrift, registration, synthetic  # noqa: E402

LEVELS = [dict(data_order=4, cp_order=2, sigma_in=4.0, sigma_ref=4.0), dict(data_order=5, cp_order=3, sigma_in=2.0, sigma_ref=2.0),
          dict(data_order=6, cp_order=4, sigma_in=1.0, sigma_ref=1.0)]
RUN_KW = dict(varnorm=True, iters=3, mciters=50, mcparam=0.8, seed=1, kind="multivariate", cost_params=dict(lambda_=0.1))


def inputs(S, D=2):
    xyz, tri = M.make_mesh_from_icosa(6)
    ref = synthetic.features(xyz, D, 7)
    subjects = [dict(xyz=xyz, tri=tri, data=synthetic.features(synthetic.known_warp(xyz, seed=9 + s, rot_deg=3.0, amp=2.0), D, 7)) for s in range(S)]
    return xyz, tri, ref, subjects


def digest(results):
    h = hashlib.sha256()
    for r in results:
        h.update(np.ascontiguousarray(r["sphere_reg"]).tobytes())
        h.update(np.ascontiguousarray(r["transformed"]).tobytes())
    return h.hexdigest()[:16]


def one_after_another(ctx, subjects, xyz, tri, ref):
    ops = registration.ProductOps(ctx)
    return [cohort.register_subject(ops, sub, xyz, tri, ref, LEVELS, **RUN_KW) for sub in subjects]


def reference_preparation_ms(ctx, xyz, tri, ref, runs=5):
    """level_features of the reference data at the three levels, as every registration of leg (a) runs it"""
    ops = registration.ProductOps(ctx)
    ref_mesh = ops.mesh(xyz, tri)
    timed = lambda name, fn, *a: fn(*a)  # noqa: E731
    out = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        for lv in LEVELS:
            ico = ops.mesh(*ops.icosphere(lv["data_order"]))
            registration.level_features(ops, timed, ref_mesh, ref, ico, lv["sigma_ref"], True, "ref")
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out[1:]))


def median_ms(fn, runs, warmup=2):
    t = []
    for k in range(warmup + runs):
        t0 = time.perf_counter()
        out = fn()
        if k >= warmup:
            t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), out


def kernels(ctx, S2, runs):
    """the two entry points at S2 copies of ico6 beside what did the same work before them"""
    xyz, tri = M.make_mesh_from_icosa(6)
    finals = np.stack([synthetic.known_warp(xyz, seed=100 + s, rot_deg=2.0, amp=1.5) for s in range(S2)])
    t_dist, maps = median_ms(lambda: M.surface_distortion(ctx, xyz, tri, finals), runs)
    t_one, _ = median_ms(lambda: M.surface_distortion(ctx, xyz, tri, finals[0]), runs)

    def dedrift_route():  # accumulate, finish, correct: the calls that returned distortion maps before msm_surface_distortion
        tmpl = M.Mesh(ctx, xyz, tri)
        d = dedrift.Dedrift(ctx, tmpl, S2)
        meshes = [M.Mesh(ctx, finals[s], tri) for s in range(S2)]
        for m in meshes:
            d.accumulate(m, xyz)
        d.finish()
        t0 = time.perf_counter()
        out = [d.correct(s, meshes[s], xyz, np.zeros((1, len(xyz))))[2] for s in range(S2)]
        dt = (time.perf_counter() - t0) * 1e3
        for m in meshes:
            m.close()
        d.close()
        tmpl.close()
        return dt, out

    correct_ms = float(np.median([dedrift_route()[0] for _ in range(3)][1:]))
    values = maps.ravel()
    t_sum, got = median_ms(lambda: M.abs_summary(ctx, values, (95.0, 98.0)), runs)

    def tool_summary():
        a = M.abs_summary(ctx, np.ascontiguousarray(maps[:, 0]).ravel(), (95.0, 98.0))
        s = M.abs_summary(ctx, np.ascontiguousarray(maps[:, 1]).ravel())
        return a, s

    t_tool, (ga, gs) = median_ms(tool_summary, runs)
    t_np, want = median_ms(lambda: dedrift.distortion_summary(list(maps)), runs)
    exact = (ga[1] == want["areal_max"] and ga[2][0] == want["areal_95"] and ga[2][1] == want["areal_98"] and gs[1] == want["shape_max"])
    return dict(copies=S2, vertices=len(xyz), values=int(values.size),
                surface_distortion_ms=dict(one_call_all_copies=t_dist, one_call_one_copy=t_one,
                                           dedrift_correct_calls_same_copies=correct_ms,
                                           note="the dedrift calls also warp and resample every copy; whole calls timed on the host clock, not the distortion kernel alone"),
                abs_summary_ms=dict(one_call_all_values_two_percentiles=t_sum, two_calls_as_cohort_files=t_tool, numpy_distortion_summary=t_np,
                                    max_and_percentiles_equal_numpy=bool(exact),
                                    mean_relative_difference=float(abs(ga[0] - want["areal_mean"]) / want["areal_mean"])))


def main(argv):
    ap = argparse.ArgumentParser(prog="time_cohort.py")
    ap.add_argument("--subjects", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workers", default="1,2,4,8")
    ap.add_argument("--kernel-copies", type=int, default=64)
    ap.add_argument("--kernel-runs", type=int, default=10)
    ap.add_argument("--commit", default="", help="the commit the figures are taken over (recorded in the output)")
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    if M.device_count() < 1:
        raise SystemExit("time_cohort.py: no GPU visible; nothing is measured without one")
    S = a.subjects
    xyz, tri, ref, subjects = inputs(S)
    ctx = M.Context(0)
    one_after_another(ctx, subjects[:1], xyz, tri, ref)  # library load, allocations
    legs, digests, walls = {}, {}, {}
    plan = [("a_one_after_another", lambda: one_after_another(ctx, subjects, xyz, tri, ref))]
    for w in [int(x) for x in a.workers.split(",")]:
        plan.append(("cohort_workers_%d" % w, lambda w=w: cohort.run_cohort(cohort.product_ops(0), subjects, xyz, tri, ref, LEVELS, workers=w, **RUN_KW)))
    for _ in range(a.runs):  # the legs alternate: a drift of the session over the run touches all of them alike
        for name, fn in plan:
            t0 = time.perf_counter()
            res = fn()
            walls.setdefault(name, []).append(time.perf_counter() - t0)
            digests.setdefault(name, set()).add(digest(res))
    for name, w in walls.items():
        legs[name] = dict(wall_s=[round(x, 4) for x in w], warm_wall_s=round(min(w), 4), warm_per_subject_s=round(min(w) / S, 4))
    all_digests = set().union(*digests.values())
    ref_ms = reference_preparation_ms(ctx, xyz, tri, ref)
    per_a = legs["a_one_after_another"]["warm_per_subject_s"]
    cohort_legs = {k: v for k, v in legs.items() if k.startswith("cohort_")}
    fastest = min(cohort_legs, key=lambda k: cohort_legs[k]["warm_wall_s"])
    line = dict(tool="time_cohort", date=time.strftime("%Y-%m-%d"), commit=a.commit, subjects=S, vertices=len(xyz), rows=2,
                levels=[(lv["data_order"], lv["cp_order"]) for lv in LEVELS], iterations_per_level=RUN_KW["iters"], mciters=RUN_KW["mciters"], runs=a.runs,
                legs=legs, same_bits_in_every_leg=len(all_digests) == 1, digests=sorted(all_digests),
                reference_preparation_ms_per_registration=round(ref_ms, 3), reference_preparation_share_of_a=round(ref_ms / 1e3 / per_a, 4),
                fastest_cohort_leg=fastest, fastest_cohort_leg_over_a=round(cohort_legs[fastest]["warm_wall_s"] / legs["a_one_after_another"]["warm_wall_s"], 4),
                host_threads_env=os.environ.get("MSMHIP_HOST_THREADS", "unset: 16 // workers inside run_cohort"),
                kernels=kernels(ctx, a.kernel_copies, a.kernel_runs))
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    ctx.close()
    return 0 if len(all_digests) == 1 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
