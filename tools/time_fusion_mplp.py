"""Times MPLP over the binary problem of a label step on the real label steps of a level's first iteration and compares it with the
present route, the stand-in msm_fusion_icm_step: writes profiles/fusion_mplp_time.json.  A measurement, not a test: nothing here is a threshold.

    python tools/time_fusion_mplp.py [--out profiles/fusion_mplp_time.json]

Per control grid (ico4 and ico3 under ico6 data, problem.pairwise_inputs(6, cp): 19 labels, the univariate strain class with the HCP parameters) the two
label sweeps of Fusion::optimize are walked from the zero labelling along the stand-in's own trajectory (the steps a run takes today).  Per step:
  - the present route: wall clock of msm_cost_triplet_octets into the caller's mapped array and of msm_fusion_icm_step with 5 passes;
  - msm_cost_fusion_mplp_step at 5 / 10 / 30 sweeps and 8 polish passes: ms in the solve launch by HIP events (msm_fusion_mplp_gpu_stats) and the
    wall clock of the whole call (octets, gather, solve, one synchronisation);
  - the energy of the stand-in's x, of MPLP's x (10 sweeps) and MPLP's bound, in the step's own model.
Over the steps: who wins how often, the largest and the median gap to the bound.  Over the level: the wall clock of the two label sweeps with either
solve, each along its own trajectory, and msm_cost_total of the labelling each ends with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import newmsm_amd as M  # noqa: E402
from newmsm_amd import api, problem  # noqa: E402

HCP = dict(rmode=3, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)  # --shearmod --bulkmod --k_exponent --regexp of the HCP configurations (tests/helpers.py)
SWEEPS, POLISH, ICM_PASSES = (5, 10, 30), 8, 5


def step_energy(unary2, octets, triplets, x):
    x = np.asarray(x)
    idx = 4 * x[triplets[:, 0]] + 2 * x[triplets[:, 1]] + x[triplets[:, 2]]
    return float(unary2[np.arange(len(x)), x].sum() + octets[np.arange(len(triplets)), idx].sum())


def label_sweeps(cf, U, triplets, E, solve):
    """the two label sweeps from the zero labelling: solve(labeling, label) -> x; returns (labeling, steps solved, seconds)"""
    labeling = np.zeros(cf.N, dtype=np.int32)
    n = 0
    t0 = time.perf_counter()
    for label in list(range(cf.L)) * 2:
        if not np.any(labeling != label):
            continue
        x = solve(labeling, label)
        labeling = np.where((x == 1) & (labeling != label), label, labeling).astype(np.int32)
        n += 1
    return labeling, n, time.perf_counter() - t0


def measure(ctx, cp_order):
    inp = problem.pairwise_inputs(6, cp_order, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", **HCP)
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    triplets = np.ascontiguousarray(inp["triplets"], dtype=np.int32)
    U = np.array(cf.computeUnaryCosts())
    E = ctx.host_array((cf.T, 8))
    nodes = np.arange(cf.N)

    def unary2_of(labeling, label):
        return np.stack([U[labeling, nodes], U[label]], axis=1)

    def icm(labeling, label):
        return api.fusion_icm_step(unary2_of(labeling, label), cf.tripletOctets(labeling, label, E), triplets, ICM_PASSES)

    refused = [0]

    def mplp(labeling, label):
        try:
            return cf.fusion_mplp_step(labeling, label, sweeps=10, polish=POLISH).x
        except M.MsmError:  # a step whose octets are not finite (a collapsed control triangle) is refused: nothing changes
            refused[0] += 1
            return np.zeros(cf.N, dtype=np.int32)

    for solve in (icm, mplp):  # warm both routes: first launches, buffers, the plan of the triplet list
        label_sweeps(cf, U, triplets, E, solve)
    # ---- per step, along the stand-in's trajectory
    steps, skipped = [], []
    labeling = np.zeros(cf.N, dtype=np.int32)
    for sweep in range(2):
        for label in range(cf.L):
            if not np.any(labeling != label):
                continue
            t0 = time.perf_counter()
            octets = cf.tripletOctets(labeling, label, E)
            t1 = time.perf_counter()
            unary2 = unary2_of(labeling, label)
            t2 = time.perf_counter()
            x_icm = api.fusion_icm_step(unary2, octets, triplets, ICM_PASSES)
            t3 = time.perf_counter()
            octets = np.array(octets)
            rec = dict(sweep=sweep, label=label, octets_ms=1e3 * (t1 - t0), icm_ms=1e3 * (t3 - t2), solve_ms={}, call_ms={}, sweeps_run={})
            if not (np.isfinite(octets).all() and np.isfinite(unary2).all()):  # refused by the MPLP solve: counted, not timed
                rec["refused"] = True
                skipped.append(rec)
                labeling = np.where((x_icm == 1) & (labeling != label), label, labeling).astype(np.int32)
                continue
            for S in SWEEPS:
                t4 = time.perf_counter()
                r = cf.fusion_mplp_step(labeling, label, sweeps=S, polish=POLISH)
                rec["call_ms"][str(S)] = 1e3 * (time.perf_counter() - t4)
                st = api.fusion_mplp_gpu_stats(ctx)
                rec["solve_ms"][str(S)] = st["kernel_ms"]
                rec["sweeps_run"][str(S)] = st["sweeps_run"]
                if S == 10:
                    rec.update(e_zero=float(r.energies[0]), e_mplp=float(r.energy), bound=float(r.bound), passes_run=r.passes_run,
                               levels_per_sweep=st["levels_per_sweep"], launches=st["launches"])
            rec["e_icm"] = step_energy(unary2, octets, triplets, x_icm)
            steps.append(rec)
            labeling = np.where((x_icm == 1) & (labeling != label), label, labeling).astype(np.int32)
    e_icm, e_mplp, bound = (np.array([s[k] for s in steps]) for k in ("e_icm", "e_mplp", "bound"))
    scale = np.maximum(1.0, np.abs(bound))
    tie = np.abs(e_icm - e_mplp) <= 1e-9 * scale
    summary = dict(steps=len(steps), steps_refused=len(skipped), mplp_wins=int(np.sum(~tie & (e_mplp < e_icm))), icm_wins=int(np.sum(~tie & (e_icm < e_mplp))), ties=int(tie.sum()),
                   gap_mplp_max=float(np.max((e_mplp - bound) / scale)), gap_mplp_median=float(np.median((e_mplp - bound) / scale)),
                   gap_icm_max=float(np.max((e_icm - bound) / scale)), gap_icm_median=float(np.median((e_icm - bound) / scale)),
                   sum_e_icm=float(e_icm.sum()), sum_e_mplp=float(e_mplp.sum()), sum_bound=float(bound.sum()),
                   octets_ms_median=float(np.median([s["octets_ms"] for s in steps])), icm_ms_median=float(np.median([s["icm_ms"] for s in steps])),
                   solve_ms_median={str(S): float(np.median([s["solve_ms"][str(S)] for s in steps])) for S in SWEEPS},
                   call_ms_median={str(S): float(np.median([s["call_ms"][str(S)] for s in steps])) for S in SWEEPS})
    # ---- the level's two label sweeps with either solve, each along its own trajectory (the median of three)
    level = {}
    for name, solve in (("icm", icm), ("mplp", mplp)):
        refused[0] = 0
        runs = [label_sweeps(cf, U, triplets, E, solve) for _ in range(3)]
        lab = runs[0][0]
        level[name] = dict(seconds=float(np.median([r[2] for r in runs])), steps=runs[0][1], total_cost=float(cf.evaluateTotalCostSum(lab)[0]),
                           labels_in_use=int(len(np.unique(lab))), steps_refused=refused[0] // 3)
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, messages="lds" if 48 * cf.T <= 152 * 1024 else "global", summary=summary, level=level, steps=steps)
    cf.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_mplp_time.json"))
    a = ap.parse_args(argv)
    ctx = M.Context(0)
    result = dict(tool="tools/time_fusion_mplp.py", data_order=6, sweeps=list(SWEEPS), polish=POLISH, icm_passes=ICM_PASSES,
                  grids=[measure(ctx, cp) for cp in (4, 3)])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    for g in result["grids"]:
        print("ico%d" % g["cp_order"], json.dumps(g["summary"]), json.dumps(g["level"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
