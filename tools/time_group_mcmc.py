"""tools/time_group_mcmc.py [--subjects 8 64] [--reps 3] [--out profiles/group_mcmc_time.json] -- what a pass of gMSM's Monte Carlo blocks costs
(msm_group_mcmc_pass), beside one iteration of the label loop with the stand-in solve on the same group.

Per size (S = 8: ico5 data / ico3 control grid; S = 64: ico6 / ico4; D = 2, correlation, --fixnan, 19 labels), after one set-up:
  * one pass from the zero labelling, K chains of `--mciters` sweeps per block: per block the GPU milliseconds of the query build plus pair costs, of the
    segment sums, of the triplet table (HIP events) and of the sweep kernels; the pass's wall clock; the energy before and after;
  * one iteration of the fusion-shaped loop (two sweeps over the labels: msm_group_fusion_move per label step, msm_fusion_icm_step on the host): its wall
    clock and the energy of its labelling.
Both energies come from the same evaluator (the (current, current) costs of msm_group_fusion_move at the labelling: pairs, then triplets).  The two are
alternated in one process, `--reps` times; medians are reported, every repetition is kept.  Observations, not a comparison against a bar: the two loops
run different optimisers and reach different labellings."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import newmsm_amd as M  # noqa: E402
from newmsm_amd import api, problem  # noqa: E402

SHAPES = {8: (5, 3), 64: (6, 4)}


def energy(g, labeling):
    quads, octets = g.fusionMove(labeling, 0)
    return float(np.sum(quads[:, 0]) + np.sum(octets[:, 0]))


def fusion_iteration(g, pairs, triplets, nodes, icm_passes):
    labeling = np.zeros(nodes, dtype=np.int32)
    for _ in range(2):
        for label in range(g.L):
            if not np.any(labeling != label):
                continue
            quads, octets = g.fusionMove(labeling, label)
            x = api.fusion_icm_step(nodes, octets, triplets, icm_passes, quads=quads, pairs=pairs)
            labeling = np.where((x == 1) & (labeling != label), label, labeling).astype(np.int32)
    return labeling


def measure(ctx, S, reps, mciters, mcparam, chains, icm_passes, draw):
    data_order, cp_order = SHAPES[S]
    g, keep = problem.build_group(ctx, S, data_order=data_order, cp_order=cp_order, D=2, fixnan=True)
    t0 = time.perf_counter()
    g.setupCostFunction()
    setup_s = time.perf_counter() - t0
    pairs, triplets = g.getPairs(), g.getTriplets()
    nodes = g.num_nodes
    zero = np.zeros(nodes, dtype=np.int32)
    e_start = energy(g, zero)
    ctx.set_mcmc_draw(1 if draw == "gpu" else 0)
    runs = []
    for r in range(reps):
        t0 = time.perf_counter()
        lab, rec = g.mcmc_pass(zero, mcparam=mcparam, iters=mciters, seed=0, it=0, chains=chains, passes=1)
        pass_s = time.perf_counter() - t0
        e_pass = energy(g, lab)
        t0 = time.perf_counter()
        flab = fusion_iteration(g, pairs, triplets, nodes, icm_passes)
        fusion_s = time.perf_counter() - t0
        e_fusion = energy(g, flab)
        b = rec[0]
        runs.append(dict(pass_wall_ms=1e3 * pass_s, fusion_wall_ms=1e3 * fusion_s, energy_after_pass=e_pass, energy_after_fusion=e_fusion,
                         accepted_blocks=int(b[:, 2].sum()), table_energy_change=float(np.sum(b[:, 1] - b[:, 0])),
                         per_block_ms=dict(pair=b[:, 4].tolist(), sum=b[:, 5].tolist(), triplet=b[:, 6].tolist(), sweep=b[:, 7].tolist())))
        print("S=%d rep %d: pass %.1f ms (pair %.2f sum %.2f triplet %.2f sweeps %.2f ms per block, %d of %d accepted) energy %.6g -> %.6g | fusion loop %.1f ms -> %.6g"
              % (S, r, 1e3 * pass_s, np.median(b[:, 4]), np.median(b[:, 5]), np.median(b[:, 6]), np.median(b[:, 7]), int(b[:, 2].sum()), S, e_start, e_pass,
                 1e3 * fusion_s, e_fusion), flush=True)
    ctx.set_mcmc_draw(0)
    med = lambda key: float(np.median([x[key] for x in runs]))  # noqa: E731
    blk = lambda key: float(np.median([np.median(x["per_block_ms"][key]) for x in runs]))  # noqa: E731
    out = dict(S=S, data_order=data_order, cp_order=cp_order, nodes_per_subject=g.N, triplets_per_subject=g.Tc, labels=g.L, pairs=int(len(pairs)),
               mciters=mciters, mcparam=mcparam, chains=chains, draw=draw, icm_passes=icm_passes, setup_ms=1e3 * setup_s, energy_start=e_start,
               median=dict(pass_wall_ms=med("pass_wall_ms"), fusion_wall_ms=med("fusion_wall_ms"), block_pair_ms=blk("pair"), block_sum_ms=blk("sum"),
                           block_triplet_ms=blk("triplet"), block_sweep_ms=blk("sweep"), energy_after_pass=med("energy_after_pass"),
                           energy_after_fusion=med("energy_after_fusion")),
               runs=runs)
    g.close()
    del keep
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--subjects", type=int, nargs="+", default=[8, 64], choices=sorted(SHAPES))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--mciters", type=int, default=200)
    ap.add_argument("--mcparam", type=float, default=0.8)
    ap.add_argument("--chains", type=int, default=1)
    ap.add_argument("--icm-passes", type=int, default=5)
    ap.add_argument("--draw", choices=("host", "gpu"), default="host")
    ap.add_argument("--out", default="profiles/group_mcmc_time.json")
    a = ap.parse_args(argv)
    ctx = M.Context(0)
    results = []
    for S in a.subjects:
        results.append(measure(ctx, S, a.reps, a.mciters, a.mcparam, a.chains, a.icm_passes, a.draw))
        with open(a.out, "w") as f:  # after every size: what has been measured is kept
            json.dump(dict(tool="tools/time_group_mcmc.py", results=results), f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1:])
