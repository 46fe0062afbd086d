"""tools/time_mplp.py [--sweeps N] [--mcmc-sweeps N] [--repeats R] [--round | --forbid | --pairs] [--polish P] [--out FILE] -- the MPLP optimiser (an extension, not newMSM's) on the
MI355X against its host literal, over the unary and triplet tables tools/time_mcmc.py builds: BASELINE config 2 (pairwise sulc, ico6 data, ico4 control
grid, 19 labels) and an ico3 control grid.  It reports and judges nothing.  Per grid: the energy of the start (all zero), the energy the Monte Carlo
optimiser reaches on the device in --mcmc-sweeps sweeps (msm_cost_mcmc_optimise, tools/time_mcmc.py's sweep count by default), the energy of MPLP's decode
and its bound after every sweep, ms per sweep on the device by the HIP events around the sweeps' kernels (without and with the bound's second pass over
the table) beside the time the sweep's table bytes take at the HBM rate, and the ms of the host literal (msm_mplp_optimise over the fetched tables).  Times
are medians of the repeats with min and max, after a warm-up, and are reported only when the device's result equals the host literal's, bit for bit.
A table the optimiser refuses (a non-finite entry) is reported as refused, with the message.  Prints one JSON object.

--round measures the rounding of the messages instead (DESIGN.md 5.19 "Rounding"; profiles/mplp_round_time.json): per grid the energy of the conditioned
decode and of the polished winner after 1 / 5 / 10 / 20 / 30 sweeps (msm_cost_mplp_round, --polish passes), the polish of the zero labelling alone
(msm_cost_mplp_polish), ms per decode pass and per polish pass by the HIP events around their launches beside one sweep and the table at the HBM rate,
and the start, the Monte Carlo optimiser's energy and the bound.  Times are reported only when the device's result equals the host literal's.

--forbid measures the forbidden-entry reading (DESIGN.md 5.19 "Forbidden entries"; profiles/mplp_forbid_time.json) on the ico4 and ico3 tables built
without label rescaling on the regular control grid, which hold NaN and +infinity entries (their counts are printed): ms per sweep, per conditioned
decode and per polish pass of the forbidden-aware kernels (msm_mplp_optimise_forbid_gpu, msm_mplp_round_forbid_gpu) and, beside them, of the plain
kernels on a copy of the table whose forbidden entries the host replaced by 1e7 -- both in one process, alternated, by the HIP events around the
kernels.  With them the energies E^ of the start, of every sweep's decode and of the rounding's candidates, and the bound.  No time is a threshold.

--pairs measures MPLP over the pair tables of a --regoption=1 level instead (profiles/mplp_pairs_time.json), on the unary and pair tables
of the same two grids with the pairwise regulariser: ms per sweep by the HIP events around the sweeps' kernels (without and with the bound's pass), us per
pair class, the pair table at the HBM rate beside them, ms per polish pass, the wall clock of one call (msm_cost_mplp_pairs_optimise, tables on the
device) alternated in the same process with the wall clock of the present route of one iteration's solve (both tables fetched, msm_pairwise_icm with
100 passes), the host literal's ms per sweep, and the energies: the zero labelling, the stand-in's, the decode and the bound after 1 / 5 / 10 / 20 / 30
sweeps, the polished winner."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import newmsm_amd as M  # noqa: E402
from newmsm_amd import api, problem  # noqa: E402

HBM_BYTES_PER_S = 6.29e12  # measured float4 copy on the MI355X (8.0e12 is the specification)


def spread(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def equal(a, b):
    return (np.array_equal(a.labeling, b.labeling) and a.sweeps_run == b.sweeps_run and a.energy == b.energy and a.energies.tobytes() == b.energies.tobytes()
            and (a.bounds is None or b.bounds is None or a.bounds.tobytes() == b.bounds.tobytes()))


def measure(ctx, cp_order, sweeps, mcmc_sweeps, repeats):
    inp = problem.pairwise_inputs(6, cp_order, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate")
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    triplets = inp["triplets"]
    start = np.zeros(cf.N, dtype=np.int32)
    table_bytes = cf.T * cf.L ** 3 * 8
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, sweeps=sweeps, repeats=repeats, triplet_table_MB=table_bytes / 1e6,
               table_ms_at_hbm_rate=table_bytes / HBM_BYTES_PER_S * 1e3, hbm_bytes_per_s=HBM_BYTES_PER_S)
    U = cf.computeUnaryCosts()
    tc = np.array(cf.computeTripletCosts(pinned=True))
    out["energy_start"] = api.mcmc_energy(U, tc, triplets, start)
    out["mcmc"] = dict(sweeps=mcmc_sweeps, mcparam=0.8, seed=3, energy=api.mcmc_energy(U, tc, triplets, cf.mcmc_optimise(start, mcparam=0.8, iters=mcmc_sweeps, seed=3)))
    try:
        cf.mplp_optimise(start, sweeps=2, bounds=True)  # warm-up: code objects, staging blocks, the scratch buffers
        cf.mplp_optimise(start, sweeps=2, bound=False)
    except M.MsmError as e:
        out["refused"] = str(e)
        cf.close()
        return out
    plain, bounded, host_ms, same = [], [], [], True
    for _ in range(repeats):
        fast = cf.mplp_optimise(start, sweeps=sweeps, bound=False)
        plain.append(api.mplp_gpu_stats(ctx))
        full = cf.mplp_optimise(start, sweeps=sweeps, bounds=True)
        bounded.append(api.mplp_gpu_stats(ctx))
        t0 = time.perf_counter()
        want = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bounds=True)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        same = same and equal(fast, want) and equal(full, want)
    out.update(results_equal=bool(same), sweeps_run=full.sweeps_run, levels_per_sweep=plain[0]["levels_per_sweep"], widest_level=plain[0]["widest_level"],
               energy=full.energy, bound=full.bound, energies=full.energies.tolist(), bounds=full.bounds.tolist())
    cf.close()
    if not same:
        return out  # no time is reported for a result that is not the host literal's
    out.update(gpu_kernel_ms_per_sweep=spread([s["kernel_ms"] / max(s["sweeps_run"], 1) for s in plain]),
               gpu_kernel_ms_per_sweep_with_bounds=spread([s["kernel_ms"] / max(s["sweeps_run"], 1) for s in bounded]),
               gpu_us_per_level=spread([1e3 * s["kernel_ms"] / max(s["sweeps_run"] * s["levels_per_sweep"], 1) for s in plain]),
               host_literal_ms=spread(host_ms), host_literal_ms_per_sweep=spread([ms / max(full.sweeps_run, 1) for ms in host_ms]))
    out["sweep_over_table_at_hbm_rate"] = out["gpu_kernel_ms_per_sweep"]["median"] / out["table_ms_at_hbm_rate"]
    return out


ROUND_SWEEPS = (1, 5, 10, 20, 30)


def measure_round(ctx, cp_order, mcmc_sweeps, repeats, polish):
    inp = problem.pairwise_inputs(6, cp_order, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate")
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    triplets = inp["triplets"]
    start = np.zeros(cf.N, dtype=np.int32)
    table_bytes = cf.T * cf.L ** 3 * 8
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, polish=polish, repeats=repeats, triplet_table_MB=table_bytes / 1e6,
               table_ms_at_hbm_rate=table_bytes / HBM_BYTES_PER_S * 1e3, hbm_bytes_per_s=HBM_BYTES_PER_S)
    U = cf.computeUnaryCosts()
    tc = np.array(cf.computeTripletCosts(pinned=True))
    out["energy_start"] = api.mcmc_energy(U, tc, triplets, start)
    out["mcmc"] = dict(sweeps=mcmc_sweeps, mcparam=0.8, seed=3, energy=api.mcmc_energy(U, tc, triplets, cf.mcmc_optimise(start, mcparam=0.8, iters=mcmc_sweeps, seed=3)))
    try:
        cf.mplp_round(start, sweeps=2, polish=2)  # warm-up
        cf.mplp_polish(start, polish=2)
    except M.MsmError as e:
        out["refused"] = str(e)
        cf.close()
        return out
    same, rows, decode_ms, polish_ms, sweep_ms = True, [], [], [], []
    for n in ROUND_SWEEPS:
        for rep in range(repeats):
            got, run, bound = cf.mplp_round(start, sweeps=n, polish=polish)
            stats = api.mplp_round_gpu_stats(ctx)
            decode_ms.append(stats["decode_ms"])
            polish_ms.append(stats["polish_ms"] / max(stats["passes_run"], 1))
            sweep = api.mplp_gpu_stats(ctx)
            sweep_ms.append(sweep["kernel_ms"] / max(sweep["sweeps_run"], 1))
        r = api.mplp_optimise(U, tc, triplets, start, sweeps=n, bound=False, messages=True)
        want = api.mplp_round(U, tc, triplets, r.labeling, messages=r.messages, mode=0, polish=polish)
        same = same and np.array_equal(got.labeling, want.labeling) and got.passes_run == want.passes_run and got.energies.tobytes() == want.energies.tobytes()
        rows.append(dict(sweeps=n, sweeps_run=run, bound=bound, energy_naive_best=float(min(r.energies.min(), out["energy_start"])), energy_rounded=got.energies[1],
                         energy_polished=float(got.energies[2:].min()) if polish else None, energy_returned=got.energy, passes_run=got.passes_run,
                         classes=stats["classes"]))
    zero = cf.mplp_polish(start, polish=64)
    zstats = api.mplp_round_gpu_stats(ctx)
    zwant = api.mplp_round(U, tc, triplets, start, mode=1, polish=64)
    same = same and np.array_equal(zero.labeling, zwant.labeling) and zero.energies.tobytes() == zwant.energies.tobytes()
    out.update(results_equal=bool(same), after_sweeps=rows,
               polish_of_zero_labelling=dict(polish=64, passes_run=zero.passes_run, energy=zero.energy, energies=zero.energies[:zero.passes_run + 1].tolist()))
    cf.close()
    if not same:
        return out
    out.update(gpu_ms_per_decode_pass=spread(decode_ms), gpu_ms_per_polish_pass=spread(polish_ms), gpu_kernel_ms_per_sweep=spread(sweep_ms),
               gpu_ms_polish_call_of_zero_labelling=zstats["polish_ms"])  # (every pass asked for is queued: those behind the fixed point return at once)
    out["decode_pass_over_table_at_hbm_rate"] = out["gpu_ms_per_decode_pass"]["median"] / out["table_ms_at_hbm_rate"]
    return out


def measure_forbid(ctx, cp_order, sweeps, repeats, polish):
    from newmsm_amd import synthetic
    inp = problem.pairwise_inputs(6, cp_order, D=1, rescale=False, warp_amp=0.0, warp_rot=0.0)  # the regular control grid under the sampling grid's own labels
    inp["src_feat"] = synthetic.features(synthetic.known_warp(inp["source_orig_xyz"], seed=77, rot_deg=3.0, amp=1.2), 1, 1234)  # (a unary table that is not flat)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate")
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    triplets = inp["triplets"]
    start = np.zeros(cf.N, dtype=np.int32)
    table_bytes = cf.T * cf.L ** 3 * 8
    U = np.array(cf.computeUnaryCosts())
    tc = np.array(cf.computeTripletCosts(pinned=True))
    counts = api.mplp_classify(U, tc)
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, sweeps=sweeps, polish=polish, repeats=repeats, triplet_table_MB=table_bytes / 1e6,
               table_ms_at_hbm_rate=table_bytes / HBM_BYTES_PER_S * 1e3, hbm_bytes_per_s=HBM_BYTES_PER_S,
               counts=dict(unary_non_finite=int(counts[0]), triplet_nan=int(counts[1]), triplet_plus_inf=int(counts[2]), triplet_minus_inf=int(counts[3])))
    stand_in = np.where(tc < np.inf, tc, 1e7)  # what the plain route can read: the yardstick
    cf.set_mplp_forbid()
    device_counts = np.zeros(4, dtype=np.int64)
    routes = {"forbid": dict(tc=tc, kw=dict(forbid=True, counts=device_counts)), "plain_on_1e7_stand_in": dict(tc=stand_in, kw=dict())}
    for r in routes.values():  # warm-up: code objects, staging blocks, the scratch buffers; and the messages the rounding is timed on
        r["run"] = api.mplp_optimise_gpu(ctx, U, r["tc"], triplets, start, sweeps=sweeps, bounds=True, messages=True, **r["kw"])
        api.mplp_round_gpu(ctx, U, r["tc"], triplets, r["run"].labeling, messages=r["run"].messages, mode=0, polish=polish, **r["kw"])
        r.update(sweep_ms=[], sweep_bounds_ms=[], decode_ms=[], polish_ms=[])
    for _ in range(repeats):
        for r in routes.values():  # alternated
            api.mplp_optimise_gpu(ctx, U, r["tc"], triplets, start, sweeps=sweeps, bound=False, **r["kw"])
            st = api.mplp_gpu_stats(ctx)
            r["sweep_ms"].append(st["kernel_ms"] / max(st["sweeps_run"], 1))
            api.mplp_optimise_gpu(ctx, U, r["tc"], triplets, start, sweeps=sweeps, bounds=True, **r["kw"])
            st = api.mplp_gpu_stats(ctx)
            r["sweep_bounds_ms"].append(st["kernel_ms"] / max(st["sweeps_run"], 1))
            r["round"] = api.mplp_round_gpu(ctx, U, r["tc"], triplets, r["run"].labeling, messages=r["run"].messages, mode=0, polish=polish, **r["kw"])
            st = api.mplp_round_gpu_stats(ctx)
            r["decode_ms"].append(st["decode_ms"])
            r["polish_ms"].append(st["polish_ms"] / max(st["passes_run"], 1))
    f = routes["forbid"]
    got = cf.mplp_optimise(start, sweeps=sweeps, bounds=True, messages=True)  # the cost function's own device tables
    want = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, bounds=True, messages=True, forbid=True)
    wround = api.mplp_round(U, tc, triplets, want.labeling, messages=want.messages, mode=0, polish=polish, forbid=True)
    same = (equal(f["run"], want) and equal(got, want) and f["run"].messages.tobytes() == want.messages.tobytes() and device_counts.tolist() == counts.tolist()
            and cf.mplp_forbidden().tolist() == counts.tolist() and np.array_equal(f["round"].labeling, wround.labeling)
            and f["round"].energies.tobytes() == wround.energies.tobytes())
    cf.close()
    out["results_equal"] = bool(same)
    for name, r in routes.items():
        row = dict(sweeps_run=r["run"].sweeps_run, energy=r["run"].energy,
                   bound=r["run"].bound, energies=r["run"].energies.tolist(), bounds=r["run"].bounds.tolist(), infinite_messages=int(np.isinf(r["run"].messages).sum()),
                   rounding_energies=r["round"].energies.tolist(), rounding_energy=r["round"].energy, passes_run=r["round"].passes_run)
        row["energy_start"] = api.mplp_round(U, r["tc"], triplets, start, mode=1, polish=0, forbid=name == "forbid").energy
        if same:  # no time is reported beside a result that is not the host literal's
            row.update(gpu_kernel_ms_per_sweep=spread(r["sweep_ms"]), gpu_kernel_ms_per_sweep_with_bounds=spread(r["sweep_bounds_ms"]),
                       gpu_ms_per_decode_pass=spread(r["decode_ms"]), gpu_ms_per_polish_pass=spread(r["polish_ms"]))
        out[name] = row
    return out


def measure_pairs(ctx, cp_order, sweeps, repeats, polish):
    inp = problem.pairwise_inputs(6, cp_order, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", rmode=1)
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    pairs = inp["pairs"]
    start = np.zeros(cf.N, dtype=np.int32)
    table_bytes = cf.P * cf.L ** 2 * 8
    out = dict(cp_order=cp_order, N=cf.N, P=cf.P, L=cf.L, sweeps=sweeps, polish=polish, repeats=repeats, pair_table_MB=table_bytes / 1e6,
               table_ms_at_hbm_rate=table_bytes / HBM_BYTES_PER_S * 1e3, hbm_bytes_per_s=HBM_BYTES_PER_S)
    U = cf.computeUnaryCosts()
    pc = np.array(cf.computePairwiseCosts())
    out["energy_start"] = api.mplp_pairs_energy(U, pc, pairs, start)
    try:
        cf.mplp_pairs_optimise(start, sweeps=2, polish=2, bounds=True)  # warm-up: code objects, staging blocks, the scratch buffers
        cf.mplp_pairs_optimise(start, sweeps=2, bound=False)
    except M.MsmError as e:
        out["refused"] = str(e)
        cf.close()
        return out
    plain, bounded, polished, host_ms, call_ms, icm_ms, same = [], [], [], [], [], [], True
    for _ in range(repeats):  # the new call and the present route of one iteration's solve, alternated in this process
        t0 = time.perf_counter()
        fast, _ = cf.mplp_pairs_optimise(start, sweeps=sweeps, bound=False)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        plain.append(api.mplp_pairs_gpu_stats(ctx))
        t0 = time.perf_counter()
        icm = api.pairwise_icm(cf.computeUnaryCosts(), cf.computePairwiseCosts(), pairs, passes=100)
        icm_ms.append((time.perf_counter() - t0) * 1e3)
        full, _ = cf.mplp_pairs_optimise(start, sweeps=sweeps, bounds=True)
        bounded.append(api.mplp_pairs_gpu_stats(ctx))
        both, pol = cf.mplp_pairs_optimise(start, sweeps=sweeps, polish=polish, bound=False)
        polished.append(api.mplp_pairs_gpu_stats(ctx))
        t0 = time.perf_counter()
        want = api.mplp_pairs_optimise(U, pc, pairs, start, sweeps=sweeps, bounds=True)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        wpol = api.mplp_pairs_polish(U, pc, pairs, want.labeling, polish=polish)
        same = (same and equal(fast, want) and equal(full, want) and np.array_equal(pol.labeling, wpol.labeling) and pol.passes_run == wpol.passes_run
                and pol.energies.tobytes() == wpol.energies.tobytes())
    out.update(results_equal=bool(same), sweeps_run=full.sweeps_run, classes_per_sweep=plain[0]["classes"], widest_class=plain[0]["widest_class"],
               energy=full.energy, bound=full.bound, energies=full.energies.tolist(), bounds=full.bounds.tolist(),
               energy_icm_stand_in=api.mplp_pairs_energy(U, pc, pairs, icm), energy_polished=pol.energy, polish_passes_run=pol.passes_run,
               polish_energies=pol.energies.tolist(),
               after_sweeps=[dict(sweeps=n, energy_decode=full.energies[n - 1], bound=full.bounds[n - 1]) for n in ROUND_SWEEPS if n <= sweeps])
    cf.close()
    if not same:
        return out  # no time is reported for a result that is not the host literal's
    out.update(gpu_kernel_ms_per_sweep=spread([s["kernel_ms"] / max(s["sweeps_run"], 1) for s in plain]),
               gpu_kernel_ms_per_sweep_with_bounds=spread([s["kernel_ms"] / max(s["sweeps_run"], 1) for s in bounded]),
               gpu_us_per_class=spread([1e3 * s["kernel_ms"] / max(s["sweeps_run"] * s["classes"], 1) for s in plain]),
               gpu_ms_per_polish_pass=spread([s["polish_ms"] / max(s["passes_run"], 1) for s in polished]),
               wall_ms_new_call=spread(call_ms), wall_ms_present_route_fetch_and_icm=spread(icm_ms),
               host_literal_ms=spread(host_ms), host_literal_ms_per_sweep=spread([ms / max(full.sweeps_run, 1) for ms in host_ms]))
    out["sweep_over_table_at_hbm_rate"] = out["gpu_kernel_ms_per_sweep"]["median"] / out["table_ms_at_hbm_rate"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweeps", type=int, default=30)
    ap.add_argument("--mcmc-sweeps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--round", action="store_true", help="measure the rounding of the messages instead of the sweeps")
    ap.add_argument("--forbid", action="store_true", help="measure the forbidden-entry reading beside the plain route on a 1e7 stand-in table")
    ap.add_argument("--pairs", action="store_true", help="measure MPLP over the pair tables of a --regoption=1 level (DESIGN.md 5.20)")
    ap.add_argument("--polish", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("time_mplp.py: no HIP device is visible (nothing is measured without one)")
    ctx = M.Context(0)
    if a.pairs:
        result = dict(tool="tools/time_mplp.py --pairs", grids=[measure_pairs(ctx, cp, a.sweeps, a.repeats, a.polish) for cp in (4, 3)])
    elif a.forbid:
        result = dict(tool="tools/time_mplp.py --forbid", grids=[measure_forbid(ctx, cp, a.sweeps, a.repeats, a.polish) for cp in (4, 3)])
    elif a.round:
        result = dict(tool="tools/time_mplp.py --round", grids=[measure_round(ctx, cp, a.mcmc_sweeps, a.repeats, a.polish) for cp in (4, 3)])
    else:
        result = dict(tool="tools/time_mplp.py", grids=[measure(ctx, cp, a.sweeps, a.mcmc_sweeps, a.repeats) for cp in (4, 3)])
    ctx.close()
    text = json.dumps(result, indent=1, default=lambda o: o.item())  # (numpy scalars)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
