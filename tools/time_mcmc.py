"""tools/time_mcmc.py [--sweeps N] [--repeats R] [--out FILE] -- the Monte Carlo optimiser (MCMC::optimise, M/mcmc_opt.h:31-134) on the host against its
sweeps on the MI355X, over the unary and triplet tables of BASELINE config 2 (pairwise sulc, ico6 data, ico4 control grid, 19 labels) and of an ico3
control grid.  In one process, alternating: the host path (msm_cost_unary_table + msm_cost_triplet_table into pinned memory + msm_mcmc_optimise) and
msm_cost_mcmc_optimise (both tables stay on the device).  A time is reported only when the two labellings are equal.  Per grid, medians of the repeats with
min and max: ms per sweep either way, us per level by the HIP events around the sweep kernels, the proposal stream's draws per second on the host alone,
the time the host path spends computing and fetching the triplet table, and the time the device path spends on its two tables.  Prints one JSON object.
With --draw gpu the single-chain call is timed once more per repeat with its proposals drawn on the device (msm_ctx_set_mcmc_draw): gpu_device_draw.

tools/time_mcmc.py --chains 1,4,16,64 --baseline-lib PARENT/newmsm_amd/libmsmhip.so [--sweeps N] [--repeats R] [--out FILE] -- several chains in one launch
(msm_cost_mcmc_optimise_chains, DESIGN.md 5.16 "Chains") against K successive msm_cost_mcmc_optimise calls of another build: the library of a checkout of
the parent commit, driven through the Python mirror that lies beside it (loaded under another name), so both builds run in this one process, alternated,
after warm-up.  Per grid and K, medians of the repeats with min and max: ms of the chains call, ms of the K baseline calls, kernel ms and us per level
(levels walked by one chain) by the HIP events, the wall ms of the threaded draw and its threads.  A time is reported only when every chain's labelling
equals the baseline call with that chain's seed.  "apart": the chains call's slowest repeat lies below the fastest repeat of the K baseline calls.

tools/time_mcmc.py --chains 1,4,16,64,256 --draw host,gpu --baseline-lib PARENT/newmsm_amd/libmsmhip.so [--sweeps N] [--repeats R] [--out FILE] -- the chains
call with the proposals drawn on the host and on the device (msm_ctx_set_mcmc_draw, DESIGN.md 5.16 "Proposals on the device") against the chains call of
the baseline build (the parent commit's), both libraries in this one process, alternated after two warm-up rounds.  Per grid, K and mode, medians of the
repeats with min and max: ms of the call, ms in the sweeps kernels, the draw's ms (host: wall clock of the threaded draw; gpu: the draw kernels by their
events) and, for gpu, accepted proposals per second of draw-kernel time.  A mode's times are reported only when every labelling equals the baseline's.
"apart": the mode's slowest repeat lies below the baseline call's fastest.  Without --baseline-lib no other build is loaded (MSM_LIB_PATH then selects the
one that is timed): a mode's labellings are compared with those of the first mode."""
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


def spread(values):
    v = sorted(values)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1])


def measure(ctx, cp_order, sweeps, repeats, mcparam, seed, device_draw=False):
    inp = problem.pairwise_inputs(6, cp_order, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate")
    cf.get_source_data()
    keep["target"].prepare_search(wait=True)
    triplets = inp["triplets"]
    start = np.zeros(cf.N, dtype=np.int32)
    kw = dict(mcparam=mcparam, seed=seed)

    def host(iters):
        t0 = time.perf_counter()
        U = cf.computeUnaryCosts()
        t1 = time.perf_counter()
        tc = cf.computeTripletCosts(pinned=True)
        t2 = time.perf_counter()
        lab = api.mcmc_optimise(U, tc, triplets, start, iters=iters, **kw)
        t3 = time.perf_counter()
        return lab, dict(unary_ms=(t1 - t0) * 1e3, triplet_fetch_ms=(t2 - t1) * 1e3, sweeps_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)

    def device(iters, draw="host"):
        ctx.set_mcmc_draw(draw)
        ctx.synchronize()
        t0 = time.perf_counter()
        lab = cf.mcmc_optimise(start, iters=iters, **kw)
        t1 = time.perf_counter()
        ctx.set_mcmc_draw("host")
        return lab, dict(total_ms=(t1 - t0) * 1e3, **api.mcmc_gpu_stats(ctx))

    for _ in range(2):  # warm-up of every shape the timed window uses: code objects, staging blocks, the pinned table buffer
        host(20), device(20)
        if device_draw:
            device(20, "gpu")
    runs_h, runs_d, runs_g, tables_ms, equal, equal_g = [], [], [], [], True, True
    for _ in range(repeats):
        lab_h, h = host(sweeps)
        lab_d, d = device(sweeps)
        if device_draw:
            lab_g, g = device(sweeps, "gpu")
            equal_g = equal_g and np.array_equal(lab_h, lab_g)
            runs_g.append(g)
        ctx.synchronize()
        t0 = time.perf_counter()
        cf.mcmc_optimise(start, iters=0, **kw)  # the two tables alone: no sweep is run
        tables_ms.append((time.perf_counter() - t0) * 1e3)
        equal = equal and np.array_equal(lab_h, lab_d)
        runs_h.append(h), runs_d.append(d)
    draws = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        api.mcmc_proposals(cf.L, mcparam, seed, cf.T, sweeps)
        draws.append(sweeps * cf.T / (time.perf_counter() - t0))
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, sweeps=sweeps, repeats=repeats, mcparam=mcparam, triplet_table_MB=cf.T * cf.L ** 3 * 8 / 1e6,
               labellings_equal=bool(equal), labels_in_result=int(len(np.unique(lab_h))), levels_per_sweep=runs_d[0]["levels_per_sweep"],
               widest_level=runs_d[0]["widest_level"], chunks=runs_d[0]["chunks"])
    cf.close()
    if not equal:
        return out  # no time is reported for a result that is not the host's
    out.update(
        host_ms_per_sweep=spread([r["sweeps_ms"] / sweeps for r in runs_h]),
        host_triplet_table_fetch_ms=spread([r["triplet_fetch_ms"] for r in runs_h]),
        host_unary_table_ms=spread([r["unary_ms"] for r in runs_h]),
        host_total_ms=spread([r["total_ms"] for r in runs_h]),
        gpu_ms_per_sweep=spread([(r["total_ms"] - t) / sweeps for r, t in zip(runs_d, tables_ms)]),
        gpu_kernel_ms_per_sweep=spread([r["kernel_ms"] / sweeps for r in runs_d]),
        gpu_us_per_level=spread([1e3 * r["kernel_ms"] / r["levels"] for r in runs_d]),
        gpu_draw_ms_per_sweep=spread([r["draw_ms"] / sweeps for r in runs_d]),
        gpu_tables_ms=spread(tables_ms),
        gpu_total_ms=spread([r["total_ms"] for r in runs_d]),
        proposal_draws_per_s=spread(draws),
    )
    if device_draw:
        out["gpu_device_draw"] = dict(labellings_equal=bool(equal_g))
        if equal_g:
            out["gpu_device_draw"].update(total_ms=spread([r["total_ms"] for r in runs_g]), kernel_ms=spread([r["kernel_ms"] for r in runs_g]))
    # "faster" only where the slower path's fastest run is above the faster path's slowest
    out["gpu_faster_total"] = out["gpu_total_ms"]["max"] < out["host_total_ms"]["min"]
    out["gpu_faster_sweeps"] = out["gpu_ms_per_sweep"]["max"] < out["host_ms_per_sweep"]["min"]
    bounds = dict(levels=out["gpu_kernel_ms_per_sweep"]["median"], proposals=out["gpu_draw_ms_per_sweep"]["median"], tables=out["gpu_tables_ms"]["median"] / sweeps)
    out["gpu_bound_by"] = max(bounds, key=bounds.get)
    # arithmetic, not a measurement: the reference's default --mciters=100000 at the per-sweep figures above
    out["arithmetic_s_per_100000_sweeps"] = dict(host=out["host_ms_per_sweep"]["median"] * 100, gpu=out["gpu_ms_per_sweep"]["median"] * 100)
    return out


def load_baseline(lib_path):
    """the Python mirror beside another build's libmsmhip.so (a checkout's newmsm_amd/), imported under a name of its own: it binds that library"""
    import importlib.util

    pkg = os.path.dirname(os.path.abspath(lib_path))
    if os.path.basename(lib_path) != "libmsmhip.so" or not os.path.exists(os.path.join(pkg, "__init__.py")):
        raise SystemExit("time_mcmc.py: --baseline-lib must be the newmsm_amd/libmsmhip.so of another checkout (its Python mirror is loaded with it)")
    if os.environ.get("MSM_LIB_PATH"):
        raise SystemExit("time_mcmc.py: MSM_LIB_PATH would bind both mirrors to one library; unset it")
    spec = importlib.util.spec_from_file_location("newmsm_amd_baseline", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["newmsm_amd_baseline"] = mod
    spec.loader.exec_module(mod)
    import newmsm_amd_baseline.problem  # noqa: F401

    assert os.path.samefile(mod.LIB_PATH, lib_path) and not os.path.samefile(mod.LIB_PATH, M.LIB_PATH), (mod.LIB_PATH, M.LIB_PATH)
    return mod


def measure_chains(ctx, base, base_ctx, cp_order, chains, sweeps, repeats, mcparam, seed):
    def build(mod, c):
        inp = mod.problem.pairwise_inputs(6, cp_order, D=1)
        cf, keep = mod.problem.build_cost(c, inp, kind="univariate")
        cf.get_source_data()
        keep["target"].prepare_search(wait=True)
        return cf, keep

    cf, keep = build(M, ctx)
    cfb, keepb = build(base, base_ctx)
    start = np.zeros(cf.N, dtype=np.int32)
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, sweeps=sweeps, repeats=repeats, mcparam=mcparam, per_K=[])

    def ours(seeds, iters):
        ctx.synchronize()
        t0 = time.perf_counter()
        res = cf.mcmc_optimise_chains(start, seeds, mcparam=mcparam, iters=iters)
        ms = (time.perf_counter() - t0) * 1e3
        return res, dict(total_ms=ms, draw_threads=api.mcmc_chains_info(ctx)[1], **api.mcmc_gpu_stats(ctx))

    def theirs(seeds, iters):
        base_ctx.synchronize()
        t0 = time.perf_counter()
        labs = [cfb.mcmc_optimise(start, mcparam=mcparam, iters=iters, seed=s) for s in seeds]
        return labs, (time.perf_counter() - t0) * 1e3

    for K in chains:
        seeds = api.chain_seeds(seed, 0, K)
        for _ in range(2):  # warm-up of both builds at this K: code objects, staging blocks, the K-chain buffers
            ours(seeds, 20), theirs(seeds[:2], 20)
        runs, base_ms, equal = [], [], True
        for _ in range(repeats):
            (lab, labs, E, best), r = ours(seeds, sweeps)
            want, ms = theirs(seeds, sweeps)
            equal = equal and all(np.array_equal(labs[k], want[k]) for k in range(K)) and np.array_equal(lab, labs[best])
            runs.append(r), base_ms.append(ms)
        row = dict(K=K, labellings_equal=bool(equal), best=int(best), chunks=runs[0]["chunks"], draw_threads=runs[0]["draw_threads"],
                   levels_per_sweep=runs[0]["levels_per_sweep"])
        if equal:  # no time is reported for a result that is not the baseline's
            row.update(chains_ms=spread([r["total_ms"] for r in runs]), baseline_ms=spread(base_ms),
                       kernel_ms=spread([r["kernel_ms"] for r in runs]), us_per_level=spread([1e3 * r["kernel_ms"] / r["levels"] for r in runs]),
                       draw_ms=spread([r["draw_ms"] for r in runs]))
            row["apart"] = bool(row["chains_ms"]["max"] < row["baseline_ms"]["min"])
            row["draw_binds"] = bool(row["draw_ms"]["median"] > row["kernel_ms"]["median"])
        out["per_K"].append(row)
    cf.close(), cfb.close()
    return out


def measure_draw(ctx, base, base_ctx, cp_order, chains, modes, sweeps, repeats, mcparam, seed):
    """the chains call of this build with the proposals drawn as `modes` say ("host", "gpu": msm_ctx_set_mcmc_draw) against the chains call of the baseline
    build, per K; a mode's times are reported only when every labelling of every repeat equals the baseline's"""
    def build(mod, c):
        inp = mod.problem.pairwise_inputs(6, cp_order, D=1)
        cf, keep = mod.problem.build_cost(c, inp, kind="univariate")
        cf.get_source_data()
        keep["target"].prepare_search(wait=True)
        return cf, keep

    cf, keep = build(M, ctx)
    cfb, keepb = build(base, base_ctx) if base else (None, None)
    start = np.zeros(cf.N, dtype=np.int32)
    out = dict(cp_order=cp_order, N=cf.N, T=cf.T, L=cf.L, sweeps=sweeps, repeats=repeats, mcparam=mcparam, per_K=[])

    def ours(mode, seeds, iters):
        ctx.set_mcmc_draw(mode)
        ctx.synchronize()
        t0 = time.perf_counter()
        res = cf.mcmc_optimise_chains(start, seeds, mcparam=mcparam, iters=iters)
        ms = (time.perf_counter() - t0) * 1e3
        r = dict(total_ms=ms, draw_threads=api.mcmc_chains_info(ctx)[1], **api.mcmc_gpu_stats(ctx))
        if mode == "gpu":
            r.update(api.mcmc_draw_stats(ctx))  # draw_ms: the draw kernels' (the host drew nothing)
        ctx.set_mcmc_draw("host")
        return res, r

    def theirs(seeds, iters):
        base_ctx.synchronize()
        t0 = time.perf_counter()
        res = cfb.mcmc_optimise_chains(start, seeds, mcparam=mcparam, iters=iters)
        return res, (time.perf_counter() - t0) * 1e3

    for K in chains:
        seeds = api.chain_seeds(seed, 0, K)
        for _ in range(2):  # warm-up of both builds at this K and in every mode: code objects, staging blocks, both proposal buffers
            for mode in modes:
                ours(mode, seeds, 20)
            if base:
                theirs(seeds, 20)
        runs, base_ms, equal = {m: [] for m in modes}, [], {m: True for m in modes}
        for _ in range(repeats):
            got = {}
            for mode in modes:
                got[mode], r = ours(mode, seeds, sweeps)
                runs[mode].append(r)
            want, ms = theirs(seeds, sweeps) if base else (got[modes[0]], None)
            if base:
                base_ms.append(ms)
            for mode in modes:
                equal[mode] = equal[mode] and np.array_equal(got[mode][1], want[1]) and np.array_equal(got[mode][0], want[0]) and got[mode][3] == want[3]
        row = dict(K=K, levels_per_sweep=runs[modes[0]][0]["levels_per_sweep"], chunks=runs[modes[0]][0]["chunks"])
        if base:
            row["baseline_ms"] = spread(base_ms)
        for mode in modes:
            rs = runs[mode]
            m = dict(labellings_equal=bool(equal[mode]), draw_threads=rs[0]["draw_threads"])
            if equal[mode]:  # no time is reported for a result that is not the baseline's
                m.update(total_ms=spread([r["total_ms"] for r in rs]), kernel_ms=spread([r["kernel_ms"] for r in rs]), draw_ms=spread([r["draw_ms"] for r in rs]))
                if base:
                    m["apart"] = bool(m["total_ms"]["max"] < row["baseline_ms"]["min"])
                if mode == "gpu":
                    m["proposals_per_s"] = spread([r["accepted"] / (r["draw_ms"] * 1e-3) for r in rs])
                    m["candidates_per_proposal"] = rs[0]["candidates"] / rs[0]["accepted"]
                    m["block_bound"] = rs[0]["block_bound"]
            row[mode] = m
        out["per_K"].append(row)
    cf.close()
    if base:
        cfb.close()
    return out


def main_chains(a):
    chains = [int(k) for k in a.chains.split(",")]
    if not chains or min(chains) < 1 or max(chains) > 256:
        raise SystemExit("time_mcmc.py: --chains takes numbers from 1 to 256")
    modes = a.draw.split(",") if a.draw else []
    if any(m not in ("host", "gpu") for m in modes):
        raise SystemExit("time_mcmc.py: --draw takes host, gpu or both")
    if not a.baseline_lib and not modes:
        raise SystemExit("time_mcmc.py: --chains needs --baseline-lib (the build the K successive calls run on)")
    base = load_baseline(a.baseline_lib) if a.baseline_lib else None
    ctx, base_ctx = M.Context(0), base.Context(0) if base else None
    if modes:
        result = dict(tool="tools/time_mcmc.py --chains --draw", host_threads=os.environ.get("MSMHIP_HOST_THREADS"),
                      grids=[measure_draw(ctx, base, base_ctx, cp, chains, modes, a.sweeps, a.repeats, a.mcparam, 3) for cp in (4, 3)])
    else:
        result = dict(tool="tools/time_mcmc.py --chains", host_threads=os.environ.get("MSMHIP_HOST_THREADS"),
                      grids=[measure_chains(ctx, base, base_ctx, cp, chains, a.sweeps, a.repeats, a.mcparam, 3) for cp in (4, 3)])
    ctx.close()
    if base:
        base_ctx.close()
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default=None, help="e.g. 1,4,16,64: time the chains call against K successive calls of --baseline-lib")
    ap.add_argument("--baseline-lib", default=None, help="newmsm_amd/libmsmhip.so of a checkout of the commit to compare with")
    ap.add_argument("--draw", default=None, help="host,gpu (with --chains): time the chains call per proposal-draw mode against the chains call of --baseline-lib; "
                    "gpu (without --chains): time the single-chain call with the draw on the device as well")
    ap.add_argument("--sweeps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--mcparam", type=float, default=0.8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if M.device_count() < 1:
        raise SystemExit("time_mcmc.py: no HIP device is visible (nothing is measured without one)")
    if a.chains:
        result = main_chains(a)
    else:
        ctx = M.Context(0)
        if a.draw not in (None, "gpu"):
            raise SystemExit("time_mcmc.py: without --chains, --draw takes gpu")
        result = dict(tool="tools/time_mcmc.py", grids=[measure(ctx, cp, a.sweeps, a.repeats, a.mcparam, 3, device_draw=a.draw == "gpu") for cp in (4, 3)])
        ctx.close()
    text = json.dumps(result, indent=1, default=lambda o: o.item())  # (numpy scalars)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
