#!/usr/bin/env python3
"""bench.py -- the BASELINE.json metrics of the MI355X hot path: label-cost evals/sec, wall-clock per ico6 pairwise
registration, gMSM subjects/hour.

Default mode (--mode pairwise): one "step" = one computeUnaryCosts() of BASELINE config 2 -- pairwise sulc (D = 1) registration,
ico6 data grid (40 962 vertices), ico4 control grid (2 562 nodes), 19 labels -> 48 678 evals = 3.18 M point samples -- as an
iteration of a registration pays for it: the per (control point, label) rotations (estimate_rotation_matrix R/point.cpp:97-152:
new every iteration), the three table kernels, and the 389 KB table delivered to host memory (the optimiser reads it there).
All inputs are resident in HBM before the timed region starts.  A plain run sets up, warms up (--warmup steps), times --steps steps and
prints the headline line; --dump-outputs DIR then also writes the table of the last timed step (rank 0) to DIR/unary_costs.npy.  The inputs
are seeded: the same arguments give the same inputs in every run.  With --full the same JSON line carries, as extra objects (rank 0, N = 1):
  steady            the table kernels alone, enqueued back to back (the round-1 headline definition)
  resample          Resampler::get_barycentric_weights for the 40 962 vertices of an ico6 sphere: queries/s per kernel and per call, its roofline,
                    the CPU port's rate beside it
  triclique_move    one label step of Fusion (I/Fusion/Fusion.h:181-196) of the triclique classes: BASELINE config 4 (D = 1) and
                    config 3 (HCP MSMAll, D = 32) at ico6 / ico4 -- per call and per kernel, with their rooflines
  registration      wall-clock of a three-level ico6 pairwise registration driven by the reference's caller loop (Monte Carlo optimiser)
  registration_fusion  the same driven by fusion moves, as --dopt=HOCR drives BASELINE config 2
  registration_msmall  the same for the HCP MSMAll schedule (BASELINE config 3: triclique cost over 32 features, 40 iterations of fusion moves)
  gmsm              one groupwise iteration per level for 64 subjects on this GPU and the subjects/hour it implies
  cpu_baseline      the CPU port (oracle/) on the host cores, on a bounded sample of the headline workload

Multi-GPU (--gpus N, one process per GPU under torch.distributed.run):
  --mode pairwise   a pairwise registration does not shard: ranks are independent replicas working on
                    different synthetic subjects -- no data-path collective, weak scaling.  value = evals of all ranks / max-over-
                    ranks wall time.
  --mode gmsm       BASELINE config 5: 64 synthetic subjects, set-up sharded by subject, every label step sharded by clique,
                    RCCL all-gather / gather over xGMI (newmsm_amd/dist.py); strong scaling.  value = subjects/hour.
                    With --full the default mode at N > 1 runs this as well and reports it as the "gmsm" object of its line (the
                    group is the path that shards; MSM_BENCH_GMSM_SCALING=0 leaves it out).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
HCP = dict(rmode=3, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)  # --shearmod --bulkmod --k_exponent --regexp of the HCP / NeuroImage2017 configs


def algorithmic_bytes(samples, evals, D):
    """per point sample 116 + 32*D bytes (source coord 24 + hit-triangle vertex ids 12 +
    3 vertex coords 72 + 3*D reference values 24*D + source feature 8*D + weight 8); per eval 72 (rotation) + 8 (output)."""
    return samples * (116 + 32 * D) + evals * 80


DOMINANT_KERNEL = "msm::k_unary_rays"  # the sampling kernel of a simple-surface target (newmsm_amd/csrc/unary_kernels.hip)
PMC_PROFILE = os.path.join("profiles", "r5_z_unary_pmc.json")  # tools/collect_profile.sh r5_z on this workload (stamped with a hash of the kernel sources)


def kernel_algorithmic_bytes(samples, evals, D):
    """The dominant kernel's share of the section 8(d) figure: it reads the source coordinate (24), the hit triangle's
    vertex ids (12) and coordinates (72) and, for D = 1, the three reference values (24) of every point sample, and the
    rotation (72) of every eval.  The moving feature, its weight and the cost output belong to the reduction kernel."""
    return samples * (108 + (24 if D == 1 else 0)) + evals * 72


def kernel_source_stamp():
    """sha256 over newmsm_amd/csrc/*.hip, *.hpp, as tools/summarise_pmc.py stamps a profile: counters of a committed profile are reported only while
    the kernel sources are the ones that were profiled"""
    import hashlib

    h = hashlib.sha256()
    root = os.path.join(ROOT, "newmsm_amd", "csrc")
    for name in sorted(os.listdir(root)):
        if name.endswith((".hip", ".hpp")):
            h.update(name.encode())
            h.update(open(os.path.join(root, name), "rb").read())
    return h.hexdigest()


def profile_is_current(prof):
    """a profile without a stamp (rounds 1-3) is taken as it is; a stamped one must match the sources"""
    stamp = prof.get("kernel_source_sha256")
    return stamp is None or stamp == kernel_source_stamp()


def pmc_traffic(args):
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (separate --pmc runs,
    (2 * FETCH_SIZE + WRITE_SIZE) * 1024 as MI355X_MICROARCH.md prescribes for gfx950).  Only valid for the default workload."""
    if (args.data_order, args.cp_order, args.dims) != (6, 4, 1):
        return None
    try:
        with open(os.path.join(ROOT, PMC_PROFILE)) as f:
            prof = json.load(f)
        if not profile_is_current(prof):
            return None
        return prof["kernels"][DOMINANT_KERNEL]["hbm_traffic_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        return None


GPU_CLOCK_HZ = 2.4e9  # MI355X peak engine clock (MI355X_MICROARCH.md)
NUM_CUS = 256


def pmc_binding_limits(args, kernel_ms):
    """What binds the dominant kernel when its working set lives in the caches (the HBM fraction is nominal): from the committed PMC passes,
    per launch, against THIS run's kernel time --
      l1_lookup_frac   TCP_TOTAL_CACHE_ACCESSES (vector L1 tag look-ups, one per cache line a wavefront's load touches) / (256 CUs x cycles): the vL1D accepts
                       one look-up per CU and cycle, the divergent gathers of the sampling kernel make ~33 of them per wavefront load
      valu_issue_frac  SQ_INSTS_VALU / (1024 SIMDs x cycles / 4): a full-rate vector instruction occupies its SIMD for four cycles
      wait_frac        SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES: the share of their resident cycles the waves spend waiting for an instruction's operands
    Only valid for the default workload and the profiled sources."""
    if (args.data_order, args.cp_order, args.dims) != (6, 4, 1) or not kernel_ms:
        return None
    try:
        with open(os.path.join(ROOT, PMC_PROFILE)) as f:
            prof = json.load(f)
        if not profile_is_current(prof):
            return None
        c = prof["kernels"][DOMINANT_KERNEL]["per_launch_mean"]
        cycles = kernel_ms * 1e-3 * GPU_CLOCK_HZ
        return {"l1_lookup_frac": c["TCP_TOTAL_CACHE_ACCESSES_sum"] / (NUM_CUS * cycles), "l1_lookups_per_launch": c["TCP_TOTAL_CACHE_ACCESSES_sum"],
                "valu_issue_frac": c["SQ_INSTS_VALU"] / (4 * NUM_CUS * cycles / 4.0), "wait_frac": c["SQ_WAIT_INST_ANY"] / c["SQ_WAVE_CYCLES"],
                "definition": "vL1D look-ups per CU-cycle (peak 1), VALU issue slots used (peak 1), share of wave cycles waiting; counters per launch from "
                              + PMC_PROFILE + ", cycles = this run's kernel time x 2.4 GHz"}
    except (OSError, KeyError, ValueError, ZeroDivisionError):
        return None


def cpu_baseline(inp, kind, threads):
    """The oracle (CPU restatement of the reference algorithm, OpenMP over control points like
    M/DiscreteCostFunction.cpp:238-242) on the same workload.  Checker / baseline only."""
    from tests.helpers import oracle_cost

    oc = oracle_cost(inp, kind)
    oc.get_source_data()
    t0 = time.perf_counter()
    U = oc.unary_table(threads=threads)  # also warms the caches
    first = time.perf_counter() - t0
    reps = max(1, min(200, int(12.0 / max(first, 1e-3))))  # about 12 s of CPU work
    t0 = time.perf_counter()
    for _ in range(reps):
        U = oc.unary_table(threads=threads)
    dt = time.perf_counter() - t0
    return U, reps * U.size / dt, dt, reps


def bench_triclique_move(ctx, D, calls, threads):
    """One label step of Fusion for a triclique (HO) cost class at ico6 / ico4: msm_cost_triplet_octets, 8 x T evaluations."""
    import numpy as np

    from newmsm_amd import problem

    kind = "ho_univariate" if D == 1 else "ho_multivariate"
    lam = 0.025 if D == 1 else 0.01  # --lambda of config/NeuroImage2017_configs/sMSM_STR... / HCP MSMAllStrainFinalconf (last level)
    inp = problem.pairwise_inputs(6, 4, D=D)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, lambda_=lam, **HCP)
    cf.get_source_data()
    rng = np.random.default_rng(0)
    lab = rng.integers(0, cf.L, cf.N).astype(np.int32)
    E = ctx.host_array((cf.T, 8))  # the optimiser's per-step buffer: mapped pinned memory the kernel writes directly
    for _ in range(5):
        cf.tripletOctets(lab, 3, E)
    cf.enable_timing(True)
    ts = []
    for i in range(calls):
        t0 = time.perf_counter()
        cf.tripletOctets(lab, i % cf.L, E)
        ts.append(time.perf_counter() - t0)
    kt = cf.kernel_times() * 1e-3  # HIP events around the move's kernel(s), on the launch stream
    cf.enable_timing(False)
    call_s, kern_s = float(np.median(ts)), float(np.median(kt))
    evals = 8 * cf.T
    samples = 8 * len(inp["source_xyz"])  # every source vertex lies in one control triangle's bin; 8 combinations each
    nbytes = samples * (116 + 32 * D) + evals * 72  # per triclique eval its points x (116 + 32 D) + 3 x 24 B of control points
    out = {
        "workload": "%s, D=%d, ico6 data / ico4 control grid: %d evals = %d point samples per move" % (kind, D, evals, samples),
        "evals_per_s_call": evals / call_s, "us_per_call": call_s * 1e6, "evals_per_s_kernel": evals / kern_s, "kernel_us": kern_s * 1e6,
        "calls": calls, "algorithmic_bytes_per_move": nbytes,
        "roofline": {"bound": "hbm", "achieved": nbytes / kern_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": nbytes / kern_s / 1e9 / HBM_PEAK_GBS,
                     "frac_per_call": nbytes / call_s / 1e9 / HBM_PEAK_GBS, "kernel": "msm::k_ho_move",
                     "note": "kernel time = HIP events around the move's launch(es) on its stream; the working set is cache resident, so this is a nominal figure"},
    }
    if threads:
        from tests.helpers import oracle_cost

        oc = oracle_cost(inp, kind, lambda_=lam, **HCP)
        oc.get_source_data()
        t0 = time.perf_counter()
        ref = oc.triplet_octets(lab, 3, threads=threads)
        dt = time.perf_counter() - t0
        got = cf.tripletOctets(lab, 3, E)
        out["cpu_port"] = {"evals_per_s": evals / dt, "cores": threads, "sample": "one move (%d evals, %.2f s), OpenMP over triplets as I/Fusion/Fusion.h:181" % (evals, dt),
                           "max_rel_diff_vs_gpu": float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)))}
    cf.close()
    return out


def bench_resample(ctx, calls, cpu):
    """The resampler half of the path: Resampler::get_barycentric_weights (R/resampler.cpp:142-167 = Octree::get_closest_triangle
    R/octree.cpp:156-214 + calc_barycentric_weights R/triangle.cpp:124-143), the 40 962 vertices of the regular ico6 sphere located on a
    warped ico6 sphere whose octree was built for this run -- what every metric_resample / sphere_project_warp / get_source_data of a
    registration is made of.  SURVEY 8(d): 144 algorithmic bytes per query (query 24 + vertex ids 12 + vertices 72 + weights 24 + ids 12)."""
    import numpy as np

    import newmsm_amd as M
    from newmsm_amd import synthetic

    xyz, tri = M.make_mesh_from_icosa(6)
    warped = synthetic.known_warp(xyz, seed=3, rot_deg=2.0, amp=0.6)
    mesh = M.Mesh(ctx, warped, tri)
    N = len(xyz)
    st, t_id, vid, w = mesh.query_triangles(xyz)
    # the call as a C / C++ host makes it: the ABI's own layout (3 x N), arrays in pinned memory of the context (msm_host_alloc) -- the copy engine reads
    # the queries and writes the three result arrays where they lie: upload, kernel, three downloads, one synchronisation
    q_soa = ctx.host_array((3, N))
    q_soa[:] = xyz.T
    o_tri, o_vid, o_w = ctx.host_array((N,), np.int32), ctx.host_array((3, N), np.int32), ctx.host_array((3, N))
    ctx.time_queries(True)
    kt, ct, pt = [], [], []
    for _ in range(calls):
        t0 = time.perf_counter()
        rc = mesh.query_triangles_soa(q_soa, o_tri, o_vid, o_w)
        ct.append(time.perf_counter() - t0)
        kt.append(ctx.query_kernel_ms() * 1e-3)
        if rc:
            raise SystemExit("msm_query_triangles failed: %d" % rc)
    kd = list(kt)  # events around the kernel of the pinned-array call: with every array in mapped memory it reads and writes them over PCIe itself (round 5)
    kt = []
    for _ in range(max(10, calls // 5)):  # the Python wrapper over pageable numpy arrays (transposes, allocations, a staging memcpy each way): its kernel works HBM to HBM
        t0 = time.perf_counter()
        mesh.query_triangles(xyz)
        pt.append(time.perf_counter() - t0)
        kt.append(ctx.query_kernel_ms() * 1e-3)
    ctx.time_queries(False)
    if not (np.array_equal(o_tri, t_id) and np.array_equal(o_vid.T, vid) and np.array_equal(o_w.T, w)):
        raise SystemExit("the pinned-array call and the wrapper disagree")
    kern_s, call_s = float(np.median(kt)), float(np.median(ct))
    nbytes = 144 * N
    out = {"workload": "get_barycentric_weights: %d queries (regular ico6 vertices) on a warped ico6 mesh (81 920 triangles, fresh octree)" % N,
           "queries_per_s_kernel": N / kern_s, "kernel_us": kern_s * 1e6, "queries_per_s_call": N / call_s, "us_per_call": call_s * 1e6, "calls": calls,
           "call": "msm_query_triangles with the four arrays in pinned memory of the context (msm_host_alloc), ABI layout: the kernel reads the queries and writes the "
                   "three result arrays where the caller has them (mapped memory, over PCIe in both directions at once), a raised status in a mapped flag: one kernel, "
                   "one synchronisation (round 4: a copy command in, the kernel, three out, a status copy)",
           "kernel_us_of_the_call": float(np.median(kd)) * 1e6,
           "kernel_us_definition": "kernel_us: the search kernel with queries and results in HBM (the wrapper's call; what the roofline is priced on); "
                                   "kernel_us_of_the_call: the same kernel reading and writing the caller's mapped arrays, 64 B per query over PCIe",
           "us_per_call_python_wrapper": float(np.median(pt)) * 1e6,
           "python_wrapper": "Mesh.query_triangles on pageable numpy arrays: (N,3) <-> 3 x N transposes, three allocations and a staging memcpy each way on top",
           "roofline": {"bound": "hbm", "achieved": nbytes / kern_s / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": nbytes / kern_s / 1e9 / HBM_PEAK_GBS,
                        "kernel": "msm::k_query<%d>" % ctx.query_lanes(N), "algorithmic_bytes_per_launch": nbytes,
                        "note": "kernel time = HIP events around the launch on its stream; a launch of this size (2 561 wavefronts) is a dependent chain of "
                                "memory accesses per query (query, grid cell, node, cones, triangle id, record), not a stream: see DESIGN.md section 5.1"}}
    if cpu:
        from oracle import oracle as O

        om = O.Mesh(warped, tri)
        tree = O.Octree(om)
        t0 = time.perf_counter()
        st, otri, ovid, ow = tree.barycentric_weights(xyz)
        dt = time.perf_counter() - t0
        out["cpu_port"] = {"queries_per_s": N / dt, "cores": 1, "sample": "the same %d queries, one thread (the reference's callers pass nthreads = 1, R/resampler.cpp:75,78)" % N,
                           "triangles_identical": bool(np.array_equal(otri, t_id)), "weights_identical": bool(np.array_equal(ow, w))}
    mesh.close()
    return out


def registration_check(ctx, levels, D, note, **kw):
    """The same registration with fewer iterations per level over the MI355X path and over the CPU port (tests/helpers.py:
    registration_parity -- the checker of tests/test_gpu_registration.py): north_star's bar is 1e-4 rad between the registered spheres."""
    from tests.helpers import registration_parity

    r = registration_parity(ctx, levels, D, **kw)
    return {"max_angle_rad_vs_cpu_port": r["max_angle_rad"], "labelings_identical": r["labelings_identical"], "labelings_compared": r["labelings"],
            "energies_max_rel_diff": r["energies_rel_diff"], "cpu_port_s": r["cpu_port_s"], "run": note, "tolerance_rad": 1e-4}


def bench_registration(ctx, optimiser="mcmc", check=True):
    """Wall-clock of a pairwise registration (tools/time_registration.py): three DISCRETE levels as in config/basic_configs (data grids
    ico4/5/6, control grids ico2/3/4, sigma 4/2/1, variance normalisation), 3 iterations per level, input and reference spheres ico6."""
    import newmsm_amd as M
    from newmsm_amd import registration, synthetic

    xyz, tri = M.make_mesh_from_icosa(6)
    ref = synthetic.features(xyz, 1, 7)
    src = synthetic.features(synthetic.known_warp(xyz, seed=9, rot_deg=3.0, amp=2.0), 1, 7)
    kw = dict(mciters=50, mcparam=0.8, seed=1, cost_params=dict(lambda_=0.1), optimiser=optimiser)
    ops = registration.ProductOps(ctx)
    for _ in range(2):  # the first run pays for allocations
        clock = {}
        t0 = time.perf_counter()
        registration.run_multiresolution(ops, xyz, tri, src, xyz, tri, ref, registration.basic_levels((3, 3, 3)), varnorm=True, timings=clock, **kw)
        wall = time.perf_counter() - t0
    how = ("the library's Monte Carlo optimiser (M/mcmc_opt.h) at 50 sweeps over the unary + T x L^3 triplet tables; FastPD / HOCR are "
           "licence-restricted and FSL-bound: not runnable here") if optimiser == "mcmc" else (
           "driven as --dopt=HOCR drives it (BASELINE config 2): per iteration the unary table and 2 x L fusion moves of 8 T strain costs, the "
           "label loop of Fusion::optimize with a stand-in for its licence-restricted binary solve (msm_fusion_icm_step)")
    out = {"wall_s": wall, "path_s": sum(v for k, v in clock.items() if k != "optimiser"), "phases_s": {k: round(v, 4) for k, v in sorted(clock.items())},
           "workload": "run_multiresolutions, 3 DISCRETE levels (data ico4/5/6, control ico2/3/4), 3 iterations each, sulc-like D=1, ico6 spheres",
           "optimiser": how}
    if check:
        iters = (1, 1, 1) if optimiser == "mcmc" else (2, 2, 2)
        out["check"] = registration_check(ctx, registration.basic_levels(iters), 1, "the same schedule and subject, %d iteration(s) per level" % iters[0], **kw)
        out["max_angle_rad_vs_cpu_port"] = out["check"]["max_angle_rad_vs_cpu_port"]
    return out


def bench_registration_msmall(ctx, check=True):
    """Wall-clock of an HCP MSMAll-shaped pairwise registration (BASELINE config 3): the schedule of
    config/HCP_multimodal_alignment/MSMAllStrainFinalconf1to1_1to3_2 -- three levels, 10 / 15 / 15 iterations, triclique cost over 32
    features, rescaled labels, variance normalisation -- on ico6 spheres, driven as --dopt=HOCR drives it: per iteration one set-up and
    2 x L fusion moves (tools/time_registration_msmall.py)."""
    import newmsm_amd as M
    from newmsm_amd import registration, synthetic

    xyz, tri = M.make_mesh_from_icosa(6)
    ref = synthetic.features(xyz, 32, 7)
    src = synthetic.features(synthetic.known_warp(xyz, seed=9, rot_deg=3.0, amp=2.0), 32, 7)
    ops = registration.ProductOps(ctx)
    for _ in range(2):  # the first run pays for allocations
        clock = {}
        t0 = time.perf_counter()
        registration.run_multiresolution(ops, xyz, tri, src, xyz, tri, ref, registration.hcp_msmall_levels(), varnorm=True, timings=clock)
        wall = time.perf_counter() - t0
    out = {"wall_s": wall, "path_s": sum(v for k, v in clock.items() if k != "optimiser"), "phases_s": {k: round(v, 4) for k, v in sorted(clock.items())},
           "workload": "run_multiresolutions, the HCP MSMAll schedule (data ico4/5/6, control ico2/3/4, 10 / 15 / 15 iterations, ho_multivariate D=32, "
                       "--triclique --rescaleL --VN), ico6 spheres: 40 set-ups + 1 520 fusion moves",
           "optimiser": "the label loop of Fusion::optimize with a stand-in for its binary solve (msm_fusion_icm_step: iterated conditional modes on the "
                        "host; ELC + FastPD are licence-restricted and FSL-bound): the path is exercised and timed as HOCR drives it, the labelings are "
                        "not HOCR's"}
    if check:
        # The WHOLE schedule once over the CPU port (VERDICT r4 missing 2: north_star's ">= 50x the reference multicore-CPU wall-clock on a full ico6 HCP MSMAll
        # pairwise registration" needs this round's CPU wall-clock beside this round's GPU one): the same caller loop, the same stand-in solve, the oracle's
        # OpenMP evaluators on this box's cores -- and with it the parity of all 40 iterations, not of one per level
        from tests.helpers import ORACLE_THREADS

        out["check"] = registration_check(ctx, registration.hcp_msmall_levels(), 32, "the same schedule and subject, every iteration (10 / 15 / 15)")
        out["max_angle_rad_vs_cpu_port"] = out["check"]["max_angle_rad_vs_cpu_port"]
        out["cpu_port_wall_s"] = out["check"]["cpu_port_s"]
        out["cpu_port_cores"] = ORACLE_THREADS
        out["vs_cpu_port_wall"] = out["cpu_port_wall_s"] / wall
        out["cpu_port_note"] = ("the full schedule over oracle/ (kind: port; OpenMP over control points / control triangles as the reference's loops, %d threads; "
                                "MSM_ORACLE_THREADS) -- the port is the faster of the two where it differs from the reference, so the ratio is understated; north_star's "
                                "target is >= 50x" % ORACLE_THREADS)
    return out


def bench_registration_gmsm(ctx, S=8, iters=2):
    """A groupwise registration as its caller loop runs it (BASELINE config 5's shape at a size a default bench run affords): Group_Mesh_registration::
    run_multiresolutions (M/group_mesh_registration.cpp:26-133) over newmsm_amd/group_registration.py -- per level the featurespace of all S subjects,
    from level 2 on project_CPgrid per subject, per iteration setupCostFunction, 2 x L label steps (4 P pair + 8 T triplet costs each), applyLabeling,
    unfold / warp / unfold per subject.  The `gmsm` object times the cost-function side at S = 64; this one is the whole loop at S = 8."""
    import numpy as np

    import newmsm_amd as M
    from newmsm_amd import group_registration as GR
    from newmsm_amd import synthetic

    xyz, tri = M.make_mesh_from_icosa(6)
    txyz = synthetic.known_warp(xyz, seed=33, rot_deg=7.0, amp=1.5)  # (an irregular template: DESIGN.md section 3)
    meshes = [(synthetic.known_warp(xyz, seed=40 + s, rot_deg=0.0, amp=1.0), tri) for s in range(S)]
    datas = [synthetic.features(synthetic.known_warp(meshes[s][0], seed=90 + s, rot_deg=3.0, amp=2.0), 2, seed=5) for s in range(S)]
    levels = [dict(data_order=d, cp_order=c, sg_order=c + 2, iters=iters, simmeasure=2, sigma_in=sg, cost_params=dict(lambda_=1.0, mu=0.4, kappa=1.6))
              for d, c, sg in ((4, 2, 4.0), (5, 3, 2.0), (6, 4, 1.0))]
    ops = GR.ProductGroupOps(ctx)
    for _ in range(2):  # the first run pays for allocations
        clock, labs = {}, []
        t0 = time.perf_counter()
        regs, _, energies = GR.run_group_multiresolution(ops, meshes, datas, txyz, tri, levels, varnorm=True, fixnan=True, timings=clock, labelings_out=labs)
        wall = time.perf_counter() - t0
    moved = max(float(np.abs(regs[s] - meshes[s][0]).max()) for s in range(S))
    return {"wall_s": wall, "path_s": sum(v for k, v in clock.items() if k != "optimiser"), "phases_s": {k: round(v, 4) for k, v in sorted(clock.items())},
            "subjects": S, "label_steps": int(sum(2 * 19 for _ in labs)), "nodes_that_took_a_label": int(sum(int(np.count_nonzero(l)) for l in labs)),
            "largest_move_mm": moved, "energies": [[round(e, 6) for e in lv] for lv in energies],
            "workload": "run_multiresolutions of a groupwise registration: %d synthetic subjects (D=2) on ico6 spheres of their own, an irregular ico6 template, levels data ico4/5/6 / "
                        "control ico2/3/4 (sigma 4/2/1, --VN --fixnan, lambda 1.0: with the stand-in solve a weaker regulariser folds the meshes, and unfold's up to 1 000 repair passes per mesh -- M/reg_tools.cpp:59-178 -- take over the run), %d iteration(s) per level" % (S, iters),
            "optimiser": "the label loop of Fusion::optimize with the stand-in binary solve (msm_fusion_icm_step), as in registration_msmall; its time is wall_s - path_s"}


BASIC_FUSION_CONFIG = """# three DISCRETE levels shaped like config/basic_configs/config_standard_MSM_strain (its AFFINE level left out), driven as --dopt=HOCR drives BASELINE config 2
--opt=DISCRETE,DISCRETE,DISCRETE
--simval=2,2,2
--sigma_in=4,2,1
--sigma_ref=4,2,1
--lambda=0.1,0.1,0.1
--it=3,3,3
--CPgrid=2,3,4
--SGgrid=4,5,6
--datagrid=4,5,6
--dopt=HOCR
--regoption=3
--VN
"""


def bench_registration_cpp(ctx, config_text, D, what, check=True):
    """The same registration with the host side in C++ (north_star: "host code stays C++ and calls HIP through a thin C-ABI"): tools/cpp/registration_bench
    -- include/msmhip_registration.hpp: run_multiresolutions + include/msmhip_config.hpp over include/msmhip.hpp over the C ABI -- run as a child process
    on the bench's synthetic subject with the schedule read from `config_text`; compared with the Python-driven loop (newmsm_amd/registration.py) over
    the same schedule: identical labelings, registered spheres within 1e-4 rad.  Matches M/mesh_registration.cpp:30-50,164-232, I/Fusion/Fusion.h:136-229."""
    import subprocess
    import tempfile

    import numpy as np

    import __graft_entry__ as g
    import newmsm_amd as M
    from newmsm_amd import config, registration, synthetic
    from newmsm_amd.bag import read_bag, write_bag

    exe = g.build_cpp_host()
    xyz, tri = M.make_mesh_from_icosa(6)
    ref = synthetic.features(xyz, D, 7)
    src = synthetic.features(synthetic.known_warp(xyz, seed=9, rot_deg=3.0, amp=2.0), D, 7)
    with tempfile.TemporaryDirectory() as tmp:
        bag, outbag, conf = os.path.join(tmp, "in.bag"), os.path.join(tmp, "out.bag"), os.path.join(tmp, "conf")
        write_bag(bag, orders=np.array([6, D], dtype=np.int32), in_data=src, ref_data=ref)
        with open(conf, "w") as f:
            f.write(config_text)
        p = subprocess.run([exe, bag, outbag, conf, "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        if p.returncode != 0:
            return {"error": p.stderr[-1000:]}
        out = json.loads(p.stdout.strip().splitlines()[-1])
        res = read_bag(outbag)
    out["phases_s"] = {k: round(v, 4) for k, v in sorted(out["phases_s"].items())}
    out["workload"] = what
    out["host"] = "C++: tools/cpp/registration_bench (include/msmhip_registration.hpp + msmhip_config.hpp over the C ABI), a child process of bench.py; second of two runs"
    out["move_call_minus_kernel_us"] = out["move_us_per_call"] - out["move_kernel_us"] if out["moves_timed"] else None
    if check:  # the Python-driven loop over the same schedule and subject
        levels, run_kw, _ = config.levels_from_config(config.parse_config(config_text), D)
        labs = []
        ops = registration.ProductOps(ctx)
        sphere, _, _ = registration.run_multiresolution(ops, xyz, tri, src, xyz, tri, ref, levels, labelings_out=labs, **run_kw)
        got = res["sphere_reg"].reshape(-1, 3)
        cosang = np.clip(np.sum(got * sphere, axis=1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(sphere, axis=1)), -1.0, 1.0)
        flat = np.concatenate(labs) if labs else np.zeros(0, dtype=np.int32)
        out["check"] = {"labelings_identical_to_the_python_run": bool(len(flat) == len(res["labelings"]) and np.array_equal(flat, res["labelings"])),
                        "labelings_compared": len(labs), "max_angle_rad_vs_python_run": float(np.max(np.arccos(cosang))), "tolerance_rad": 1e-4}
    return out


GMSM_LEVELS = [(4, 2), (5, 3), (6, 4)]  # --datagrid / --CPgrid of the gMSM configuration of docs/guide.md:390-407
GMSM_ITERATIONS = 9                      # --it=9,9,9


GMSM_PMC_PROFILE = os.path.join("profiles", "r5_gstep_pmc.json")
FP64_VALU_PEAK = 1024 * 2.4e9 / 4  # wave-instructions/s: 256 CUs x 4 SIMDs, a 64-lane FP64 (or any full-rate VALU) instruction every 4 cycles at 2.4 GHz
                                   # (MI355X_MICROARCH.md: 78.6 TFLOP/s FP64 vector = this x 64 lanes x 2 flops)


def gmsm_valu_profile(S, data_order, cp_order):
    """VALU wave-instructions of k_group_pairwise per label step from the committed rocprofv3 PMC passes (SQ_INSTS_VALU per launch x launches
    per step), valid for the profiled configuration only: 64 subjects, ico6 / ico4, the bench's label-change model."""
    if (S, data_order, cp_order) != (64, 6, 4):
        return None
    try:
        with open(os.path.join(ROOT, GMSM_PMC_PROFILE)) as f:
            prof = json.load(f)
        if not profile_is_current(prof):
            return None
        k = [v for name, v in prof["kernels"].items() if "k_group_pairwise" in name][0]
        return {"per_launch": k["per_launch_mean"]["SQ_INSTS_VALU"], "launches_per_step": k["launches_per_step"], "kernel_avg_ns": k["kernel_avg_ns_from_kernel_stats"]}
    except (OSError, KeyError, IndexError, ValueError):
        return None


def gmsm_iteration(ctx, S, data_order, cp_order, comm, label_steps, change=0.10):
    """One iteration of group registration at one level: setupCostFunction (M/DiscreteGroupModel.cpp:163-196) + the cost evaluations of
    Fusion::optimize (2 sweeps x L label steps, I/Fusion/Fusion.h:138-196).  Returns (set-up s, per-label-step s, steps in an iteration)."""
    import numpy as np

    from newmsm_amd import dist as D
    from newmsm_amd import problem

    mine = list(D.shard(S, comm.rank, comm.world))
    g, keep = problem.build_group(ctx, S, data_order, cp_order, D=2, subjects=mine)
    comm.barrier()
    t0 = time.perf_counter()
    D.sharded_group_setup(g, S, comm)  # the first iteration of a level also allocates the group's buffers (kept for the other eight): reported as setup_first_s
    setup_first_s = time.perf_counter() - t0
    setups = []
    for _ in range(3):  # iterations 2 - 4 of a level's nine: the median (the second still sizes a few hints -- list capacities, the forests' depth -- from the first)
        comm.barrier()
        t0 = time.perf_counter()
        D.sharded_group_setup(g, S, comm)  # complete on return (its collectives waited for, the library's stream synchronised); the slowest rank's time counts (max_over_ranks)
        setups.append(time.perf_counter() - t0)
    setup_s = sorted(setups)[1]
    mover = D.ShardedMove(g, comm)
    change_fraction = change
    rng = np.random.default_rng(3)
    lab = rng.integers(0, g.L, g.num_nodes).astype(np.int32)
    for _ in range(3):  # untimed: the first two deliveries into a newly pinned destination are several times slower than the steady state (8-35 ms against 1.9 at ico5 / ico3)
        mover.move(lab, 1)
    # between label steps Fusion changes the labels of the nodes that took the proposal: here a tenth of the nodes per step (the
    # library keeps the (current, current) pair costs of the pairs whose two nodes did not change)
    labs = []
    for i in range(label_steps):
        change = rng.random(g.num_nodes) < change_fraction
        lab = np.where(change, rng.integers(0, g.L, g.num_nodes), lab).astype(np.int32)
        labs.append(lab)
    # an iteration is two sweeps over the labels (I/Fusion/Fusion.h:136-138): half of its steps propose a label for the second time, and
    # the library then has the (label, label) pair costs of the first visit.  The timed steps keep that ratio: label_steps / 2 labels, twice.
    half = max(1, label_steps // 2)
    proposed = [(2 + i % half) % g.L for i in range(2 * half)]
    # HIP events around each step's kernels (on the context's stream; two event records per step) in the SAME steps: the GPU time of the mix of first and
    # second visits that the delivered time is measured on
    g.time_moves(True)
    comm.barrier()
    t0 = time.perf_counter()
    each, kms = [], []
    for i in range(2 * half):
        t1 = time.perf_counter()
        q, o = mover.move(labs[i % len(labs)], proposed[i])
        each.append(time.perf_counter() - t1)
        kms.append(g.move_kernels_ms())
    comm.barrier()
    step_s = (time.perf_counter() - t0) / (2 * half)
    g.time_moves(False)
    sizes = dict(L=g.L, pairs=g.P, triplets=g.T, nodes=g.num_nodes, step_kernels_s=float(np.mean(kms)) * 1e-3 if kms and min(kms) >= 0 else None,
                 step_ms_each=[round(t * 1e3, 3) for t in each], step_kernels_ms_each=[round(float(k), 3) for k in kms])
    mover.close()
    g.close()
    sizes["setup_first_s"] = setup_first_s
    return setup_s, step_s, 2 * sizes["L"], sizes


def bench_gmsm(ctx, S, comm, label_steps=6, change=0.10):
    from newmsm_amd import dist as D

    levels, total, cold, roofline = [], 0.0, 0.0, None
    for data_order, cp_order in GMSM_LEVELS:
        setup_s, step_s, steps, sizes = gmsm_iteration(ctx, S, data_order, cp_order, comm, label_steps, change)
        setup_s, step_s = D.max_over_ranks(setup_s, comm), D.max_over_ranks(step_s, comm)
        it_s = setup_s + steps * step_s
        total += GMSM_ITERATIONS * it_s
        first_s = D.max_over_ranks(sizes["setup_first_s"], comm)
        cold += GMSM_ITERATIONS * it_s + max(0.0, first_s - setup_s)
        levels.append({"data_order": data_order, "cp_order": cp_order, "setup_s": setup_s, "setup_first_s": first_s, "label_step_s": step_s, "label_step_kernels_s": sizes["step_kernels_s"],
                       "label_steps_per_iteration": steps, "iteration_s": it_s, "pair_evals_per_step": 4 * sizes["pairs"], "triplet_evals_per_step": 8 * sizes["triplets"],
                       "label_step_ms_each": sizes["step_ms_each"], "label_step_kernels_ms_each": sizes["step_kernels_ms_each"]})
        prof = gmsm_valu_profile(S, data_order, cp_order) if comm.world == 1 and change == 0.10 else None
        if prof and sizes["step_kernels_s"]:
            # the label step is priced against FP64 / integer vector issue, not HBM (0.61 GB per launch = 0.06 of the HBM roofline): achieved =
            # the pair kernel's VALU wave-instructions per step (counters of the committed profile) / this run's GPU time of a step
            per_step = prof["per_launch"] * prof["launches_per_step"]
            achieved = per_step / sizes["step_kernels_s"]
            roofline = {"bound": "fp64_valu", "achieved": achieved / 1e9, "peak": FP64_VALU_PEAK / 1e9, "unit": "G wave-instructions/s", "frac": achieved / FP64_VALU_PEAK,
                        "frac_per_step_delivered": per_step / step_s / FP64_VALU_PEAK, "kernel": "msm::k_group_pairwise",
                        "valu_wave_instructions_per_label_step": per_step, "source": GMSM_PMC_PROFILE + ": SQ_INSTS_VALU per launch x launches per step",
                        "step_kernels_ms_events": sizes["step_kernels_s"] * 1e3, "kernel_avg_ms_rocprof": prof["kernel_avg_ns"] * 1e-6,
                        "level": "ico%d / ico%d" % (data_order, cp_order),
                        "note": "a step's GPU time (HIP events around its kernels on the launch stream) also holds the strain triplets and the kept-cost copies.  "
                                "An upper bound on what instruction issue explains, not the binding limit: rewrites that cut the instructions by up to a third left the "
                                "step where it was, a quarter wavefront per pair cost (more dependent chains in flight) took it from 12.5 to 9.3 ms (DESIGN.md 5.6)"}
    # the set-up against the HBM roofline in SURVEY 8(d)'s units: get_patch_data is L adaptive-barycentric resamples per subject = (V + Vt) nearest-triangle
    # queries of 144 B each (forward and reverse weights) + the D x Vt resampled values written, per (subject, label)
    last = levels[-1]
    V6 = 10 * 4 ** last["data_order"] + 2
    setup_bytes = S * 19 * ((V6 + V6) * 144 + 2 * V6 * 8)
    setup_roofline = {"bound": "hbm", "achieved": setup_bytes / last["setup_s"] / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": setup_bytes / last["setup_s"] / 1e9 / HBM_PEAK_GBS,
                      "algorithmic_bytes": setup_bytes, "level": "ico%d / ico%d" % (last["data_order"], last["cp_order"]),
                      "definition": "S x L x ((V + Vt) queries x 144 B + D x Vt x 8 B of resampled features): the resampling a subject's set-up is made of, SURVEY 8(d) units; "
                                    "the 19 search trees per subject (the larger half of the GPU time, DESIGN 5.6), the weight-list surgery and the patch lists have no unit there",
                      "note": "nominal and small by construction: a subject's set-up is ~100 dependent launches over tens of MB that live in L2; the GPU is busy (two set-up "
                              "pipelines side by side gain 8 %), not the memory system"}
    out = {"subjects": S, "levels": levels, "iterations_per_level": GMSM_ITERATIONS, "path_s_per_group": total, "subjects_per_hour": S / total * 3600.0,
           "path_s_per_group_cold": cold, "subjects_per_hour_cold": S / cold * 3600.0,
           "cold_definition": "the same with every level's FIRST set-up as measured (setup_first_s: it allocates the level's buffers -- feature maps, patch values, forests, kept costs -- "
                              "through the pool; a process that registers group after group pays it once per size, a single group pays it three times)",
           "setup_roofline": setup_roofline,
           "config": {"label_change_fraction": change, "label_steps_timed": label_steps,
                      "model": "between label steps that fraction of the nodes changes its label (the library keeps the (current, current) costs of untouched pairs); half of the "
                               "timed steps are second visits of their label, as in the two sweeps of an iteration (I/Fusion/Fusion.h:136-138)"}}
    if roofline:
        out["roofline"] = roofline
    out.update({
            "definition": "cost-function side of a groupwise registration (docs/guide.md:390-407: 3 levels x 9 iterations): per iteration one "
                          "setupCostFunction (get_patch_data for every subject) + 2 x L label steps of 4 P pair + 8 T triplet costs delivered to the optimiser's "
                          "rank; measured on one iteration per level (set-up: the median of the second to fourth call, buffers allocated by the first) and %d label steps (half of them second visits of their label, as in the two sweeps of an iteration) with config.label_change_fraction of the nodes changing their label between steps.  The MRF solve (ELC / FastPD, licence-restricted, serial) is not "
                          "part of the path and not in this figure" % label_steps})
    return out


def gmsm_cpu_port(S, threads, levels, labels_sampled=3, subjects_sampled=None, evals=200000):
    """The CPU leg of the gMSM object (VERDICT r4 missing 2): the oracle's restatement of DiscreteGroupModel::get_patch_data (M/DiscreteGroupModel.cpp:88-121) and
    DiscreteGroupCostFunction::computePairwiseCost / computeTripletCost (M/DiscreteGroupCostFunction.cpp:26-98) timed on this box's host cores on a BOUNDED
    sample of the same synthetic group, and the figure the GPU object reports -- subjects/hour of the cost-function side -- projected from it with the same
    accounting (per iteration one set-up of S subjects + 2 L label steps of 4 P pair and 8 T triplet costs, the reference evaluating all of them: it keeps none).
      set-up   `subjects_sampled` subjects (default: one per thread, the reference's OpenMP loop is over the subjects) x `labels_sampled` of the L labels at
               every level: core-seconds per (subject, label), scaled to S x L
      costs    `evals` pair and `evals` triplet evaluations at random (pair, labels) of the last level's group over all threads, as Fusion::optimize's loops
    The port is the faster of the two in every place it differs from the reference (a merge instead of std::map::find per patch entry, arrays instead of
    NEWMAT objects): the ratio is understated, never overstated."""
    import numpy as np

    from newmsm_amd import api, synthetic
    from oracle import oracle as O

    n_sub = max(2, min(S, subjects_sampled or threads))
    out = {"cores": threads, "kind": "port", "levels": []}
    t_all = time.perf_counter()
    total = 0.0
    rng = np.random.default_rng(5)
    for data_order, cp_order in levels:
        dxyz, dtri = api.make_mesh_from_icosa(data_order)
        cxyz, ctri = api.make_mesh_from_icosa(cp_order)
        _, mvd = api.cp_spacings(cxyz, ctri)
        samples, _ = api.label_sampling_grid(cp_order + 2, 0.5 * mvd)
        L = len(samples)
        og = O.Group(n_sub, simmeasure=2, lambda_=0.2)
        tm, cp = O.Mesh(dxyz, dtri), O.Mesh(cxyz, ctri)
        og.set_template(tm, None)
        og.set_controlgrid(cp)
        keep = [tm, cp]
        for s in range(n_sub):  # problem.build_group's subjects
            feat = synthetic.features(synthetic.known_warp(dxyz, seed=90 + s, rot_deg=2.0, amp=1.0), 2, seed=5)
            m = O.Mesh(dxyz, dtri)
            og.set_subject(s, m, feat)
            m.set_coords(synthetic.known_warp(dxyz, seed=40 + s, rot_deg=1.0 + 0.1 * s, amp=0.5))
            og.set_subject(s, m, feat)
            og.reset_cpgrid(s, synthetic.known_warp(cxyz, seed=40 + s, rot_deg=1.0 + 0.1 * s, amp=0.5))
            keep.append(m)
        ls = min(labels_sampled, L)
        og.set_labels(samples[:ls])
        og.set_threads(threads)
        t0 = time.perf_counter()
        og.setup()
        setup_wall = time.perf_counter() - t0
        # wall x min(threads, subjects) core-seconds went into n_sub x ls (subject, label) units (the loop is over the subjects: at most n_sub threads busy)
        core_s_per_unit = setup_wall * min(threads, n_sub) / (n_sub * ls)
        n = min(evals, 50 * og.P)
        pr, la, lb = rng.integers(0, og.P, n), rng.integers(0, ls, n), rng.integers(0, ls, n)
        t0 = time.perf_counter()
        og.pairwise_batch(pr, la, lb, threads)
        pair_rate = n / (time.perf_counter() - t0)
        tr, a, b, c = rng.integers(0, og.T, n), rng.integers(0, ls, n), rng.integers(0, ls, n), rng.integers(0, ls, n)
        t0 = time.perf_counter()
        og.triplet_batch(tr, a, b, c, threads)
        trip_rate = n / (time.perf_counter() - t0)
        N, Tc = len(cxyz), len(ctri)
        P, T = N * S * (S - 1) // 2, S * Tc
        setup_s = S * L * core_s_per_unit / threads
        step_s = 4 * P / pair_rate + 8 * T / trip_rate
        it_s = setup_s + 2 * L * step_s
        total += GMSM_ITERATIONS * it_s
        out["levels"].append({"data_order": data_order, "cp_order": cp_order, "setup_core_s_per_subject_and_label": core_s_per_unit, "pair_evals_per_s": pair_rate,
                              "triplet_evals_per_s": trip_rate, "projected_setup_s": setup_s, "projected_label_step_s": step_s, "projected_iteration_s": it_s,
                              "sample": "%d subjects x %d labels set up (%.1f s wall), %d pair + %d triplet evaluations" % (n_sub, ls, setup_wall, n, n)})
        del og, keep
    out["projected_path_s_per_group"] = total
    out["projected_subjects_per_hour"] = S / total * 3600.0
    out["sample_wall_s"] = time.perf_counter() - t_all
    out["note"] = ("projected from the bounded sample above with the GPU object's accounting (levels x %d iterations x (set-up of %d subjects + 2 L label steps of 4 P pair "
                   "and 8 T triplet costs)); the whole group on the CPU would take the projected time" % (GMSM_ITERATIONS, S))
    return out


def free_port():
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


class stdout_to_stderr:
    """file descriptor 1 points at stderr inside the block: RCCL prints a version banner on stdout when its first communicator comes up, and the
    contract is ONE JSON line there"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def self_launch(n, argv):
    """`python bench.py --gpus N` with N > 1 outside a launcher: start the N ranks as `python -m torch.distributed.run` would be typed by hand --
    one process per GPU, rendezvous on 127.0.0.1 -- as a CHILD process, pass its output through and exit with its code.  This process has not
    imported torch or touched HIP and never does (a process that has initialised the GPU must not be replaced by or turned into another).
    The reference's own scale-out launches independent processes the same way (gMSM_scripts/group_reg_dataset.sh:9-33: SLURM tasks)."""
    import subprocess

    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ, MSM_BENCH_SELF_LAUNCHED="1")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 1) // n)))
    sys.stdout.flush()
    raise SystemExit(subprocess.call(cmd, env=env))


def bench_template_allreduce(comm, S, V, Dfeat, reps=20):
    """The collective north_star names: the group-mean template update of a groupwise run -- what gMSM_scripts/run_gMSM.sh:66-139 does with files,
    `wb_command -surface-average` and `-metric-reduce MEAN / STDEV` -- as ONE all-reduce(sum) of [sum xyz | sum f | sum f^2 | n] over the ranks'
    accumulators (newmsm_amd/dist.py: group_template_update; RCCL over xGMI with the nccl backend).  Every rank holds the registered spheres and
    resampled features of ITS subjects (synthetic here: subject s contributes the constant s + 1, so the reduced sums are known)."""
    import numpy as np
    import torch

    from newmsm_amd import dist as D

    mine = list(D.shard(S, comm.rank, comm.world))
    n = 3 * V + 2 * Dfeat * V + 1
    out = {"bytes": 8 * n, "ranks": comm.world, "subjects": S, "layout": "[sum xyz 3V | sum f DV | sum f^2 DV | n] f64, V = %d, D = %d" % (V, Dfeat),
           "collective": "none (one process, no communicator)" if comm.dist is None else "all_reduce(sum), backend %s, tensors on %s" % (comm.backend, comm.device)}
    spheres = np.empty((len(mine), V, 3))
    feats = np.empty((len(mine), Dfeat, V))
    for k, s in enumerate(mine):
        spheres[k], feats[k] = s + 1.0, s + 1.0
    t0 = time.perf_counter()
    res = D.group_template_update(spheres, feats, comm)
    out["us_call_first"] = (time.perf_counter() - t0) * 1e6
    ok = res["n_subjects"] == S and np.allclose(res["mean"], (S + 1) / 2.0)
    if comm.dist is not None:
        acc = torch.ones(n, dtype=torch.float64, device=comm.device)
        ts = []
        for _ in range(reps):
            acc.fill_(1.0)
            if comm.on_gpu:
                torch.cuda.synchronize()
            comm.barrier()
            t0 = time.perf_counter()
            comm.dist.all_reduce(acc, op=comm.dist.ReduceOp.SUM)
            if comm.on_gpu:
                torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        ok = ok and bool((acc == float(comm.world)).all().item())
        out["us"] = D.max_over_ranks(float(np.median(ts)), comm) * 1e6
        out["us_definition"] = "median of %d all-reduces of the accumulator tensor, issue to completion on the slowest rank" % reps
    t0 = time.perf_counter()
    D.group_template_update(spheres, feats, comm)
    out["us_call"] = D.max_over_ranks(time.perf_counter() - t0, comm) * 1e6
    out["us_call_definition"] = "group_template_update: local sums on the host, upload, the all-reduce, download, mean sphere / mean / stdev"
    out["sums_correct"] = bool(ok)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=["pairwise", "gmsm"], default="pairwise")
    ap.add_argument("--data-order", type=int, default=6)
    ap.add_argument("--cp-order", type=int, default=4)
    ap.add_argument("--dims", type=int, default=1)
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--label-change", type=float, default=0.10, help="gMSM: fraction of the nodes whose label changes between two label steps")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline: the steady and roofline figures, the extra objects, the CPU "
                                                        "baseline (without it a run sets up, warms up, times --steps steps and prints the headline line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline and the CPU legs of the extra objects")
    ap.add_argument("--no-extras", action="store_true", help="--full without the extra objects (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last step computed to DIR/<name>.npy (pairwise mode: "
                                                          "rank 0's unary cost table, L x N float64)")
    ap.add_argument("--dry-launch", action="store_true", help="launch the ranks, create the communicator, count the ranks through it, print that and stop "
                                                              "(no GPU work: the check that --gpus N really starts N ranks; gloo when no GPU is visible)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and args.mode != "pairwise":
        ap.error("--dump-outputs is implemented for --mode pairwise only")

    # --gpus N outside a launcher: become the launcher's parent BEFORE torch or HIP are touched (the driver's N = 1 command shape with N > 1)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus, sys.argv[1:])

    import numpy as np
    import torch

    from newmsm_amd import dist as D

    t_start = time.perf_counter()
    rank, local_rank, world = D.env()
    if world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the launcher started %d rank(s) (WORLD_SIZE): the line would misreport n_gpus" % (args.gpus, world))
    if args.dry_launch:
        gpu = torch.cuda.is_available() and os.environ.get("MSM_BENCH_REHEARSAL") != "1"
        with stdout_to_stderr():
            comm = D.init("nccl" if gpu else "gloo", local_rank if gpu else None)
            seen = D.count_ranks(comm)
        ranks = D.all_reduce_sum(np.eye(world)[rank], comm)
        tmpl = bench_template_allreduce(comm, 64, 2562, 2, reps=3)
        if rank == 0:
            print(json.dumps({"dry_launch": True, "n_gpus": seen, "world": world, "gpus_asked": args.gpus, "backend": comm.backend,
                              "every_rank_reported": bool((ranks == 1.0).all()), "self_launched": os.environ.get("MSM_BENCH_SELF_LAUNCHED") == "1",
                              "template_allreduce": tmpl}))
        comm.close()
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product path has no CPU fallback")
    # rehearsal of the N > 1 path on a one-GPU box: all ranks share cuda:0 and talk over gloo
    rehearse = os.environ.get("MSM_BENCH_REHEARSAL") == "1"
    device_index = 0 if rehearse else local_rank
    torch.cuda.set_device(device_index)
    # MSM_BENCH_FORCE_DIST=1: a one-rank process group, so that a one-GPU box runs the RCCL collectives of the N > 1 path
    force = os.environ.get("MSM_BENCH_FORCE_DIST") == "1"
    with stdout_to_stderr():
        comm = D.init("gloo" if rehearse else "nccl", device_index) if (world > 1 or force) else D.Comm()
        n_gpus = D.count_ranks(comm)  # an all-reduce of ones over the communicator: the ranks RCCL saw (also brings the communicator up)

    import __graft_entry__ as g

    if rank == 0:
        g.build()
    comm.barrier()
    import newmsm_amd as M
    from newmsm_amd import problem

    stream = torch.cuda.Stream()
    ctx = M.Context(device_index, stream=stream.cuda_stream)

    def sync_all():
        comm.barrier()
        torch.cuda.synchronize()

    if n_gpus != args.gpus:
        raise SystemExit("bench.py: the communicator has %d rank(s), --gpus says %d" % (n_gpus, args.gpus))

    def template_allreduce():
        """gmsm.template_allreduce: the group-mean template update at ico6, D = 2 over this run's communicator; a single process makes a
        one-rank RCCL communicator for it, so that the N = 1 line shows the same call"""
        try:
            if comm.dist is not None:
                return bench_template_allreduce(comm, args.subjects, 40962, 2)
            os.environ["MASTER_PORT"] = str(free_port())
            with stdout_to_stderr():
                one = D.init("nccl", device_index)
                try:
                    return bench_template_allreduce(one, args.subjects, 40962, 2)
                finally:
                    one.close()
        except Exception as e:  # reported, not fatal
            return {"error": repr(e)}

    if args.mode == "gmsm":
        # strong scaling: the same 64-subject group whatever N.  One "step" = the cost-function side of one iteration at the last level
        # (ico6 / ico4); --warmup iterations untimed, --steps timed ones are folded into the per-level measurement (set-up once per level)
        sync_all()
        t0 = time.perf_counter()
        res = bench_gmsm(ctx, args.subjects, comm, label_steps=max(2, min(args.steps, 8)), change=args.label_change)
        if args.full:
            res["template_allreduce"] = template_allreduce()
        sync_all()
        if rank == 0:
            last = res["levels"][-1]
            print(json.dumps({
                "metric": "gMSM subjects/hour", "value": res["subjects_per_hour"], "unit": "subjects/hour", "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
                "ms_per_step": last["iteration_s"] * 1e3, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": "gMSM groupwise, %d synthetic subjects (D=2), levels data ico4/5/6 / control ico2/3/4, %d iterations per level, sharded over %d GPU(s) "
                                       "(BASELINE config 5); a step = one iteration at ico6 / ico4" % (args.subjects, GMSM_ITERATIONS, world),
                           "sharding": "set-up by subject (all-gather of resampled feature maps + patch lists), label steps by clique (each rank's GPU copies its slice into host memory shared with rank 0; a gather across nodes)"},
                "gmsm": res, "bench_wall_s": time.perf_counter() - t0,
            }))
        comm.close()
        ctx.close()
        return

    kind = "univariate" if args.dims == 1 else "multivariate"
    # one synthetic subject per rank (different warp / feature phase)
    inp = problem.pairwise_inputs(args.data_order, args.cp_order, D=args.dims, seed=1234 + 17 * rank)
    cf, keep = problem.build_cost(ctx, inp, kind=kind)
    cf.get_source_data()
    # many tables against one target: have the target's direction table in place before the first step (by default it is built
    # in the background while the complete search serves the first tables, DESIGN.md section 5.2: 14 ms of host time, once per
    # resolution level -- reported below as set-up, not part of a step)
    t0 = time.perf_counter()
    keep["target"].prepare_search(wait=True)
    raytable_ms = (time.perf_counter() - t0) * 1e3
    ptr, _ = cf.patches()
    evals = cf.L * cf.N
    samples = cf.L * int(ptr[-1])
    U = ctx.host_array((cf.L, cf.N))  # pinned: the table's copy to the host is one copy-engine command

    with torch.cuda.stream(stream):
        for _ in range(args.warmup):
            cf.computeUnaryCosts(U)
        sync_all()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            cf.computeUnaryCosts(U)  # rotations + table kernels + table on the host, synchronous: what an iteration pays
        sync_all()
        wall = time.perf_counter() - t0
    if not np.isfinite(U).all() and not os.environ.get("MSM_BENCH_NOCHECK"):
        raise SystemExit("non-finite unary costs")
    Ucopy = np.array(U)  # the table of the last timed step
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "unary_costs.npy"), Ucopy)  # (labels, control points) float64, as computeUnaryCosts delivers it

    wall = D.max_over_ranks(wall, comm)
    if args.full:
        cf.enable_timing(True)  # HIP events around the dominant kernel of every launch, on the launch stream
        with torch.cuda.stream(stream):
            # the kernels alone, enqueued back to back (no rotation kernel between them would be wrong: every call recomputes it)
            for _ in range(args.warmup):
                cf.computeUnaryCosts_async()
            ctx.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ts = time.perf_counter()
            e0.record(stream)
            for _ in range(args.steps):
                cf.computeUnaryCosts_async()
            e1.record(stream)
            ctx.synchronize()
            steady_wall = time.perf_counter() - ts
        step_ms = e0.elapsed_time(e1) / args.steps  # HIP events on the launch stream: rotations + the three table kernels
        kt = cf.kernel_times()[-min(args.steps, 64):]
        kernel_ms = float(np.mean(kt))  # the sampling kernel alone (the dominant kernel), last <= 64 launches of the back-to-back run
        kernel_ms = D.max_over_ranks(kernel_ms, comm)
    # N > 1: the pairwise headline above is N independent replicas (weak scaling, no collective).  The path that does shard is the
    # groupwise one, so a --full run also measures it -- the SAME 64-subject group on N GPUs (strong scaling: set-up by subject with
    # the RCCL all-gathers, label steps by clique) -- and reports it next to the headline; compare with "gmsm" of the N = 1 line.
    gmsm_scaling = None
    if world > 1 and args.full and not args.no_extras and os.environ.get("MSM_BENCH_GMSM_SCALING", "1") != "0":
        try:
            gmsm_scaling = bench_gmsm(ctx, args.subjects, comm, change=args.label_change)
            gmsm_scaling["scaling"] = "strong"
            gmsm_scaling["template_allreduce"] = template_allreduce()
        except Exception as e:  # reported, not fatal: the headline of this run stands
            gmsm_scaling = {"error": repr(e)}

    if rank == 0:
        value = world * evals * args.steps / wall
        out = {
            "metric": "label-cost evals/sec",
            "value": value,
            "unit": "evals/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": wall / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic",
            "config": {
                "workload": "pairwise sulc (D=%d) unary label-cost table, ico%d data grid / ico%d control grid, %d labels, "
                            "%d evals = %d point samples per step (BASELINE config 2)" % (args.dims, args.data_order, args.cp_order, cf.L, evals, samples),
                "kind": kind, "simmeasure": "correlation", "replicas": world,
                "step": "label rotations + sampling / fix-up / reduction kernels + the table copied to pinned host memory, one synchronous call",
                "setup_not_in_step_ms": {"direction_table_of_the_target_once_per_level": raytable_ms},
            },
        }
        if args.full:
            abytes = algorithmic_bytes(samples, evals, args.dims)
            kbytes = kernel_algorithmic_bytes(samples, evals, args.dims)
            achieved = kbytes / (kernel_ms * 1e-3) / 1e9
            out["steady"] = {"ms_per_step": steady_wall / args.steps * 1e3, "value": world * evals * args.steps / steady_wall,
                             "definition": "table kernels (incl. the rotation kernel) enqueued back to back, no copy of the table to the host, one synchronisation at the end"}
            out["roofline"] = {
                "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "traffic": pmc_traffic(args), "traffic_source": PMC_PROFILE + " (rocprofv3 --pmc passes of tools/collect_profile.sh, round 5)",
                "kernel": DOMINANT_KERNEL, "kernel_ms": kernel_ms, "algorithmic_bytes_per_launch": kbytes,
                "binding": pmc_binding_limits(args, kernel_ms),
                "note": "nominal: the level's working set (tens of MB) lives in L2 / Infinity Cache, counter traffic is far below the algorithmic bytes; "
                        "the kernel is bound by the L1 lookup rate of its divergent gathers (DESIGN.md section 5.2)",
                # the whole table (rotation + sampling + fix-up + reduction kernels, HIP events around one step) against the full 8(d) figure
                "step_ms_events": step_ms, "algorithmic_bytes_per_table": abytes,
                "table_achieved": abytes / (step_ms * 1e-3) / 1e9, "table_frac": abytes / (step_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
            }
        if gmsm_scaling is not None:
            out["gmsm"] = gmsm_scaling
        threads = D.host_cores()  # cgroup / affinity aware: the GPU box gives one GPU's share of the host
        os.environ.setdefault("MSM_ORACLE_THREADS", str(threads))  # the CPU legs of the registration objects (tests/helpers.py reads it on import)
        def stage(name):  # MSM_BENCH_TRACE=1: the object being measured, on stderr as it starts (which one was running when a run ended early)
            if os.environ.get("MSM_BENCH_TRACE"):
                print("[bench %.1f s] %s" % (time.perf_counter() - t_start, name), file=sys.stderr, flush=True)

        if world == 1 and args.full and not args.no_extras:
            with torch.cuda.stream(stream):
                stage("triclique_move")
                out["triclique_move"] = {"d1": bench_triclique_move(ctx, 1, 200, 0 if args.no_cpu_baseline else threads),
                                         "d32": bench_triclique_move(ctx, 32, 200, 0 if args.no_cpu_baseline else threads)}
                stage("resample")
                out["resample"] = bench_resample(ctx, 100, not args.no_cpu_baseline)
                chk = not args.no_cpu_baseline  # the checks run the CPU port (a few seconds each)
                stage("registration")
                out["registration"] = bench_registration(ctx, check=chk)
                stage("registration_fusion")
                out["registration_fusion"] = bench_registration(ctx, "fusion", check=chk)
                stage("registration_msmall")
                out["registration_msmall"] = bench_registration_msmall(ctx, check=chk)
                from newmsm_amd import config as _config

                stage("registration_*_cpp")
                out["registration_fusion_cpp"] = bench_registration_cpp(ctx, BASIC_FUSION_CONFIG, 1, "run_multiresolutions, 3 DISCRETE levels (data ico4/5/6, control ico2/3/4, "
                                                                        "sigma 4/2/1, --VN), 3 iterations each, sulc-like D=1, ico6 spheres, --dopt=HOCR --regoption=3 (stand-in solve)")
                out["registration_msmall_cpp"] = bench_registration_cpp(ctx, _config.PRESETS["HCP_MSMAll"], 32, "run_multiresolutions, the HCP MSMAll schedule "
                                                                        "(config text through the reference's grammar), ho_multivariate D=32, ico6 spheres: 40 set-ups + 1 520 fusion moves (stand-in solve)")
                stage("registration_gmsm")
                try:
                    out["registration_gmsm"] = bench_registration_gmsm(ctx)
                except Exception as e:  # reported, not fatal
                    out["registration_gmsm"] = {"error": repr(e)}
                stage("gmsm")
                out["gmsm"] = bench_gmsm(ctx, args.subjects, comm, change=args.label_change)
                stage("gmsm.template_allreduce")
                out["gmsm"]["template_allreduce"] = template_allreduce()
                if not args.no_cpu_baseline:
                    stage("gmsm.cpu_port")
                    out["gmsm"]["cpu_port"] = gmsm_cpu_port(args.subjects, threads, GMSM_LEVELS)
                    out["gmsm"]["vs_cpu_port"] = out["gmsm"]["subjects_per_hour"] / out["gmsm"]["cpu_port"]["projected_subjects_per_hour"]
        if world == 1 and args.full and not args.no_cpu_baseline:
            Uo, rate, dt, reps = cpu_baseline(inp, kind, threads)
            out["cpu_baseline"] = {
                "value": rate, "unit": "evals/s", "cores": threads, "kind": "port",
                "sample": "%d full unary tables (%d evals each, %.1f s in total) of the same workload, OpenMP over control points" % (reps, Uo.size, dt),
                "max_abs_diff_vs_gpu": float(np.max(np.abs(Uo - Ucopy))),
            }
        print(json.dumps(out))
    comm.close()
    ctx.close()


if __name__ == "__main__":
    main()
