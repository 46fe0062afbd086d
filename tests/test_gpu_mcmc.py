"""The Monte Carlo optimiser's sweeps on the GPU (msm_mcmc_optimise_gpu, msm_cost_mcmc_optimise; newmsm_amd/csrc/mcmc.cpp, mcmc_kernels.hip): one workgroup
walks the triplets level by level with the labelling in LDS and takes its proposals from the host's own stream.  Every case asks for the labelling of the
host optimiser (msm_mcmc_optimise) on the same arguments, exactly."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic

from helpers import angles

pytestmark = pytest.mark.gpu
HCP = dict(rmode=3, lambda_=0.01, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)
CHUNK = "MSMHIP_MCMC_CHUNK_SWEEPS"


@functools.lru_cache(maxsize=None)
def _faces(order):
    xyz, tri = M.make_mesh_from_icosa(order)
    return len(xyz), np.ascontiguousarray(api.estimate_triplets(tri), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _random_case(order, L, sweeps, seed=7, mcparam=0.3):
    """random tables on the faces of an icosphere and the host optimiser's labelling for them (computed once, never written)"""
    N, triplets = _faces(order)
    rng = np.random.default_rng(100 + order)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = np.zeros(N, dtype=np.int32)
    want = api.mcmc_optimise(U, tc, triplets, start, mcparam=mcparam, iters=sweeps, seed=seed)
    for a in (U, tc, triplets, start, want):
        a.setflags(write=False)
    return U, tc, triplets, start, want, dict(mcparam=mcparam, iters=sweeps, seed=seed)


def _both(ctx, U, tc, triplets, start, **kw):
    want = api.mcmc_optimise(U, tc, triplets, start, **kw)
    got = api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    return got


@pytest.mark.parametrize("chunk", ["1", "3", None])
@pytest.mark.parametrize("order", [0, 2])
def test_random_tables_on_icosphere_faces(ctx, monkeypatch, order, chunk):
    """T = 20 and T = 320, 19 labels, 50 sweeps; a chunk of one sweep, of three (the last one shorter) and the default (the whole run in one)"""
    if chunk is None:
        monkeypatch.delenv(CHUNK, raising=False)
    else:
        monkeypatch.setenv(CHUNK, chunk)
    U, tc, triplets, start, want, kw = _random_case(order, 19, 50)
    got = api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw)
    assert np.array_equal(got, want) and len(np.unique(want)) > 3  # (the sweeps did move the labelling)
    stats = api.mcmc_gpu_stats(ctx)
    assert stats["chunks"] == {"1": 50, "3": 17, None: 1}[chunk]
    assert stats["levels_per_sweep"] == {0: 10, 2: 28}[order] and stats["levels"] == 50 * stats["levels_per_sweep"]


def test_a_single_chain_reports_as_one_chain_either_draw(ctx, monkeypatch):
    """T = 320, 19 labels, 50 sweeps in chunks of three: the single-chain call is the chains' path with K = 1 and reports what it always did, with the
    proposals drawn on the host and on the device; a following call without sweeps returns at once and leaves the stats"""
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start, want, kw = _random_case(2, 19, 50)
    assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw), want)
    stats = api.mcmc_gpu_stats(ctx)
    assert api.mcmc_chains_info(ctx) == (1, 1)
    assert stats["chunks"] == 17 and stats["levels_per_sweep"] == 28 and stats["levels"] == 1400 and stats["draw_ms"] > 0
    ctx.set_mcmc_draw(1)
    try:
        assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw), want)
        stats = api.mcmc_gpu_stats(ctx)
        assert api.mcmc_chains_info(ctx) == (1, 0)
        assert stats["chunks"] == 17 and stats["levels_per_sweep"] == 28 and stats["levels"] == 1400 and stats["draw_ms"] == 0
        assert api.mcmc_draw_stats(ctx)["accepted"] == 50 * 320
        assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **dict(kw, iters=0)), start)
        assert api.mcmc_gpu_stats(ctx) == stats and api.mcmc_chains_info(ctx) == (1, 0)
    finally:
        ctx.set_mcmc_draw(0)


def test_ico4_faces(ctx, monkeypatch):
    """T = 5120: the widest level holds 320 triplets"""
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start, want, kw = _random_case(4, 5, 4)
    assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw), want) and want.any()
    stats = api.mcmc_gpu_stats(ctx)
    assert stats["levels_per_sweep"] == 32 and stats["widest_level"] == 320 and stats["chunks"] == 2


def test_a_level_wider_than_the_workgroup(ctx, monkeypatch):
    """1500 mutually disjoint triplets are one level of 1500: walked in strides; 1500 more reuse their nodes in reverse order (a second level)"""
    monkeypatch.setenv(CHUNK, "3")
    first = np.arange(4500, dtype=np.int32).reshape(1500, 3)
    triplets = np.concatenate([first, np.arange(4500, dtype=np.int32)[::-1].reshape(1500, 3)])
    level, _, off = api.mcmc_schedule(triplets, 4500)
    assert np.diff(off).tolist() == [1500, 1500]
    rng = np.random.default_rng(5)
    L = 4
    got = _both(ctx, rng.normal(size=(L, 4500)), rng.normal(size=(3000, L, L, L)), triplets, np.zeros(4500, dtype=np.int32), mcparam=0.4, iters=7, seed=3)
    assert len(np.unique(got)) == L and api.mcmc_gpu_stats(ctx)["widest_level"] == 1500


def test_labellings_beyond_64_kb_of_lds_and_beyond_a_workgroup(ctx, monkeypatch):
    """70 000 nodes are 140 000 bytes of labels (the launch asks for more than the 64 KB a kernel gets by default); 80 001 do not fit and are refused"""
    monkeypatch.setenv(CHUNK, "3")
    rng = np.random.default_rng(15)
    N, T, L = 70000, 3000, 3
    triplets = rng.integers(0, N, (T, 3)).astype(np.int32)
    triplets[:, 0] = np.arange(N - T, N)  # the highest nodes are named
    start = rng.integers(0, L, N).astype(np.int32)
    got = _both(ctx, rng.normal(size=(L, N)), rng.normal(size=(T, L, L, L)), triplets, start, mcparam=0.4, iters=5, seed=2)
    assert not np.array_equal(got, start)
    before = api.mcmc_gpu_stats(ctx)
    with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY.*80001 nodes do not fit the LDS"):
        api.mcmc_optimise_gpu(ctx, np.zeros((1, 80001)), np.zeros((1, 1, 1, 1)), [[0, 1, 80000]], np.zeros(80001, dtype=np.int32), iters=1)
    assert api.mcmc_gpu_stats(ctx) == before


def test_lists_that_are_no_mesh_and_empty_runs(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "1")
    rng = np.random.default_rng(6)
    L, N = 6, 9
    # a triplet that names a node twice (and one three times), two identical triplets in a row
    triplets = np.array([[0, 0, 1], [2, 3, 4], [2, 3, 4], [5, 5, 5], [4, 0, 5], [8, 7, 8], [6, 1, 6]], dtype=np.int32)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = rng.integers(0, L, N).astype(np.int32)
    got = _both(ctx, U, tc, triplets, start, mcparam=0.3, iters=25, seed=1)
    assert not np.array_equal(got, start)
    # no triplets, no sweeps: the labelling stays
    assert np.array_equal(_both(ctx, U, np.zeros((0, L, L, L)), np.zeros((0, 3), dtype=np.int32), start, mcparam=0.3, iters=5, seed=1), start)
    assert np.array_equal(_both(ctx, U, tc, triplets, start, mcparam=0.3, iters=0, seed=1), start)
    # one label: every proposal is the label every node already has
    zeros = np.zeros(N, dtype=np.int32)
    assert np.array_equal(_both(ctx, U[:1], tc[:, :1, :1, :1], triplets, zeros, mcparam=0.3, iters=4, seed=1), zeros)


def _count_ties(U, tc, triplets, start, mcparam, iters, seed):
    """the sweeps in plain Python over the proposal stream: (visits, visits in which the lowest of the eight costs is reached more than once, labelling)"""
    L = U.shape[0]
    stream = api.mcmc_proposals(L, mcparam, seed, len(triplets), iters)
    lab = np.array(start, dtype=np.int64)
    visits = ties = 0
    for sweep in stream:
        for t, (a, b, c) in enumerate(triplets):
            p = int(sweep[t])
            cur = (lab[a], lab[b], lab[c])
            costs = []
            for k in range(8):
                la, lb, lc = (p if k & 4 else cur[0]), (p if k & 2 else cur[1]), (p if k & 1 else cur[2])
                with np.errstate(invalid="ignore"):  # (infinities of both signs meet in the NaN case)
                    costs.append(tc[t, la, lb, lc] + (U[la, a] + U[lb, b] + U[lc, c]) / 3.0)
            best = 0  # std::min_element: the first of equal minima; a NaN is never smaller, nothing is smaller than a NaN
            for k in range(1, 8):
                if costs[k] < costs[best]:
                    best = k
            visits += 1
            ties += sum(1 for v in costs if v == costs[best]) > 1
            for bit, n in ((4, a), (2, b), (1, c)):
                if best & bit:
                    lab[n] = p
    return visits, ties, lab.astype(np.int32)


def test_ties_take_the_first_of_equal_costs(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    N, triplets = _faces(1)
    L, kw = 4, dict(mcparam=0.4, iters=30, seed=9)
    rng = np.random.default_rng(8)
    start = rng.integers(0, L, N).astype(np.int32)
    # one constant: all eight costs are equal in every visit, combination 000 wins and nothing moves
    U, tc = np.full((L, N), 1.5), np.full((len(triplets), L, L, L), -0.25)
    assert np.array_equal(_both(ctx, U, tc, triplets, start, **kw), start)
    # small integers (the unary ones multiples of three: exact thirds): exact ties between the eight costs in most visits
    U = 3.0 * rng.integers(0, 2, (L, N))
    tc = 1.0 * rng.integers(0, 2, (len(triplets), L, L, L))
    visits, ties, replay = _count_ties(U, tc, triplets, start, **kw)
    assert visits == 30 * len(triplets) and ties > visits // 2, (visits, ties)
    got = _both(ctx, U, tc, triplets, start, **kw)
    assert np.array_equal(got, replay) and not np.array_equal(got, start)


def test_nan_and_infinity_in_the_tables(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    N, triplets = _faces(1)
    L, kw = 5, dict(mcparam=0.3, iters=20, seed=4)
    rng = np.random.default_rng(12)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = np.zeros(N, dtype=np.int32)
    tc[0, 0, 0, 0] = np.nan       # costs[0] of the very first visit (every node still has label 0): nothing is smaller than a NaN there
    tc[3, 1, 0, 0] = np.nan       # a NaN in a later slot is never smaller
    tc[5, 0, 2, 0] = np.inf
    tc[7, :, :, 1] = -np.inf      # several equal infinities
    tc[9] = np.nan                # a triplet whose visits see nothing but NaN: it never changes a label
    a, b, c = triplets[12]
    U[2, a], U[0, b], U[1, c] = np.nan, np.inf, -np.inf
    got = _both(ctx, U, tc, triplets, start, **kw)
    assert got.any()
    # the first visit kept combination 000 whatever was proposed: replay it
    visits, _, replay = _count_ties(U, tc, triplets, start, kw["mcparam"], 1, kw["seed"])
    assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, mcparam=kw["mcparam"], iters=1, seed=kw["seed"]), replay)


def test_a_start_labelling_that_is_not_zero(ctx, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    U, tc, triplets, _, _, kw = _random_case(2, 19, 50)
    start = np.random.default_rng(2).integers(0, 19, U.shape[1]).astype(np.int32)
    got = _both(ctx, U, tc, triplets, start, mcparam=0.9, iters=3, seed=21)
    assert not np.array_equal(got, start)


def test_refusals_are_the_host_optimisers(ctx):
    U, tc, triplets, start, _, kw = _random_case(0, 19, 50)
    api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, **kw)
    before = api.mcmc_gpu_stats(ctx)
    bad = np.array(start)
    bad[7] = 19
    for fn in (lambda *a, **k: api.mcmc_optimise(*a, **k), lambda *a, **k: api.mcmc_optimise_gpu(ctx, *a, **k)):
        with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 7 out of range"):
            fn(U, tc, triplets, bad, **kw)
        bad_t = np.array(triplets)
        bad_t[11, 2] = U.shape[1]
        with pytest.raises(M.MsmError, match="msm_mcmc_optimise: triplet node out of range"):
            fn(U, tc, bad_t, start, **kw)
        with pytest.raises(M.MsmError, match=r"the geometric distribution parameter must be in \(0, 1\]"):
            fn(U, tc, triplets, start, mcparam=0.0, iters=3, seed=1)
    after = api.mcmc_gpu_stats(ctx)
    after.pop("draw_ms"), before.pop("draw_ms")
    assert after == before  # nothing ran in between


@pytest.mark.parametrize("kind,D", [("univariate", 1), ("multivariate", 3)])
def test_cost_function_tables_stay_on_the_device(ctx, monkeypatch, kind, D):
    """msm_cost_mcmc_optimise = computeUnaryCosts + computeTripletCosts + the host optimiser; twice in a row; once behind a queued label step"""
    monkeypatch.setenv(CHUNK, "3")
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=D)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **HCP)
    cf.get_source_data()
    kw = dict(mcparam=0.3, iters=20, seed=6)
    start = np.zeros(cf.N, dtype=np.int32)
    want = api.mcmc_optimise(cf.computeUnaryCosts(), cf.computeTripletCosts(), inp["triplets"], start, **kw)
    assert want.any()
    assert np.array_equal(cf.mcmc_optimise(start, **kw), want)
    assert np.array_equal(cf.mcmc_optimise(start, **kw), want)
    if kind == "univariate":  # a label step queued ahead on the context is resolved (here: dropped) before the tables are computed
        E = ctx.host_array((cf.T, 8))
        dropped = cf.prefetch_stats()[1]
        cf.prefetchTripletOctets(want, 3, E)
        assert np.array_equal(cf.mcmc_optimise(start, **kw), want)
        assert cf.prefetch_stats()[1] == dropped + 1
        ctx.release_host_array(E)
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 3 out of range"):
        bad = np.array(start)
        bad[3] = cf.L
        cf.mcmc_optimise(bad, **kw)
    cf.close()


def test_level_loop_with_the_opt_in(ctx):
    """run_discrete_level(optimiser="mcmc") with ProductOps(mcmc_gpu=True): the labellings, energies and coordinates of the run without it"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    kw = dict(cp_order=2, iters=2, mciters=20, mcparam=0.3, seed=5, kind="univariate", optimiser="mcmc", cost_params=dict(lambda_=0.05))
    t_gpu = {}
    got = registration.run_discrete_level(registration.ProductOps(ctx, mcmc_gpu=True), xyz, tri, ref, xyz, tri, src, xyz, timings=t_gpu, **kw)
    want = registration.run_discrete_level(registration.ProductOps(ctx), xyz, tri, ref, xyz, tri, src, xyz, **kw)
    assert "triplet_table" not in t_gpu and "unary_table" not in t_gpu and "optimiser" in t_gpu  # neither table was fetched
    assert len(got[3]) == 2 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and any(l.any() for l in got[3])
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_both_executables_with_the_opt_in(ctx, tmp_path):
    """MSMHIP_MCMC=gpu: tools/register_files.py and tools/cpp/newmsm write, for a --dopt=MCMC configuration, the bytes they write without it"""
    import __graft_entry__ as g
    from newmsm_amd import config, meshio

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(5)
    ref = synthetic.features(xyz, 2, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 2, 5)
    d = str(tmp_path) + "/"
    text = (config.PRESETS["standard_MSM_strain"].replace("--it=50,20,25,25", "--it=50,2,2,2").replace("--datagrid=5,5,5,6", "--datagrid=5,4,5,5")
            .replace("--SGgrid=0,4,5,6", "--SGgrid=0,4,5,5").replace("--CPgrid=0,2,3,4", "--CPgrid=0,2,3,3").replace("--dopt=HOCR", "--dopt=MCMC"))
    assert "--dopt=MCMC" in text
    with open(d + "conf", "w") as f:
        f.write(text + "--mciters=0,20,20,20\n")
    meshio.save_surface(d + "in.surf.gii", synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7) + 0.25, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    plain = {k: v for k, v in os.environ.items() if k != "MSMHIP_MCMC"}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    for tag, cmd in (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe])):
        for mode, env in (("host.", plain), ("gpu.", dict(plain, MSMHIP_MCMC="gpu"))):
            run = subprocess.run(cmd + common + ["--out=" + d + tag + mode, "-v"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
            assert ("MCMC sweeps on the GPU" in run.stdout) == (mode == "gpu."), run.stdout  # the opt-in was read, and only where it was set
        for n in names:
            with open(d + tag + "host." + n, "rb") as fa, open(d + tag + "gpu." + n, "rb") as fb:
                assert fa.read() == fb.read(), "%s of %s differs with MSMHIP_MCMC=gpu" % (n, tag)
    reg, _ = meshio.load_surface(d + "cppgpu.sphere.reg.surf.gii")
    assert angles(reg, meshio.load_surface(d + "in.surf.gii")[0]).max() > 1e-4  # something was registered
