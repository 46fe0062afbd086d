"""Several Monte Carlo optimiser chains in one launch (msm_mcmc_optimise_chains_gpu, msm_cost_mcmc_optimise_chains; newmsm_amd/csrc/mcmc.cpp,
mcmc_kernels.hip: k_mcmc_chains, k_mcmc_chain_terms; DESIGN.md 5.16 "Chains"): workgroup k walks chain k over the shared schedule and tables.  Every chain is
compared exactly with the host optimiser (api.mcmc_optimise) on its seed, every energy with a plain serial sum, best with std::min_element's rule."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic

import mcmc_chain_cases as cases
from helpers import angles

pytestmark = pytest.mark.gpu
HCP = dict(rmode=3, lambda_=0.01, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)
CHUNK = "MSMHIP_MCMC_CHUNK_SWEEPS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _both(ctx, U, tc, triplets, start, seeds, mcparam, iters):
    """the GPU chains against K host runs, serial energies and the rule; returns (labelings, energies, best)"""
    labs, E, best = cases.host_chains(U, tc, triplets, start, seeds, mcparam, iters)
    cases.check_chains(api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, mcparam=mcparam, iters=iters), labs, E, best)
    assert api.mcmc_chains_info(ctx)[0] == len(seeds)
    return labs, E, best


def test_one_chain_is_the_single_chain_call(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 1)
    single = api.mcmc_optimise_gpu(ctx, U, tc, triplets, start, mcparam=cases.MCPARAM, iters=cases.SWEEPS, seed=seeds[0])
    assert api.mcmc_chains_info(ctx) == (1, 1)
    one = api.mcmc_gpu_stats(ctx)
    got = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    cases.check_chains(got, labs, E, best)
    assert best == 0 and np.array_equal(got[0], single) and np.array_equal(got[1][0], single) and len(np.unique(single)) > 3
    assert api.mcmc_chains_info(ctx) == (1, 1)
    stats = api.mcmc_gpu_stats(ctx)
    assert all(stats[k] == one[k] for k in ("levels", "chunks", "levels_per_sweep", "widest_level")) and stats["chunks"] == 17


@pytest.mark.parametrize("chunk", ["1", "3", None])
@pytest.mark.parametrize("K", [2, 5, 17])
@pytest.mark.parametrize("order", [0, 2])
def test_random_tables_on_icosphere_faces(ctx, monkeypatch, order, K, chunk):
    """T = 20 and T = 320, 19 labels, 50 sweeps; chunks of one sweep, of three (the last one shorter) and the default (the whole run in one); 17 chains are
    more than the host threads.  The seeds make a chain other than 0 win, with all energies distinct (asserted on the host in test_mcmc_chains_cpu.py)."""
    if chunk is None:
        monkeypatch.delenv(CHUNK, raising=False)
    else:
        monkeypatch.setenv(CHUNK, chunk)
    U, tc, triplets, start = cases.tables(order)
    seeds, labs, E, best = cases.icosphere_chains(order, K)
    assert best != 0 and len(set(E.tolist())) == K
    cases.check_chains(api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS), labs, E, best)
    stats = api.mcmc_gpu_stats(ctx)
    assert stats["chunks"] == {"1": 50, "3": 17, None: 1}[chunk]
    assert stats["levels_per_sweep"] == {0: 10, 2: 28}[order] and stats["levels"] == 50 * stats["levels_per_sweep"]  # the levels one chain walked
    chains, threads = api.mcmc_chains_info(ctx)
    assert chains == K and 1 <= threads <= min(K, 16)


def test_host_threads_do_not_change_the_result(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 17)
    for threads in (1, 4, 16):
        monkeypatch.setenv("MSMHIP_HOST_THREADS", str(threads))
        cases.check_chains(api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS), labs, E, best)
        assert api.mcmc_chains_info(ctx) == (17, threads)


def test_ico4_faces(ctx, monkeypatch):
    """T = 5120: the widest level holds 320 triplets"""
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start = cases.tables(4, 5)
    labs, _, _ = _both(ctx, U, tc, triplets, start, [7, 8, 9], 0.3, 4)
    assert labs.any() and not np.array_equal(labs[0], labs[1])
    stats = api.mcmc_gpu_stats(ctx)
    assert stats["levels_per_sweep"] == 32 and stats["widest_level"] == 320 and stats["chunks"] == 2


def test_a_level_wider_than_the_workgroup(ctx, monkeypatch):
    """1500 mutually disjoint triplets are one level of 1500: walked in strides; 1500 more reuse their nodes in reverse order (a second level)"""
    monkeypatch.setenv(CHUNK, "3")
    first = np.arange(4500, dtype=np.int32).reshape(1500, 3)
    triplets = np.concatenate([first, np.arange(4500, dtype=np.int32)[::-1].reshape(1500, 3)])
    rng = np.random.default_rng(5)
    L = 4
    labs, _, _ = _both(ctx, rng.normal(size=(L, 4500)), rng.normal(size=(3000, L, L, L)), triplets, np.zeros(4500, dtype=np.int32), [3, 4], 0.4, 7)
    assert len(np.unique(labs[1])) == L and api.mcmc_gpu_stats(ctx)["widest_level"] == 1500


def test_labellings_beyond_64_kb_of_lds(ctx, monkeypatch):
    """70 000 nodes are 140 000 bytes of labels per chain: the new kernel's launch asks for more than the 64 KB a kernel gets by default"""
    monkeypatch.setenv(CHUNK, "3")
    rng = np.random.default_rng(15)
    N, T, L = 70000, 3000, 3
    triplets = rng.integers(0, N, (T, 3)).astype(np.int32)
    triplets[:, 0] = np.arange(N - T, N)  # the highest nodes are named
    start = rng.integers(0, L, N).astype(np.int32)
    labs, _, _ = _both(ctx, rng.normal(size=(L, N)), rng.normal(size=(T, L, L, L)), triplets, start, [2, 11], 0.4, 5)
    assert not np.array_equal(labs[0], start) and not np.array_equal(labs[0], labs[1])


def test_lists_that_are_no_mesh(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "1")
    rng = np.random.default_rng(6)
    L, N = 6, 9
    # a triplet that names a node twice (and one three times), two identical triplets in a row
    triplets = np.array([[0, 0, 1], [2, 3, 4], [2, 3, 4], [5, 5, 5], [4, 0, 5], [8, 7, 8], [6, 1, 6]], dtype=np.int32)
    U, tc = rng.normal(size=(L, N)), rng.normal(size=(len(triplets), L, L, L))
    start = rng.integers(0, L, N).astype(np.int32)
    labs, _, _ = _both(ctx, U, tc, triplets, start, [1, 2], 0.3, 25)
    assert not np.array_equal(labs[0], start)


def test_equal_seeds_no_sweeps_and_no_triplets(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    U, tc, triplets, start = cases.tables(0)
    labs, E, best = _both(ctx, U, tc, triplets, start, [9, 9, 4], cases.MCPARAM, cases.SWEEPS)
    assert np.array_equal(labs[0], labs[1]) and E[0] == E[1] and best != 1  # of two equal chains the lower index
    labs, E, best = _both(ctx, U, tc, triplets, start, [6, 6], cases.MCPARAM, cases.SWEEPS)
    assert best == 0 and E[0] == E[1]
    # no sweeps: every chain is the start, the energies are the start's, best is 0
    start = np.random.default_rng(3).integers(0, cases.LABELS, U.shape[1]).astype(np.int32)
    labs, E, best = _both(ctx, U, tc, triplets, start, [1, 2, 3], 0.3, 0)
    assert best == 0 and np.array_equal(labs, np.tile(start, (3, 1))) and E[0] == E[1] == E[2] == api.mcmc_energy(U, tc, triplets, start)
    # no triplets
    labs, E, best = _both(ctx, U, tc[:0], np.zeros((0, 3), dtype=np.int32), start, [1, 2], 0.3, 5)
    assert best == 0 and np.array_equal(labs, np.tile(start, (2, 1))) and E[0] == E[1]


def test_refusals_launch_nothing(ctx):
    U, tc, triplets, start = cases.tables(0)
    kw = dict(mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, [1, 2, 3], **kw)
    before, info = api.mcmc_gpu_stats(ctx), api.mcmc_chains_info(ctx)
    assert info[0] == 3
    for seeds in ([], list(range(257)), None):  # K = 0, K = 257, NULL seeds
        with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*msm_mcmc_optimise_chains"):
            api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
        assert api.mcmc_gpu_stats(ctx) == before and api.mcmc_chains_info(ctx) == info
    with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY.*80001 nodes do not fit the LDS"):
        api.mcmc_optimise_chains_gpu(ctx, np.zeros((1, 80001)), np.zeros((1, 1, 1, 1)), [[0, 1, 80000]], np.zeros(80001, dtype=np.int32), [1, 2], iters=1)
    assert api.mcmc_gpu_stats(ctx) == before and api.mcmc_chains_info(ctx) == info
    bad = np.array(start)
    bad[7] = cases.LABELS
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 7 out of range"):
        api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, bad, [1, 2], **kw)
    bad_t = np.array(triplets)
    bad_t[11, 2] = U.shape[1]
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: triplet node out of range"):
        api.mcmc_optimise_chains_gpu(ctx, U, tc, bad_t, start, [1, 2], **kw)
    with pytest.raises(M.MsmError, match=r"the geometric distribution parameter must be in \(0, 1\]"):
        api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, [1, 2], mcparam=0.0, iters=3)
    assert api.mcmc_gpu_stats(ctx) == before and api.mcmc_chains_info(ctx) == info


def test_a_second_call_repeats_the_bits(ctx, monkeypatch):
    monkeypatch.delenv(CHUNK, raising=False)
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 5)
    kw = dict(mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    first = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
    api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, [40, 41], **kw)  # another shape in between
    second = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
    cases.check_chains(first, labs, E, best)
    cases.check_chains(second, labs, E, best)
    assert first[2].tobytes() == second[2].tobytes()


def test_cost_function_tables_stay_on_the_device(ctx, monkeypatch, capsys):
    """msm_cost_mcmc_optimise_chains = computeUnaryCosts + computeTripletCosts + the host chains, on an ico4-data / ico2-control problem with 19 labels.  The
    difference between the best chain's table energy and msm_cost_total of its labelling is printed, not asserted: the table entries and
    the on-demand costs are not known to be bit-equal."""
    monkeypatch.setenv(CHUNK, "3")
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", **HCP)
    cf.get_source_data()
    assert cf.L == 19
    seeds, kw = api.chain_seeds(6, 0, 3), dict(mcparam=0.3, iters=20)
    start = np.zeros(cf.N, dtype=np.int32)
    U, tc = np.array(cf.computeUnaryCosts()), np.array(cf.computeTripletCosts()).reshape(cf.T, cf.L, cf.L, cf.L)
    labs, E, best = cases.host_chains(U, tc, inp["triplets"], start, seeds, **kw)
    cases.check_chains(api.mcmc_optimise_chains(U, tc, inp["triplets"], start, seeds, **kw), labs, E, best)
    assert labs.any() and not np.array_equal(labs[0], labs[1])
    got = cf.mcmc_optimise_chains(start, seeds, **kw)
    cases.check_chains(got, labs, E, best)
    assert got[2][got[3]] <= got[2][0] and api.mcmc_chains_info(ctx)[0] == 3
    cases.check_chains(cf.mcmc_optimise_chains(start, seeds, **kw), labs, E, best)  # twice in a row
    assert np.array_equal(cf.mcmc_optimise(start, seed=seeds[0], **kw), labs[0]) and api.mcmc_chains_info(ctx) == (1, 1)
    total = cf.evaluateTotalCostSum(got[0])[0]
    with capsys.disabled():
        print("\nbest chain %d: table energy %.17g, msm_cost_total %.17g, difference %.3e" % (best, E[best], total, E[best] - total))
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*msm_mcmc_optimise_chains"):
        cf.mcmc_optimise_chains(start, [], **kw)
    cf.close()


def test_level_loop_with_three_chains(ctx):
    """run_discrete_level(optimiser="mcmc", mcmc_chains=3): ProductOps(mcmc_gpu=True) and the host branch give the same labellings, energies and coordinates;
    mcmc_chains=1 is the call without the argument"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    kw = dict(cp_order=2, iters=2, mciters=20, mcparam=0.3, seed=5, kind="univariate", optimiser="mcmc", cost_params=dict(lambda_=0.05))

    def run(gpu, **more):
        return registration.run_discrete_level(registration.ProductOps(ctx, mcmc_gpu=gpu), xyz, tri, ref, xyz, tri, src, xyz, **kw, **more)

    got = run(True, mcmc_chains=3)
    assert api.mcmc_chains_info(ctx)[0] == 3
    want = run(False, mcmc_chains=3)
    assert len(got[3]) == 2 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and any(l.any() for l in got[3])
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    one, plain = run(True, mcmc_chains=1), run(True)
    assert api.mcmc_chains_info(ctx) == (1, 1)
    assert all(np.array_equal(a, b) for a, b in zip(one[3], plain[3])) and one[2] == plain[2] and np.array_equal(one[0], plain[0])


def test_both_executables_with_three_chains(ctx, tmp_path):
    """MSMHIP_MCMC_CHAINS=3: tools/register_files.py and tools/cpp/newmsm write the same bytes as each other, with and without MSMHIP_MCMC=gpu;
    MSMHIP_MCMC_CHAINS=0 ends either with a message and exit status 1"""
    import __graft_entry__ as g
    from newmsm_amd import config, meshio

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(5)
    ref = synthetic.features(xyz, 2, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 2, 5)
    d = str(tmp_path) + "/"
    text = (config.PRESETS["standard_MSM_strain"].replace("--it=50,20,25,25", "--it=50,2,2,2").replace("--datagrid=5,5,5,6", "--datagrid=5,4,5,5")
            .replace("--SGgrid=0,4,5,6", "--SGgrid=0,4,5,5").replace("--CPgrid=0,2,3,4", "--CPgrid=0,2,3,3").replace("--dopt=HOCR", "--dopt=MCMC"))
    assert "--dopt=MCMC" in text and "--CPgrid=0,2,3,3" in text
    with open(d + "conf", "w") as f:
        f.write(text + "--mciters=0,20,20,20\n")
    meshio.save_surface(d + "in.surf.gii", synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7) + 0.25, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    plain = {k: v for k, v in os.environ.items() if k not in ("MSMHIP_MCMC", "MSMHIP_MCMC_CHAINS")}
    three = dict(plain, MSMHIP_MCMC_CHAINS="3")
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    tools = (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe]))
    for tag, cmd in tools:
        for mode, env in (("host.", three), ("gpu.", dict(three, MSMHIP_MCMC="gpu"))):
            run = subprocess.run(cmd + common + ["--out=" + d + tag + mode, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
            assert "MCMC with 3 chains per iteration." in run.stdout and ("MCMC sweeps on the GPU" in run.stdout) == (mode == "gpu."), run.stdout
        bad = subprocess.run(cmd + common + ["--out=" + d + "bad."], cwd=ROOT, env=dict(plain, MSMHIP_MCMC_CHAINS="0"), capture_output=True, text=True, timeout=600)
        assert bad.returncode == 1 and "MSMHIP_MCMC_CHAINS=0" in bad.stderr and not os.path.exists(d + "bad." + names[0]), bad.stderr
    for n in names:
        with open(d + "pyhost." + n, "rb") as f:
            want = f.read()
        for other in ("pygpu.", "cpphost.", "cppgpu."):
            with open(d + other + n, "rb") as f:
                assert f.read() == want, "%s differs between pyhost. and %s" % (n, other)
    # one chain is the run without the variable
    for env, out in ((dict(plain, MSMHIP_MCMC="gpu"), "unset."), (dict(plain, MSMHIP_MCMC="gpu", MSMHIP_MCMC_CHAINS="1"), "one.")):
        run = subprocess.run([exe] + common + ["--out=" + d + out, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert run.returncode == 0 and "chains per iteration" not in run.stdout, run.stderr
    for n in names:
        with open(d + "unset." + n, "rb") as fa, open(d + "one." + n, "rb") as fb:
            assert fa.read() == fb.read(), n
    reg, _ = meshio.load_surface(d + "cppgpu.sphere.reg.surf.gii")
    assert angles(reg, meshio.load_surface(d + "in.surf.gii")[0]).max() > 1e-4  # something was registered
