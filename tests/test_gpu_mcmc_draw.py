"""The Monte Carlo optimiser's proposals drawn on the device (msm_ctx_set_mcmc_draw, msm_mcmc_draw_gpu; newmsm_amd/csrc/mcmc_draw.hpp, mcmc_draw_kernels.hip:
k_mcmc_draw; DESIGN.md 5.16 "Proposals on the device").  The device's streams are compared exactly with the library's own host stream (std::mt19937 +
std::geometric_distribution) chain by chain; with the context's mode set, every GPU entry point of the optimiser is compared exactly with what it gives
without it.  Shapes: streams that cross many 312-candidate blocks and end their chunks inside one, heavy rejection, thresholds in LDS and in global
memory, more chains than host threads."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic

import mcmc_chain_cases as cases

pytestmark = pytest.mark.gpu
HCP = dict(rmode=3, lambda_=0.01, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)
CHUNK, BLOCKS = "MSMHIP_MCMC_CHUNK_SWEEPS", "MSMHIP_MCMC_DRAW_BLOCKS"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWEEPS = 50
# (L, p): the default, six candidates in seven rejected, one label, every label 0, more thresholds than the 4096 that go to LDS
STREAMS = [(19, float(np.float32(0.8))), (3, 0.05), (1, 0.5), (4, 1.0), (5000, 0.01)]
SEED_SETS = [api.chain_seeds(3, 0, 1), api.chain_seeds(3, 0, 5), api.chain_seeds(3, 0, 17), [2 ** 32 + 5, 2 ** 40 + 1]]


@pytest.fixture
def draw_ctx(ctx, monkeypatch):
    """the session's context with the proposals drawn on the device; host draw again afterwards"""
    monkeypatch.delenv(BLOCKS, raising=False)
    ctx.set_mcmc_draw(1)
    yield ctx
    ctx.set_mcmc_draw(0)


@functools.lru_cache(maxsize=None)
def _host_stream(L, p, seed, T):
    out = api.mcmc_proposals(L, p, seed, T, SWEEPS)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _schedule_places(order):
    """(order, pos) of the icosphere's faces: the schedule's triplets by level, and where triplet t stands among them"""
    N, triplets = cases.faces(order)
    by_level = api.mcmc_schedule(triplets, N)[1]
    pos = np.empty(len(triplets), dtype=np.int32)
    pos[by_level] = np.arange(len(triplets), dtype=np.int32)
    return by_level, pos


@pytest.mark.parametrize("chunk", [1, 3, 50])
@pytest.mark.parametrize("L,p", STREAMS, ids=["L%d_p%g" % s for s in STREAMS])
@pytest.mark.parametrize("order", [0, 2])
def test_the_stream_alone(ctx, monkeypatch, order, L, p, chunk):
    """T = 20 and T = 320 (the faces of ico0 and ico2), 50 sweeps in chunks of 1, 3 (the last one shorter) and 50: every chain's stream is the host's, with
    the identity and with the schedule's places; the context's mode does not matter to this entry point"""
    monkeypatch.delenv(BLOCKS, raising=False)
    T = len(cases.faces(order)[1])
    by_level, pos = _schedule_places(order)
    for seeds in SEED_SETS:
        want = np.stack([_host_stream(L, p, int(s), T) for s in seeds])
        for places in (None, pos):
            got = api.mcmc_draw_gpu(ctx, L, p, seeds, T, SWEEPS, chunk_sweeps=chunk, pos=places)
            assert got.dtype == np.uint16 and got.shape == (len(seeds), SWEEPS, T)
            assert np.array_equal(got, want if places is None else want[:, :, by_level])
            stats = api.mcmc_draw_stats(ctx)
            assert stats["accepted"] == len(seeds) * SWEEPS * T and stats["candidates"] >= stats["accepted"]
            assert stats["block_bound"] == api.mcmc_draw_block_bound(min(chunk, SWEEPS - (SWEEPS - 1) // chunk * chunk) * T, L, p)
    if (L, p) == (3, 0.05):
        assert stats["candidates"] > 5 * stats["accepted"]  # heavy rejection
    if p == 1.0:
        assert stats["candidates"] == stats["accepted"] and not got.any()


def test_the_stream_alone_refusals(ctx):
    with pytest.raises(M.MsmError, match="not a permutation"):
        api.mcmc_draw_gpu(ctx, 19, 0.8, [1], 4, 2, pos=[0, 1, 1, 3])
    with pytest.raises(M.MsmError, match="not a permutation"):
        api.mcmc_draw_gpu(ctx, 19, 0.8, [1], 4, 2, pos=[0, 1, 2, 4])
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID"):
        api.mcmc_draw_gpu(ctx, 19, 0.8, list(range(257)), 4, 2)
    with pytest.raises(M.MsmError, match="geometric distribution parameter"):
        api.mcmc_draw_gpu(ctx, 19, 0.0, [1], 4, 2)
    with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY"):
        api.mcmc_draw_gpu(ctx, 19, 0.8, [1, 2], 2 ** 15, 2 ** 15)
    assert api.mcmc_draw_gpu(ctx, 19, 0.8, [1, 2], 0, 5).shape == (2, 5, 0) and api.mcmc_draw_gpu(ctx, 19, 0.8, [1, 2], 5, 0).shape == (2, 0, 5)


def test_context_mode_round_trip(ctx):
    assert ctx.get_mcmc_draw() == 0
    try:
        ctx.set_mcmc_draw(1)
        assert ctx.get_mcmc_draw() == 1
        with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*msm_ctx_set_mcmc_draw"):
            ctx.set_mcmc_draw(2)
        assert ctx.get_mcmc_draw() == 1
    finally:
        ctx.set_mcmc_draw(0)
    assert ctx.get_mcmc_draw() == 0


@pytest.mark.parametrize("chunk", ["1", "3", None])
@pytest.mark.parametrize("K", [2, 5, 17, 64])
@pytest.mark.parametrize("order", [0, 2])
def test_chains_with_the_draw_on_the_device(draw_ctx, monkeypatch, order, K, chunk):
    """the cases of test_gpu_mcmc_chains.py, and 64 chains (four times the host's draw threads): every chain is the host optimiser's on its seed"""
    if chunk is None:
        monkeypatch.delenv(CHUNK, raising=False)
    else:
        monkeypatch.setenv(CHUNK, chunk)
    U, tc, triplets, start = cases.tables(order)
    seeds, labs, E, best = cases.icosphere_chains(order, K)
    cases.check_chains(api.mcmc_optimise_chains_gpu(draw_ctx, U, tc, triplets, start, seeds, mcparam=cases.MCPARAM, iters=cases.SWEEPS), labs, E, best)
    assert api.mcmc_chains_info(draw_ctx) == (K, 0)  # no host thread drew
    stats, draw = api.mcmc_gpu_stats(draw_ctx), api.mcmc_draw_stats(draw_ctx)
    assert stats["chunks"] == {"1": 50, "3": 17, None: 1}[chunk] and stats["draw_ms"] == 0.0
    assert draw["accepted"] == K * cases.SWEEPS * len(triplets) and draw["candidates"] >= draw["accepted"] and draw["draw_ms"] > 0.0


@pytest.mark.parametrize("chunk", ["1", "3", None])
def test_single_chain_with_the_draw_on_the_device(draw_ctx, monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv(CHUNK, raising=False)
    else:
        monkeypatch.setenv(CHUNK, chunk)
    for order in (0, 2):
        U, tc, triplets, start = cases.tables(order)
        for seed in (7, 2 ** 32 + 7):
            want = api.mcmc_optimise(U, tc, triplets, start, mcparam=cases.MCPARAM, iters=cases.SWEEPS, seed=seed)
            got = api.mcmc_optimise_gpu(draw_ctx, U, tc, triplets, start, mcparam=cases.MCPARAM, iters=cases.SWEEPS, seed=seed)
            assert np.array_equal(got, want) and len(np.unique(want)) > 3
            assert api.mcmc_chains_info(draw_ctx) == (1, 0) and api.mcmc_gpu_stats(draw_ctx)["draw_ms"] == 0.0
            assert api.mcmc_draw_stats(draw_ctx)["accepted"] == cases.SWEEPS * len(triplets)


def test_no_sweeps_and_no_triplets_launch_no_draw(draw_ctx):
    U, tc, triplets, start = cases.tables(0)
    start = np.random.default_rng(3).integers(0, cases.LABELS, U.shape[1]).astype(np.int32)
    labs, E, best = cases.host_chains(U, tc, triplets, start, [1, 2, 3], 0.3, 0)
    cases.check_chains(api.mcmc_optimise_chains_gpu(draw_ctx, U, tc, triplets, start, [1, 2, 3], mcparam=0.3, iters=0), labs, E, best)
    none = np.zeros((0, 3), dtype=np.int32)
    labs, E, best = cases.host_chains(U, tc[:0], none, start, [1, 2], 0.3, 5)
    cases.check_chains(api.mcmc_optimise_chains_gpu(draw_ctx, U, tc[:0], none, start, [1, 2], mcparam=0.3, iters=5), labs, E, best)
    assert np.array_equal(api.mcmc_optimise_gpu(draw_ctx, U, tc, triplets, start, mcparam=0.3, iters=0, seed=4), start)


def test_repeats_and_the_mode_switched_off_again(ctx, monkeypatch):
    monkeypatch.setenv(CHUNK, "3")
    monkeypatch.delenv(BLOCKS, raising=False)
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 5)
    kw = dict(mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    try:
        ctx.set_mcmc_draw(1)
        first = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
        api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, [40, 41], **kw)  # another shape in between
        second = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
        assert api.mcmc_chains_info(ctx) == (5, 0)
    finally:
        ctx.set_mcmc_draw(0)
    off = api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
    chains, threads = api.mcmc_chains_info(ctx)
    assert chains == 5 and 1 <= threads <= 5 and api.mcmc_gpu_stats(ctx)["draw_ms"] > 0.0  # host threads drew again
    for got in (first, second, off):
        cases.check_chains(got, labs, E, best)
    assert first[2].tobytes() == second[2].tobytes() == off[2].tobytes()


def test_cost_function_tables_with_the_draw_on_the_device(ctx, monkeypatch):
    """msm_cost_mcmc_optimise and its chains form on the ico4-data / ico2-control problem of test_gpu_mcmc_chains.py: the host-draw results"""
    monkeypatch.setenv(CHUNK, "3")
    monkeypatch.delenv(BLOCKS, raising=False)
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", **HCP)
    cf.get_source_data()
    seeds, kw = api.chain_seeds(6, 0, 3), dict(mcparam=0.3, iters=20)
    start = np.zeros(cf.N, dtype=np.int32)
    want = cf.mcmc_optimise_chains(start, seeds, **kw)
    assert api.mcmc_chains_info(ctx)[1] >= 1 and want[1].any()
    want_one = cf.mcmc_optimise(start, seed=seeds[1], **kw)
    try:
        ctx.set_mcmc_draw(1)
        got = cf.mcmc_optimise_chains(start, seeds, **kw)
        assert api.mcmc_chains_info(ctx) == (3, 0)
        got_one = cf.mcmc_optimise(start, seed=seeds[1], **kw)
        assert api.mcmc_chains_info(ctx) == (1, 0)
    finally:
        ctx.set_mcmc_draw(0)
    cases.check_chains(got, want[1], want[2], want[3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got_one, want_one) and np.array_equal(want_one, want[1][1])
    cf.close()


def test_level_loop_with_the_draw_on_the_device(ctx, monkeypatch):
    """run_discrete_level(optimiser="mcmc") with three chains and with one, on the inputs of test_gpu_mcmc_chains.py: ProductOps(mcmc_gpu=True,
    mcmc_draw_gpu=True) gives the labellings, energies and coordinates of ProductOps(mcmc_gpu=True)"""
    monkeypatch.delenv(BLOCKS, raising=False)
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    kw = dict(cp_order=2, iters=2, mciters=20, mcparam=0.3, seed=5, kind="univariate", optimiser="mcmc", cost_params=dict(lambda_=0.05))
    with pytest.raises(ValueError, match="needs mcmc_gpu"):
        registration.ProductOps(ctx, mcmc_draw_gpu=True)
    assert ctx.get_mcmc_draw() == 0
    try:
        for chains in (3, 1):
            want = registration.run_discrete_level(registration.ProductOps(ctx, mcmc_gpu=True), xyz, tri, ref, xyz, tri, src, xyz, mcmc_chains=chains, **kw)
            assert api.mcmc_chains_info(ctx)[1] >= 1
            ops = registration.ProductOps(ctx, mcmc_gpu=True, mcmc_draw_gpu=True)
            assert ctx.get_mcmc_draw() == 1
            got = registration.run_discrete_level(ops, xyz, tri, ref, xyz, tri, src, xyz, mcmc_chains=chains, **kw)
            assert api.mcmc_chains_info(ctx) == (chains, 0)
            ctx.set_mcmc_draw(0)
            assert len(got[3]) == 2 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and any(l.any() for l in got[3])
            assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    finally:
        ctx.set_mcmc_draw(0)


def test_both_executables_with_the_draw_on_the_device(ctx, tmp_path):
    """MSMHIP_MCMC_DRAW=gpu beside MSMHIP_MCMC=gpu and three chains, on the inputs of test_gpu_mcmc_chains.py: tools/register_files.py and tools/cpp/newmsm
    write the bytes they write without it; without MSMHIP_MCMC=gpu either ends with a message and exit status 1"""
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
    plain = {k: v for k, v in os.environ.items() if k not in ("MSMHIP_MCMC", "MSMHIP_MCMC_CHAINS", "MSMHIP_MCMC_DRAW", BLOCKS)}
    three = dict(plain, MSMHIP_MCMC_CHAINS="3", MSMHIP_MCMC="gpu")
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    for tag, cmd in (("py", [sys.executable, "tools/register_files.py"]), ("cpp", [exe])):
        for mode, env in (("host.", dict(three, MSMHIP_MCMC_DRAW="host")), ("gpu.", dict(three, MSMHIP_MCMC_DRAW="gpu"))):
            run = subprocess.run(cmd + common + ["--out=" + d + tag + mode, "-v"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
            assert "MCMC sweeps on the GPU" in run.stdout and ("MCMC proposals drawn on the GPU." in run.stdout) == (mode == "gpu."), run.stdout
        bad = subprocess.run(cmd + common + ["--out=" + d + "bad."], cwd=ROOT, env=dict(plain, MSMHIP_MCMC_DRAW="gpu"), capture_output=True, text=True, timeout=600)
        assert bad.returncode == 1 and "MSMHIP_MCMC_DRAW=gpu" in bad.stderr and not os.path.exists(d + "bad." + names[0]), bad.stderr
    for n in names:
        with open(d + "pyhost." + n, "rb") as f:
            want = f.read()
        for other in ("pygpu.", "cpphost.", "cppgpu."):
            with open(d + other + n, "rb") as f:
                assert f.read() == want, "%s differs between pyhost. and %s" % (n, other)


def test_the_block_bound_ends_the_call_cleanly(ctx, monkeypatch):
    """MSMHIP_MCMC_DRAW_BLOCKS=1 (testing) and streams that need more than one block of 312 candidates: the kernel's ordinary bounded exit -- an error
    that names the draw, the caller's arrays as they were -- and the next call on the context, without the variable, gives the right bits"""
    monkeypatch.delenv(CHUNK, raising=False)
    U, tc, triplets, start = cases.tables(2)
    seeds, labs, E, best = cases.icosphere_chains(2, 5)
    kw = dict(mcparam=cases.MCPARAM, iters=cases.SWEEPS)
    L, N = U.shape
    c_ip, c_dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    try:
        ctx.set_mcmc_draw(1)
        monkeypatch.setenv(BLOCKS, "1")
        with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY.*msm_mcmc_draw_gpu: the proposal draw"):
            api.mcmc_draw_gpu(ctx, 19, 0.8, [1, 2], 320, 2)
        assert api.mcmc_draw_gpu(ctx, 19, 0.8, [1, 2], 20, 3).shape == (2, 3, 20)  # 60 proposals fit one block
        with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY.*msm_mcmc_optimise_chains_gpu: the proposal draw"):
            api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw)
        # the single-chain call through the C interface: its labelling argument stays as it was
        lab = np.full(N, 3, dtype=np.int32)
        Uc, tcc, trc = np.ascontiguousarray(U), np.ascontiguousarray(tc), np.ascontiguousarray(triplets, dtype=np.int32)
        st = M.lib().msm_mcmc_optimise_gpu(ctx.h, Uc.ctypes.data_as(c_dp), tcc.ctypes.data_as(c_dp), trc.ctypes.data_as(c_ip), N, L, len(trc), cases.MCPARAM,
                                           cases.SWEEPS, 7, lab.ctypes.data_as(c_ip))
        assert st == -7 and b"the proposal draw" in M.lib().msm_last_error() and (lab == 3).all()
        monkeypatch.delenv(BLOCKS)
        cases.check_chains(api.mcmc_optimise_chains_gpu(ctx, U, tc, triplets, start, seeds, **kw), labs, E, best)
        want = api.mcmc_optimise(U, tc, triplets, np.full(N, 3, dtype=np.int32), mcparam=cases.MCPARAM, iters=cases.SWEEPS, seed=7)
        assert np.array_equal(api.mcmc_optimise_gpu(ctx, U, tc, triplets, lab, mcparam=cases.MCPARAM, iters=cases.SWEEPS, seed=7), want)
    finally:
        ctx.set_mcmc_draw(0)
