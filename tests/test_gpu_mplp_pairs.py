"""MPLP over the pair tables on the GPU (msm_mplp_pairs_optimise_gpu / _polish_gpu, msm_cost_mplp_pairs_optimise; newmsm_amd/csrc/mplp_pairs.cpp and
mplp_pairs_kernels.hip): every case asks for the host literal's bits on the same arguments (test_mplp_pairs_cpu.py holds the host literal
to the numpy restatement).

The update kernel has one boundary: up to 64 labels a wavefront takes a pair (lane a holds column a), above 64 the four wavefronts of a workgroup share
one pair with their minima in LDS.  L = 63, 64, 65 sit on either side of it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, config, problem, registration, synthetic

import mplp_pairs_literal as PL
from helpers import angles

pytestmark = pytest.mark.gpu

WAVE_LABELS = 64  # kMplpPairWaveLabels


def _both(ctx, case, sweeps, bound=True, bounds=True, messages=True):
    """the GPU run, held to the host literal's bits"""
    kw = dict(sweeps=sweeps, bound=bound, bounds=bounds, messages=messages)
    got = api.mplp_pairs_optimise_gpu(ctx, *case, **kw)
    PL.same(got, api.mplp_pairs_optimise(*case, **kw))
    return got


def _polish_both(ctx, case, passes):
    got = api.mplp_pairs_polish_gpu(ctx, *case, polish=passes)
    PL.same_round(got, api.mplp_pairs_polish(*case, polish=passes))
    return got


@pytest.mark.parametrize("L", [1, 2, 3])
def test_one_pair(ctx, L):
    """fewer entries than a wavefront has lanes"""
    got = _both(ctx, PL.one_pair(L), 6)
    assert got.sweeps_run >= 1


@pytest.mark.parametrize("L", [16, 19, WAVE_LABELS - 1, WAVE_LABELS, WAVE_LABELS + 1])
def test_ico0_edges(ctx, L):
    """P = 30, 10 sweeps, on either side of the one-wavefront-per-pair boundary"""
    got = _both(ctx, PL.ico_case(0, L), 10)
    assert got.sweeps_run == 10 and got.labeling.any()


def test_ico0_edges_200_labels(ctx):
    """40 000 entries per pair on the workgroup route"""
    _both(ctx, PL.ico_case(0, 200), 3)


def test_one_pair_1024_labels_and_the_capacity(ctx):
    _both(ctx, PL.one_pair(1024), 2)
    big = (np.zeros((1025, 2)), np.zeros((1, 1025, 1025)), np.array([[0, 1]], dtype=np.int32), np.zeros(2, dtype=np.int32))
    for call in (lambda: api.mplp_pairs_optimise(*big, sweeps=2), lambda: api.mplp_pairs_optimise_gpu(ctx, *big, sweeps=2),
                 lambda: api.mplp_pairs_polish(*big, polish=2), lambda: api.mplp_pairs_polish_gpu(ctx, *big, polish=2)):
        with pytest.raises(M.MsmError, match="MSM_ERR_CAPACITY.*1025 labels"):
            call()


@pytest.mark.parametrize("shuffled", [False, True])
def test_ico2_edges(ctx, shuffled):
    """P = 480 in mesh order, and shuffled with half of the pairs reversed; the sweep's launches are the colouring's classes"""
    case = PL.ico_case(2, 19, 12, 0.0, False, shuffled)
    got = _both(ctx, case, 5)
    pcol, pk, _, _ = api.mplp_pairs_colouring(case[2], case[0].shape[1])
    stats = api.mplp_pairs_gpu_stats(ctx)
    assert stats["classes"] == pk and stats["sweeps_run"] == got.sweeps_run == 5 and stats["widest_class"] == np.bincount(pcol).max()
    assert stats["kernel_ms"] > 0.0


def test_ico4_edges(ctx):
    """P = 7680, the widest class past a thousand pairs"""
    _both(ctx, PL.ico_case(4, 5), 3)
    assert api.mplp_pairs_gpu_stats(ctx)["widest_class"] > 1000


def test_star_and_an_isolated_node(ctx):
    """40 classes of one pair, and an incidence list longer than any unrolled load"""
    case = PL.star_case()
    got = _both(ctx, case, 6)
    assert api.mplp_pairs_gpu_stats(ctx)["classes"] == 40 and got.labeling[41] == np.argmin(case[0][:, 41])


def test_doubled_pair(ctx):
    _both(ctx, PL.doubled_case(), 8)


def test_tables_with_entries_of_1e7(ctx):
    _both(ctx, PL.ico_case(0, 19, 13, 0.05), 10)
    _both(ctx, PL.ico_case(2, 7, 13, 0.05), 5)


def test_whole_number_tables_with_ties(ctx):
    _both(ctx, PL.ico_case(1, 4, 21, 0.0, True), 6)


def test_fixed_points_and_runs_longer_than_a_chunk(ctx):
    """a chain of three nodes reaches its fixed point early (the launches behind it return at once); 300 sweeps are more than one chunk of 256"""
    got = _both(ctx, PL.chain_case(3, 3, 1), 300)
    assert 1 <= got.sweeps_run < 256
    assert np.all(got.energies[got.sweeps_run:] == got.energies[got.sweeps_run - 1]) and np.all(got.bounds[got.sweeps_run:] == got.bound)
    _both(ctx, PL.random_case(PL.K4, 4, 3, 2), 300)  # a run that (with cycles) goes on past one chunk


def test_optional_outputs_and_zero_work(ctx):
    case = PL.ico_case(0, 19)
    U, pc, pairs, start = case
    full = _both(ctx, case, 4)
    for bound in (False, True):
        for bounds in (False, True):
            for messages in (False, True):
                got = _both(ctx, case, 4, bound=bound, bounds=bounds, messages=messages)
                assert (got.bound is None) == (not bound and not bounds) and (got.bounds is None) == (not bounds) and (got.messages is None) == (not messages)
                PL.same(got, full)
    none = _both(ctx, case, 0)
    assert np.array_equal(none.labeling, start) and none.sweeps_run == 0
    empty = _both(ctx, (U, np.zeros((0, 19, 19)), np.zeros((0, 2), dtype=np.int32), start), 3)
    assert np.array_equal(empty.labeling, start) and empty.sweeps_run == 0


def test_refusals_are_the_host_literals(ctx):
    """every refusal of the host literal, with its message, and nothing written: every output is pre-filled and handed over through ctypes"""
    ok = PL.ico_case(0, 5, 31)
    _both(ctx, ok, 2)
    _polish_both(ctx, ok, 2)
    before = api.mplp_pairs_gpu_stats(ctx)
    for args, pattern in PL.refusals():
        st, st2, untouched = PL.raw(*args, 3, ctx=ctx)
        assert st != 0 and st2 != 0 and untouched, pattern
        assert (st, st2) == PL.raw(*args, 3)[:2], pattern  # the host literal's statuses
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_pairs_optimise_gpu(ctx, *args, sweeps=3)
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_pairs_polish_gpu(ctx, *args, polish=3)
    for counts in (dict(N=0), dict(N=-3), dict(L=0), dict(L=-1), dict(P=-1)):  # negative counts, and no nodes or labels at all
        st, st2, untouched = PL.raw(*ok, 3, ctx=ctx, **counts)
        assert st != 0 and st2 != 0 and untouched, counts
    st, st2, untouched = PL.raw(*ok, -1, ctx=ctx)  # a negative count of sweeps, of passes
    assert st != 0 and st2 != 0 and untouched
    with pytest.raises(M.MsmError, match="MSM_ERR_INVALID.*polish passes"):
        api.mplp_pairs_polish_gpu(ctx, *ok, polish=1025)
    assert api.mplp_pairs_gpu_stats(ctx) == before  # no sweep and no pass ran in between
    st, st2, untouched = PL.raw(*ok, 3, ctx=ctx)
    assert st == 0 and st2 == 0 and not untouched
    _both(ctx, ok, 2)  # and the context is as good as before


def test_every_combination_of_absent_outputs(ctx):
    """NULL for each of sweeps_run, energy, bound, energies, bounds, messages (64 combinations), and for each of the polish's passes_run, energy,
    energies (8), through ctypes on both routes: what is asked for is what the full call gives, bit for bit"""
    import ctypes as C
    import itertools

    from newmsm_amd._lib import c_dp, c_ip, lib

    U, pc, pairs, start = (np.ascontiguousarray(a) for a in PL.ico_case(0, 19))
    L, N = U.shape
    P, sweeps, passes = len(pairs), 4, 3
    head = (U.ctypes.data_as(c_dp), pc.ctypes.data_as(c_dp), pairs.ctypes.data_as(c_ip), N, L, P)
    full = api.mplp_pairs_optimise(U, pc, pairs, start, sweeps=sweeps, bounds=True, messages=True)
    pfull = api.mplp_pairs_polish(U, pc, pairs, start, polish=passes)
    null_i, null_d = C.cast(None, c_ip), C.cast(None, c_dp)
    routes = [(lib().msm_mplp_pairs_optimise, lib().msm_mplp_pairs_polish, ()), (lib().msm_mplp_pairs_optimise_gpu, lib().msm_mplp_pairs_polish_gpu, (ctx.h,))]
    for optimise, polish, first in routes:
        for want in itertools.product((False, True), repeat=6):
            lab, run, energy, bound = np.array(start), np.full(1, -7, dtype=np.int32), np.full(1, -7.0), np.full(1, -7.0)
            energies, bounds, messages = np.full(sweeps, -7.0), np.full(sweeps, -7.0), np.full((P, 2, L), -7.0)
            arrays = (run, energy, bound, energies, bounds, messages)
            ptrs = [a.ctypes.data_as(c_ip if a.dtype == np.int32 else c_dp) if w else (null_i if a.dtype == np.int32 else null_d) for a, w in zip(arrays, want)]
            assert optimise(*first, *head, sweeps, lab.ctypes.data_as(c_ip), *ptrs) == 0, want
            assert np.array_equal(lab, full.labeling), want
            wanted = (np.int32(full.sweeps_run), full.energy, full.bound, full.energies, full.bounds, full.messages)
            for a, w, value in zip(arrays, want, wanted):
                expect = np.asarray(value, dtype=a.dtype).reshape(a.shape) if w else np.full_like(a, -7)
                assert a.tobytes() == expect.tobytes(), want
        for want in itertools.product((False, True), repeat=3):
            lab, run, energy, energies = np.array(start), np.full(1, -7, dtype=np.int32), np.full(1, -7.0), np.full(1 + passes, -7.0)
            arrays = (run, energy, energies)
            ptrs = [a.ctypes.data_as(c_ip if a.dtype == np.int32 else c_dp) if w else (null_i if a.dtype == np.int32 else null_d) for a, w in zip(arrays, want)]
            assert polish(*first, *head, passes, lab.ctypes.data_as(c_ip), *ptrs) == 0, want
            assert np.array_equal(lab, pfull.labeling), want
            for a, w, value in zip(arrays, want, (np.int32(pfull.passes_run), pfull.energy, pfull.energies)):
                expect = np.asarray(value, dtype=a.dtype).reshape(a.shape) if w else np.full_like(a, -7)
                assert a.tobytes() == expect.tobytes(), want


POLISH = [("ico0", (PL.ico_case, (0, 19))), ("ico2 shuffled", (PL.ico_case, (2, 7, 12, 0.0, False, True))), ("star", (PL.star_case, ())),
          ("ties", (PL.ico_case, (1, 4, 21, 0.0, True)))]


@pytest.mark.parametrize("name,spec", POLISH, ids=[n for n, _ in POLISH])
@pytest.mark.parametrize("passes", [0, 1, 8])
def test_polish(ctx, name, spec, passes):
    case = PL.make(spec)
    got = _polish_both(ctx, case, passes)
    assert got.energy <= got.energies[0] and len(got.energies) == 1 + passes
    stats = api.mplp_pairs_gpu_stats(ctx)
    assert stats["passes_run"] == got.passes_run <= passes


def test_polish_to_its_fixed_point_and_past_one_wavefront_of_labels(ctx):
    got = _polish_both(ctx, PL.ico_case(2, 7), 40)
    assert 1 <= got.passes_run < 40
    _polish_both(ctx, PL.ico_case(0, WAVE_LABELS + 1), 3)
    _polish_both(ctx, PL.ico_case(0, 200), 2)


LAMBDA = dict(lambda_=0.1, rexp=2.0)


@pytest.mark.parametrize("kind,D", [("univariate", 1), ("multivariate", 3)])
@pytest.mark.parametrize("polish", [0, 8])
def test_cost_function_tables_stay_on_the_device(ctx, kind, D, polish):
    """msm_cost_mplp_pairs_optimise = computeUnaryCosts + computePairwiseCosts + the host literals, at data ico4 / control grid ico2; twice in a row"""
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=D)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, rmode=1, **LAMBDA)
    cf.get_source_data()
    start = np.zeros(cf.N, dtype=np.int32)
    U, pc = cf.computeUnaryCosts(), cf.computePairwiseCosts()
    want = api.mplp_pairs_optimise(U, pc, inp["pairs"], start, sweeps=5, bounds=True)
    assert want.labeling.any() and want.bound <= want.energy
    wp = api.mplp_pairs_polish(U, pc, inp["pairs"], want.labeling, polish=polish) if polish else None
    for _ in range(2):
        got, gp = cf.mplp_pairs_optimise(start, sweeps=5, polish=polish, bounds=True)
        assert got.sweeps_run == want.sweeps_run and got.bound == want.bound
        assert got.energies.tobytes() == want.energies.tobytes() and got.bounds.tobytes() == want.bounds.tobytes()
        if polish:
            PL.same_round(gp, wp)
            assert got.energy == wp.energy
        else:
            assert gp is None and np.array_equal(got.labeling, want.labeling) and got.energy == want.energy
    with pytest.raises(M.MsmError, match="label of node 3 out of range"):
        bad = np.array(start)
        bad[3] = cf.L
        cf.mplp_pairs_optimise(bad, sweeps=5)
    cf.close()


def test_cost_function_without_pairs_is_refused(ctx):
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind="univariate", rmode=3)  # sets triplets, no pairs
    cf.get_source_data()
    with pytest.raises(M.MsmError, match="MSM_ERR_STATE.*pairs must be set first"):
        cf.mplp_pairs_optimise(np.zeros(cf.N, dtype=np.int32), sweeps=2)
    cf.close()


def _level_inputs():
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    return xyz, tri, ref, src


@pytest.mark.parametrize("polish", [False, True])
def test_level_loop(ctx, polish):
    """run_discrete_level(optimiser="mplp_pairs"): with the tables on the device, the labellings, energies and coordinates of the fetched-table route; no
    iteration's energy lies above the zero labelling's"""
    xyz, tri, ref, src = _level_inputs()
    kw = dict(cp_order=2, iters=3, mciters=5, kind="univariate", optimiser="mplp_pairs", rmode=1, cost_params=dict(lambda_=0.1), converge=False)
    t_gpu, t_host = {}, {}
    ops = dict(mplp_round=polish, mplp_polish=4, mplp_pairs=True)
    got = registration.run_discrete_level(registration.ProductOps(ctx, **ops), xyz, tri, ref, xyz, tri, src, xyz, timings=t_gpu, **kw)
    seen = []  # per iteration of the host route: the table energy of the zero labelling it starts from, and of the labelling it returns

    class Recording(registration.ProductOps):
        def mplp_pairs_solve(self, unary, paircosts, pairs, labeling, sweeps):
            lab = super().mplp_pairs_solve(unary, paircosts, pairs, labeling, sweeps)
            assert not np.any(labeling)
            seen.append((api.mplp_pairs_energy(unary, paircosts, pairs, labeling), api.mplp_pairs_energy(unary, paircosts, pairs, lab)))
            return lab

    want = registration.run_discrete_level(Recording(ctx, mplp_gpu=False, **ops), xyz, tri, ref, xyz, tri, src, xyz, timings=t_host, **kw)
    assert len(seen) == 3 and all(e <= e0 for e0, e in seen) and seen[0][1] < seen[0][0]
    assert "pairwise_table" not in t_gpu and "unary_table" not in t_gpu and "optimiser" in t_gpu  # neither table was fetched
    assert "pairwise_table" in t_host and "unary_table" in t_host
    assert len(got[3]) == 3 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and got[3][0].any()
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_level_loop_needs_the_pairwise_regulariser_and_the_opt_in(ctx):
    xyz, tri, ref, src = _level_inputs()
    with pytest.raises(ValueError, match="needs ops.mplp_pairs"):  # ProductOps(mplp_pairs=True) is the level loop's opt-in
        registration.run_discrete_level(registration.ProductOps(ctx), xyz, tri, ref, xyz, tri, src, xyz, cp_order=2, iters=1, mciters=2, kind="univariate",
                                        optimiser="mplp_pairs", rmode=1, cost_params=dict(lambda_=0.1))
    with pytest.raises(ValueError, match="you cannot run higher order clique regularisers with fastPD"):
        registration.run_discrete_level(registration.ProductOps(ctx), xyz, tri, ref, xyz, tri, src, xyz, cp_order=2, iters=1, mciters=2, kind="univariate",
                                        optimiser="mplp_pairs", rmode=3, cost_params=dict(lambda_=0.1))


CONF = ("--simval=2,2\n--sigma_in=2,2\n--sigma_ref=2,2\n--lambda=0.1,0.1\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=1,2\n--SGgrid=3,4\n--datagrid=3,4\n"
        "--regoption=1\n--regexp=2\n--dopt=MPLP\n--VN\n--rescaleL\n--mciters=5,5\n")


def test_both_executables(ctx, tmp_path):
    """MSMHIP_MPLP=on MSMHIP_MPLP_PAIRS=on: tools/register_files.py and tools/cpp/newmsm write the same bytes for a two-level --regoption=1 / --dopt=MPLP
    configuration, with and without the polish; without MSMHIP_MPLP_PAIRS both end with the FastPD-only message and status 1, and the variable is refused
    without MSMHIP_MPLP=on or with another value"""
    import __graft_entry__ as g
    from newmsm_amd import meshio

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 2, 5)
    src = synthetic.features(synthetic.known_warp(xyz, seed=8, rot_deg=3.0, amp=2.0), 2, 5)
    d = str(tmp_path) + "/"
    with open(d + "conf", "w") as f:
        f.write(CONF)
    meshio.save_surface(d + "in.surf.gii", synthetic.known_warp(xyz, seed=3, rot_deg=0.0, amp=0.7) + 0.25, tri)
    meshio.save_surface(d + "ref.surf.gii", xyz, tri)
    meshio.save_metric(d + "in.func.gii", src)
    meshio.save_metric(d + "ref.func.gii", ref)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--inmesh=" + d + "in.surf.gii", "--refmesh=" + d + "ref.surf.gii", "--indata=" + d + "in.func.gii", "--refdata=" + d + "ref.func.gii", "--conf=" + d + "conf"]
    plain = {k: v for k, v in os.environ.items() if not k.startswith("MSMHIP_MPLP")}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    refused = [(dict(MSMHIP_MPLP="on"), "--regoption=1"), (dict(), "Unrecognized optimiser"), (dict(MSMHIP_MPLP_PAIRS="on"), "it needs MSMHIP_MPLP=on"),
               (dict(MSMHIP_MPLP="on", MSMHIP_MPLP_PAIRS="yes"), "MSMHIP_MPLP_PAIRS=yes")]
    runs = [("plain.", dict(MSMHIP_MPLP="on", MSMHIP_MPLP_PAIRS="on")),
            ("polish.", dict(MSMHIP_MPLP="on", MSMHIP_MPLP_PAIRS="on", MSMHIP_MPLP_ROUND="on", MSMHIP_MPLP_POLISH="4"))]
    for tag, cmd in (("py.", [sys.executable, "tools/register_files.py"]), ("cpp.", [exe])):
        for env, message in refused:
            off = subprocess.run(cmd + common + ["--out=" + d + "off." + tag], cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=600)
            assert off.returncode == 1 and message in off.stdout + off.stderr, (env, off.returncode, off.stdout, off.stderr)
            assert not any(os.path.exists(d + "off." + tag + n) for n in names)
        for run_tag, env in runs:
            run = subprocess.run(cmd + common + ["--out=" + d + run_tag + tag], cwd=root, env=dict(plain, **env), capture_output=True, text=True, timeout=600)
            assert run.returncode == 0, run.stderr
    for run_tag, _ in runs:
        for n in names:
            with open(d + run_tag + "py." + n, "rb") as fa, open(d + run_tag + "cpp." + n, "rb") as fb:
                assert fa.read() == fb.read(), "%s differs between the two executables" % (run_tag + n)
    reg, _ = meshio.load_surface(d + "plain.cpp.sphere.reg.surf.gii")
    assert angles(reg, meshio.load_surface(d + "in.surf.gii")[0]).max() > 1e-4  # something was registered
