"""The MPLP optimiser's sweeps on the GPU (msm_mplp_optimise_gpu, msm_cost_mplp_optimise; newmsm_amd/csrc/mplp.cpp, mplp_kernels.hip):
a launch per level, a workgroup per factor.  Every case asks for the host literal's bits (msm_mplp_optimise) on the same arguments: labelling, sweeps
run, energies, bounds and messages."""
import os
import subprocess
import sys

import numpy as np
import pytest

import newmsm_amd as M
from newmsm_amd import api, problem, registration, synthetic

from helpers import angles
import mplp_literal as ML

pytestmark = pytest.mark.gpu
HCP = dict(rmode=3, lambda_=0.01, mu=0.4, kappa=1.6, k_exp=2.0, rexp=2.0)


def _both(ctx, case, sweeps, **kw):
    U, tc, triplets, start = case
    kw = dict(dict(bounds=True, messages=True), **kw)
    want = api.mplp_optimise(U, tc, triplets, start, sweeps=sweeps, **kw)
    got = api.mplp_optimise_gpu(ctx, U, tc, triplets, start, sweeps=sweeps, **kw)
    ML.same(got, want)
    assert api.mplp_gpu_stats(ctx)["sweeps_run"] == want.sweeps_run
    return got


def _small(triplets, N, L, seed):
    triplets = np.asarray(triplets, dtype=np.int32)
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 1.0, (L, N)), rng.uniform(0.0, 1.0, (len(triplets), L, L, L)), triplets, rng.integers(0, L, N).astype(np.int32)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_one_triplet(ctx, L):
    """T = 1: one level of one workgroup whose L^3 entries are fewer than its threads; the run ends at its fixed point on both sides"""
    got = _both(ctx, _small([[0, 1, 2]], 3, L, 40 + L), 10)
    assert got.sweeps_run <= 3 and api.mplp_gpu_stats(ctx)["levels_per_sweep"] == 1


@pytest.mark.parametrize("L", [16, 19, 20])
def test_ico0_faces(ctx, L):
    """T = 20, 10 sweeps; L^3 a multiple of the workgroup's 256 threads (16) and not (19, 20)"""
    got = _both(ctx, ML.ico_case(0, L), 10)
    stats = api.mplp_gpu_stats(ctx)
    assert got.sweeps_run == 10 and got.labeling.any() and stats["levels_per_sweep"] == 10 and stats["kernel_ms"] > 0


@pytest.mark.parametrize("slots", ["1", "4"])
def test_fewer_copies_of_the_minima_in_lds(ctx, monkeypatch, slots):
    """the update kernel keeps 64 copies of every minimum at 19 labels and a single one from 683 labels on; MSMHIP_MPLP_SLOTS asks for fewer"""
    monkeypatch.setenv("MSMHIP_MPLP_SLOTS", slots)
    assert _both(ctx, ML.ico_case(0, 19), 10).sweeps_run == 10


def test_ico0_faces_61_labels(ctx):
    """L = 61: 3 L = 183 cavities and minima per factor (32 copies of each fit), 226 981 entries"""
    assert _both(ctx, ML.ico_case(0, 61), 3).sweeps_run == 3


@pytest.mark.parametrize("shuffled", [False, True])
def test_ico2_faces(ctx, shuffled):
    """T = 320, L = 19, 5 sweeps; in mesh order (28 levels) and with the triplet list shuffled (another schedule, other incidence orders)"""
    case = ML.ico_case(2, 19, 12, 0.0, False, shuffled)
    got = _both(ctx, case, 5)
    stats = api.mplp_gpu_stats(ctx)
    assert got.labeling.any() and stats["levels_per_sweep"] == len(api.mcmc_schedule(case[2], case[0].shape[1])[2]) - 1
    if not shuffled:
        assert stats["levels_per_sweep"] == 28


def test_ico4_faces(ctx):
    """T = 5120, L = 5, 3 sweeps: 32 levels, the widest of 320 factors"""
    _both(ctx, ML.ico_case(4, 5), 3)
    stats = api.mplp_gpu_stats(ctx)
    assert stats["levels_per_sweep"] == 32 and stats["widest_level"] == 320 and stats["sweeps_run"] == 3


def test_fan_round_one_hub_and_an_isolated_node(ctx):
    """twelve triangles share node 0 (twelve levels of one factor, an incidence list of twelve slots); node 13 is in no triplet and decodes to argmin theta"""
    case = ML.fan_case()
    got = _both(ctx, case, 8)
    assert api.mplp_gpu_stats(ctx)["levels_per_sweep"] == 12 and api.mplp_gpu_stats(ctx)["widest_level"] == 1
    # the isolated node alone, from a start that is its worst label
    U, tc, triplets, start = case
    start = np.array(start)
    start[13] = int(np.argmax(U[:, 13]))
    assert _both(ctx, (U, tc, triplets, start), 2).labeling[13] == int(np.argmin(U[:, 13]))


def test_tables_with_entries_of_1e7(ctx):
    got = _both(ctx, ML.ico_case(0, 19, 13, 0.05), 10)
    assert np.all(np.diff(got.bounds) >= -ML.tol(*ML.ico_case(0, 19, 13, 0.05)[:3]))
    _both(ctx, ML.ico_case(2, 7, 13, 0.05), 5)


def test_whole_number_tables_with_ties(ctx):
    """labels 1 and 2 tie at every node after every sweep: the lowest label on both sides"""
    got = _both(ctx, ML.ico_case(1, 4, 21, 0.0, True), 6)
    assert got.labeling.any() and not np.any(got.labeling == 2)


def test_fixed_points_and_runs_longer_than_a_chunk(ctx):
    """two triangles sharing a node reach their fixed point after some 46 of 200 sweeps (the launches behind it return at once); 300 sweeps of the
    octahedron are more than one chunk of 256"""
    got = _both(ctx, _small([[0, 1, 2], [2, 3, 4]], 5, 3, 1), 200)
    assert 3 < got.sweeps_run < 200
    _both(ctx, _small(ML.OCTAHEDRON, 6, 3, 1), 300)


def test_optional_outputs_and_zero_work(ctx):
    case = ML.ico_case(0, 19)
    U, tc, triplets, start = case
    full = _both(ctx, case, 4)
    ML.same(_both(ctx, case, 4, bounds=False, messages=False), full)        # the bound alone: one pass after the last sweep
    bare = _both(ctx, case, 4, bound=False, bounds=False, messages=False)
    assert bare.bound is None
    ML.same(bare, full)
    none = _both(ctx, case, 0)
    assert np.array_equal(none.labeling, start) and none.sweeps_run == 0
    empty = _both(ctx, (U, np.zeros((0, 19, 19, 19)), np.zeros((0, 3), dtype=np.int32), start), 3)
    assert np.array_equal(empty.labeling, start) and empty.sweeps_run == 0


def test_refusals_are_the_host_literals(ctx):
    U, tc, triplets, start = (np.array(a) for a in ML.ico_case(0, 5, 31))
    _both(ctx, (U, tc, triplets, start), 2)
    before = api.mplp_gpu_stats(ctx)
    bad_label, bad_node, twice = np.array(start), np.array(triplets), np.array(triplets)
    bad_label[7] = 5
    bad_node[11, 2] = U.shape[1]
    twice[4, 2] = twice[4, 0]
    nan_u, inf_t = np.array(U), np.array(tc)
    nan_u[2, 3] = np.nan
    inf_t[19, 4, 4, 4] = -np.inf
    cases = [((U, tc, triplets, bad_label), "MSM_ERR_INVALID.*msm_mcmc_optimise: label of node 7 out of range"),
             ((U, tc, bad_node, start), "MSM_ERR_INVALID.*msm_mcmc_optimise: triplet node out of range"),
             ((U, tc, twice, start), "MSM_ERR_INVALID.*triplet 4 names a node twice"),
             ((nan_u, tc, triplets, start), "MSM_ERR_INVALID.*the unary table holds a non-finite value.*--fixnan"),
             ((U, inf_t, triplets, start), "MSM_ERR_INVALID.*the triplet table holds a non-finite value.*--fixnan"),
             ((np.zeros((1025, 3)), np.zeros((0, 1, 1, 1)), np.zeros((0, 3), dtype=np.int32), np.zeros(3, dtype=np.int32)), "MSM_ERR_CAPACITY.*1025 labels")]
    for args, pattern in cases:
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise_gpu(ctx, *args, sweeps=3)
    assert api.mplp_gpu_stats(ctx) == before  # no sweep ran in between
    _both(ctx, (U, tc, triplets, start), 2)    # and the context is as good as before


def test_every_non_finite_entry_is_refused_by_its_table(ctx):
    """the device's one classification pass read the plain way: the host literal's refusals (test_mplp_cpu.py), and no sweep runs"""
    ok = ML.ico_case(0, 5, 31)
    _both(ctx, ok, 2)
    before = api.mplp_gpu_stats(ctx)
    for args, pattern in ML.non_finite_refusals():
        with pytest.raises(M.MsmError, match=pattern):
            api.mplp_optimise_gpu(ctx, *args, sweeps=3)
    assert api.mplp_gpu_stats(ctx) == before
    _both(ctx, ok, 2)


@pytest.mark.parametrize("kind", ["univariate", "ho_univariate"])
def test_cost_function_tables_stay_on_the_device(ctx, kind):
    """msm_cost_mplp_optimise = computeUnaryCosts + computeTripletCosts + the host literal; twice in a row"""
    inp = problem.pairwise_inputs(data_order=4, cp_order=2, D=1)
    cf, keep = problem.build_cost(ctx, inp, kind=kind, **HCP)
    cf.get_source_data()
    start = np.zeros(cf.N, dtype=np.int32)
    kw = dict(sweeps=5, bounds=True, messages=True)
    want = api.mplp_optimise(cf.computeUnaryCosts(), cf.computeTripletCosts(), inp["triplets"], start, **kw)
    assert want.labeling.any() and want.energy <= want.energies.min() and want.bound <= want.energy
    ML.same(cf.mplp_optimise(start, **kw), want)
    ML.same(cf.mplp_optimise(start, **kw), want)
    with pytest.raises(M.MsmError, match="msm_mcmc_optimise: label of node 3 out of range"):
        bad = np.array(start)
        bad[3] = cf.L
        cf.mplp_optimise(bad, **kw)
    cf.close()


def test_level_loop(ctx):
    """run_discrete_level(optimiser="mplp"): with the tables on the device, the labellings, energies and coordinates of the fetched-table route"""
    xyz, tri = M.make_mesh_from_icosa(4)
    ref = synthetic.features(xyz, 1, 21)
    src = synthetic.features(synthetic.known_warp(xyz, seed=23, rot_deg=4.0, amp=2.5), 1, 21)
    # labeldist 0.4: at the default 0.5 the sampling grid's own vertices, which every second iteration takes as labels, let neighbouring control points
    # meet; the collapsed triangles make the regulariser non-finite and the optimiser refuses such a table (as it does for both routes)
    kw = dict(cp_order=2, iters=3, mciters=5, seed=5, kind="univariate", optimiser="mplp", cost_params=dict(lambda_=0.0005), labeldist=0.4)
    t_gpu, t_host = {}, {}
    got = registration.run_discrete_level(registration.ProductOps(ctx), xyz, tri, ref, xyz, tri, src, xyz, timings=t_gpu, **kw)
    want = registration.run_discrete_level(registration.ProductOps(ctx, mplp_gpu=False), xyz, tri, ref, xyz, tri, src, xyz, timings=t_host, **kw)
    assert "triplet_table" not in t_gpu and "unary_table" not in t_gpu and "optimiser" in t_gpu  # neither table was fetched
    assert "triplet_table" in t_host and "unary_table" in t_host
    assert len(got[3]) == 3 and all(np.array_equal(a, b) for a, b in zip(got[3], want[3])) and all(l.any() for l in got[3])
    assert got[2] == want[2] and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


CONF = ("--simval=2,2\n--sigma_in=2,2\n--sigma_ref=2,2\n--lambda=0.2,0.2\n--it=2,2\n--opt=DISCRETE,DISCRETE\n--CPgrid=2,3\n--SGgrid=4,5\n--datagrid=4,5\n"
        "--regoption=3\n--regexp=2\n--dopt=MPLP\n--VN\n--k_exponent=2\n--bulkmod=1.6\n--shearmod=0.4\n--rescaleL\n--mciters=5,5\n")


def test_both_executables(ctx, tmp_path):
    """MSMHIP_MPLP=on: tools/register_files.py and tools/cpp/newmsm write the same bytes for a two-level --dopt=MPLP configuration; without the variable
    both end with the reference's message and exit status 1"""
    import __graft_entry__ as g
    from newmsm_amd import meshio

    exe = g.build_cpp_newmsm()
    xyz, tri = M.make_mesh_from_icosa(5)
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
    plain = {k: v for k, v in os.environ.items() if k != "MSMHIP_MPLP"}
    names = ["sphere.reg.surf.gii", "sphere.LR.reg.surf.gii", "transformed_and_reprojected.func.gii"]
    for tag, cmd in (("py.", [sys.executable, "tools/register_files.py"]), ("cpp.", [exe])):
        off = subprocess.run(cmd + common + ["--out=" + d + "off." + tag], cwd=root, env=plain, capture_output=True, text=True, timeout=600)
        assert off.returncode == 1 and "Unrecognized optimiser" in off.stdout + off.stderr, (off.returncode, off.stdout, off.stderr)
        assert not any(os.path.exists(d + "off." + tag + n) for n in names)
        run = subprocess.run(cmd + common + ["--out=" + d + tag], cwd=root, env=dict(plain, MSMHIP_MPLP="on"), capture_output=True, text=True, timeout=600)
        assert run.returncode == 0, run.stderr
    for n in names:
        with open(d + "py." + n, "rb") as fa, open(d + "cpp." + n, "rb") as fb:
            assert fa.read() == fb.read(), "%s differs between the two executables" % n
    reg, _ = meshio.load_surface(d + "cpp.sphere.reg.surf.gii")
    assert angles(reg, meshio.load_surface(d + "in.surf.gii")[0]).max() > 1e-4  # something was registered
